// Motion-compensated temporal denoising on the dense flows (oflk_denoise_frames_host, oflk_denoise_sequence): the kernel.
// Included by oflk.hip after oflk_interp.hpp: the sample (lean_taps_at / lean_load / lean_finish) and the forward-backward
// test (fb_finish) are oflk_kernels.hpp's, used as they are.
#pragma once

namespace oflk {

// ---------------------------------------------------------------------------
// The statement (include/oflk.h, tests/denoise_model.py).  Frames [T][H][W] float32 or uint8; F_s = (uf[s], vf[s]) the flow
// frame s -> s+1 and G_s = (ub[s], vb[s]) the flow s+1 -> s; R = radius in [1, 4]; h2 = f32(strength) * f32(strength).
// sample and inside are the interpolation's: a point that is not inside [0, W-1] x [0, H-1] (NaN and the infinities
// included) samples as 0 and reads no tap.  Every operation is rounded on its own.  For output frame t, pixel (x, y):
//   c = f32(frame[t][y][x]);  num = c;  den = 1.0f;  count = 0
//   two chains, backward (sgn = -1) and forward (sgn = +1), each: (px, py) = (f64(x), f64(y)), alive
//   for k = 1 .. R:   for sgn in (-1, +1), in this order:
//     s' = t + sgn*k;  the chain has ended, or s' < 0, or s' > T-1: nothing
//     forward:  (A, B) = (F_{s'-1}, G_{s'-1});   backward: (A, B) = (G_{s'}, F_{s'})
//     us = sample(A.u, px, py); vs = sample(A.v, px, py);  qx = px + f64(us); qy = py + f64(vs)
//     bu, bv = samples of B at (qx, qy);  e2, m2 as fb_finish;  ok = inside(qx, qy) and e2 <= alpha*m2 + beta
//     not ok: the chain ends
//     ok: (px, py) = (qx, qy);  v = sample(frame[s'], qx, qy);  d = v - c;  w = 1.0f - (d*d) / h2
//         if w > 0:  num = num + w*v;  den = den + w;  count += 1        (a NaN w is not > 0)
//   out = num / den;  uint8 frames: out clamped to [0, 255], then (unsigned char)rintf(out), half to even
// This is the interpolation's side test with the point carried from frame to frame.
//
// -0 and lean_taps_at's sign-bit range test, re-argued for the chained point.  The test reads a coordinate of -0 as outside
// where the statement's closed comparison takes it as inside, so none may arise.  A chain starts at px = f64(x) with x a
// pixel index, which is +0 or positive.  A step forms qx = px + f64(us): a sum of two doubles is -0 only when both terms are
// -0 (x + (-x) is +0 under round to nearest), and px is not.  The next step's px is a qx that passed the test, hence again
// +0 or positive: by induction no px and no qx of a chain is -0.  The same holds for py and qy.
//
// No load leaves its plane: every tap offset is lean_taps_at's (an outside point gives offset 0), added to the base of one
// frame or flow plane whose slot the block-uniform frame index picks; a chain that has ended, or whose next frame lies
// outside the sequence, issues no load at all (its lanes are masked off the gathers).
//
// One lane per output pixel of one output frame, k_interp's 64 x 4 block; the frames of a launch lie along grid.z.  The two
// chains are independent and written side by side: each of the R steps has both directions' eight pair loads of A in
// flight together, then the eight of B and the four of the two frames, whose taps are B's (the point q).  Gathers per output
// pixel: 2 directions x R steps x (4 of A + 4 of B + 2 of the frame) = 20 R pair loads (36 for interpolation at refine 2),
// nearly all of them L1 / L2 hits next to the pixel; unique bytes per output pixel are (2 R + 1) pixels and 16 B x 2 R of
// flows read, shared by the 2 R + 1 output frames that use them, and one pixel and one count byte written.
//
// The arrays are rings, so that a chunked sequence call keeps only the window it needs: frame s lies in slot s % fcap,
// pair s in slot s % pcap (the host form passes fcap = T and pcap = T - 1: slot s is s).
// ---------------------------------------------------------------------------
struct DenoiseArgs {
    const void *frames;               // fcap slots [H][W] float32 or uint8
    const float *uf, *vf, *ub, *vb;   // pcap slots [H][W]
    void *out;                        // [n][H][W] of the frames' type: output frame t0 + z at z
    unsigned char *count;             // [n][H][W] or NULL
    int H, W;
    int T;                            // frames of the sequence: the chains end at frames 0 and T - 1
    int t0;                           // the sequence index of this launch's first output frame
    int fcap, pcap;
    int radius;
    float alpha, beta, h2;
};

// One chain of a pixel: the carried point, whether it is alive, and what a step leaves behind for the next phase
struct DenoiseChain {
    double px, py;
    bool alive;
    bool go;          // this step runs: alive and its frame is in the sequence
    LeanTaps tq;      // the taps of q
    float us, vs;
    double qx, qy;
};

// the four pair loads of both components of a flow at the taps t
template <bool NARROW>
__device__ __forceinline__ void denoise_load_flow(const LeanGeom &lg, const float *u, const float *v, const LeanTaps &t, PairF &u0,
                                                  PairF &u1, PairF &v0, PairF &v1)
{
    lean_load<NARROW>(lg, u, t, u0, u1);
    lean_load<NARROW>(lg, v, t, v0, v1);
}

template <class PIX, bool COUNT, bool NARROW>
__global__ __launch_bounds__(256) void k_denoise(DenoiseArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const int t = a.t0 + (int)blockIdx.z;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const unsigned cell = (unsigned)y * (unsigned)a.W + (unsigned)x;   // < 2^30 (host check)
    const PIX *frames = static_cast<const PIX *>(a.frames);
    const LeanGeom lg = lean_geom(a.H, a.W);

    const float c = ld_pix<PIX>(frames + (size_t)(t % a.fcap) * plane, cell);
    float num = c, den = 1.0f;
    unsigned cnt = 0;
    DenoiseChain bw, fw;
    bw.px = fw.px = (double)x;
    bw.py = fw.py = (double)y;
    bw.alive = fw.alive = true;

    for (int k = 1; k <= a.radius; k++) {
        // block-uniform: the frames of this step and the pairs between them and the frames before
        const int sb = t - k, sf = t + k;
        const bool in_b = sb >= 0, in_f = sf <= a.T - 1;
        if (!in_b && !in_f) break;
        const size_t ob = (size_t)((in_b ? sb : 0) % a.pcap) * plane, of = (size_t)((in_f ? sf - 1 : 0) % a.pcap) * plane;
        const PIX *img_b = frames + (size_t)((in_b ? sb : 0) % a.fcap) * plane;
        const PIX *img_f = frames + (size_t)((in_f ? sf : 0) % a.fcap) * plane;
        bw.go = bw.alive && in_b;
        fw.go = fw.alive && in_f;

        // A at the carried points: backward G_{sb}, forward F_{sf-1}.  Only the loads are under a lane's `go`: the taps and
        // the sums around them are formed for every lane (a lane that does not run holds zeros and its last point, and what
        // it forms is not used).  The lanes whose two chains both run -- nearly all of them away from the ends of the
        // sequence -- take one branch that issues both directions' loads, so that they are in flight together: loads under
        // a branch of their own are waited for inside it, before the other direction's could be issued.
        const PairF zero{0.0f, 0.0f};
        const LeanTaps tb = lean_taps_at(lg, bw.py, bw.px), tf = lean_taps_at(lg, fw.py, fw.px);
        PairF g0 = zero, g1 = zero, g2 = zero, g3 = zero, i0 = zero, i1 = zero;
        PairF f0 = zero, f1 = zero, f2 = zero, f3 = zero, j0 = zero, j1 = zero;
        if (bw.go && fw.go) {
            denoise_load_flow<NARROW>(lg, a.ub + ob, a.vb + ob, tb, g0, g1, g2, g3);
            denoise_load_flow<NARROW>(lg, a.uf + of, a.vf + of, tf, f0, f1, f2, f3);
        } else if (bw.go) {
            denoise_load_flow<NARROW>(lg, a.ub + ob, a.vb + ob, tb, g0, g1, g2, g3);
        } else if (fw.go) {
            denoise_load_flow<NARROW>(lg, a.uf + of, a.vf + of, tf, f0, f1, f2, f3);
        }
        bw.us = lean_finish(tb, g0, g1); bw.vs = lean_finish(tb, g2, g3);
        fw.us = lean_finish(tf, f0, f1); fw.vs = lean_finish(tf, f2, f3);

        // B and the frame at q: backward F_{sb} and frame sb, forward G_{sf-1} and frame sf
        bw.qx = bw.px + (double)bw.us; bw.qy = bw.py + (double)bw.vs;
        fw.qx = fw.px + (double)fw.us; fw.qy = fw.py + (double)fw.vs;
        bw.tq = lean_taps_at(lg, bw.qy, bw.qx);
        fw.tq = lean_taps_at(lg, fw.qy, fw.qx);
        g0 = g1 = g2 = g3 = f0 = f1 = f2 = f3 = zero;
        if (bw.go && fw.go) {
            denoise_load_flow<NARROW>(lg, a.uf + ob, a.vf + ob, bw.tq, g0, g1, g2, g3);
            denoise_load_flow<NARROW>(lg, a.ub + of, a.vb + of, fw.tq, f0, f1, f2, f3);
            lean_load<NARROW, PIX>(lg, img_b, bw.tq, i0, i1);
            lean_load<NARROW, PIX>(lg, img_f, fw.tq, j0, j1);
        } else if (bw.go) {
            denoise_load_flow<NARROW>(lg, a.uf + ob, a.vf + ob, bw.tq, g0, g1, g2, g3);
            lean_load<NARROW, PIX>(lg, img_b, bw.tq, i0, i1);
        } else if (fw.go) {
            denoise_load_flow<NARROW>(lg, a.ub + of, a.vb + of, fw.tq, f0, f1, f2, f3);
            lean_load<NARROW, PIX>(lg, img_f, fw.tq, j0, j1);
        }

        // the test, the carried point and the weighted sample: backward first, as the statement sums
        float e;
        unsigned char ok;
        fb_finish(bw.us, bw.vs, bw.tq, g0, g1, g2, g3, a.alpha, a.beta, e, ok);
        bw.alive = bw.go && ok;
        if (bw.alive) {
            bw.px = bw.qx; bw.py = bw.qy;
            // + 0: a sample's sum starts at its first term (lean_finish), map_coordinates' at +0, which shows in the sign of a
            // zero that reaches num
            const float v = lean_finish(bw.tq, i0, i1) + 0.0f, d = v - c, w = 1.0f - (d * d) / a.h2;
            if (w > 0.0f) { num = num + w * v; den = den + w; cnt++; }
        }
        fb_finish(fw.us, fw.vs, fw.tq, f0, f1, f2, f3, a.alpha, a.beta, e, ok);
        fw.alive = fw.go && ok;
        if (fw.alive) {
            fw.px = fw.qx; fw.py = fw.qy;
            const float v = lean_finish(fw.tq, j0, j1) + 0.0f, d = v - c, w = 1.0f - (d * d) / a.h2;
            if (w > 0.0f) { num = num + w * v; den = den + w; cnt++; }
        }
    }

    const float r = num / den;
    const size_t o = (size_t)blockIdx.z * plane + cell;
    if constexpr (sizeof(PIX) == 1) static_cast<unsigned char *>(a.out)[o] = (unsigned char)rintf(fminf(fmaxf(r, 0.0f), 255.0f));
    else static_cast<float *>(a.out)[o] = r;
    if constexpr (COUNT) a.count[o] = (unsigned char)cnt;
}
}  // namespace oflk
