// Motion-compensated frame interpolation on the dense flows (oflk_interpolate_frames): the kernel.  Included by oflk.hip
// after oflk_kernels.hpp, whose sample (lean_taps_at / lean_load / lean_finish) and forward-backward test (fb_finish) it uses.
#pragma once

namespace oflk {

// ---------------------------------------------------------------------------
// The statement (include/oflk.h, tests/interp_model.py).  Pair b has frames A = frame b and B = frame b+1, F = (uf, vf) the
// flow A -> B and G = (ub, vb) the flow B -> A; tau in (0, 1) is the output time.  sample(img, x, y) is warp_image's bilinear
// sample at one float64 point with a float32 result; a coordinate that is not inside [0, W-1] x [0, H-1] (NaN and the
// infinities included) samples as 0 and reads no tap of its own: lean_taps_at turns it into offset 0 and lean_finish into
// the value 0, so that a flow value never becomes an address.  Every operation is rounded on its own.  For output pixel
// (x, y) and R = refine:
//   side(img, F, G, s):   px = f64(x); py = f64(y)
//                         R times:  us = sample(F.u, px, py); vs = sample(F.v, px, py)
//                                   px = f64(x) - s * f64(us); py = f64(y) - s * f64(vs)
//                         us, vs = samples of F at (px, py);  qx = px + f64(us); qy = py + f64(vs)
//                         bu, bv = samples of G at (qx, qy);  e2, m2 as fb_finish
//                         ok = inside(px, py) and inside(qx, qy) and e2 <= alpha*m2 + beta;  value = sample(img, px, py)
//   a, ok_a = side(A, F, G, tau);  b, ok_b = side(B, G, F, 1.0 - tau);  t = f32(tau)
//   both: a + t*(b - a);  only ok_a: a;  only ok_b: b;  neither: A[y][x] + t*(B[y][x] - A[y][x]);  status = ok_a | ok_b << 1
//   uint8 frames: (unsigned char)rintf(out), half to even
// lean_taps_at reads the sign bit for its range test, so a coordinate of -0 would count as outside where the statement's
// closed comparison takes it: none arises here.  px = f64(x) - t with x >= 0 is -0 only for x = -0, which no pixel index
// is, and qx = px + f64(us) is -0 only when both terms are.
//
// One thread per output pixel of one slice; slice z = b * n + j is time tau[j] of pair b, so that the n times of a pair
// are adjacent slices that run while its flows are in L2.  Both sides' chains are independent and written side by side:
// each of the R + 1 flow rounds has the eight gathers of both sides in flight together, then the eight of the partner
// flows, then the four of the two frames.  Unique bytes per output pixel: (16 B of flows + two pixels) / n read, one pixel
// and one status byte written.  Gathers per output pixel: 2 sides x ((R + 2) flow samples x 2 planes + 1 frame sample)
// x 2 row pairs = 8 R + 20 pair loads, 36 at R = 2, nearly all of them L1 / L2 hits next to the pixel.
// The taus travel in the launch arguments (a uniform index into them is a scalar load).
// ---------------------------------------------------------------------------
struct InterpArgs {
    const void *frames;               // [B+1][H][W] float32 or uint8
    const float *uf, *vf, *ub, *vb;   // [B][H][W]
    void *out;                        // [B][n][H][W] of the frames' type
    unsigned char *status;            // [B][n][H][W] or NULL
    int H, W, n;
    unsigned z0;                      // first slice of this launch, counted from the first time of the arrays' first pair
                                      // (< n: the launcher cuts B * n slices at the grid's z limit and moves the arrays)
    int refine;
    float alpha, beta;
    double tau[OFLK_INTERP_MAX_TAUS];
};

// both components of a flow at one point: taps, four pair loads
template <bool NARROW>
__device__ __forceinline__ void interp_flow(const LeanGeom &lg, const float *u, const float *v, double py, double px,
                                            LeanTaps &t, float &us, float &vs)
{
    t = lean_taps_at(lg, py, px);
    PairF u0, u1, v0, v1;
    lean_load<NARROW>(lg, u, t, u0, u1);
    lean_load<NARROW>(lg, v, t, v0, v1);
    us = lean_finish(t, u0, u1);
    vs = lean_finish(t, v0, v1);
}

template <class PIX, bool STATUS, bool NARROW>
__global__ __launch_bounds__(256) void k_interp(InterpArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const unsigned z = a.z0 + blockIdx.z, b = z / (unsigned)a.n, j = z - b * (unsigned)a.n;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const size_t fo = (size_t)b * plane, cell = (size_t)y * a.W + x;
    const float *uf = a.uf + fo, *vf = a.vf + fo, *ub = a.ub + fo, *vb = a.vb + fo;
    const PIX *fa = static_cast<const PIX *>(a.frames) + fo, *fb = fa + plane;
    const LeanGeom lg = lean_geom(a.H, a.W);
    const double tau = a.tau[j];
    const double sa = tau, sb = 1.0 - tau;
    const double xd = (double)x, yd = (double)y;

    // the fixed-point solves of p + s F(p) = (x, y) on both sides, then the flow at the solved points
    double pxa = xd, pya = yd, pxb = xd, pyb = yd;
    LeanTaps ta, tb;
    float usa, vsa, usb, vsb;
    for (int r = 0; r < a.refine; r++) {
        interp_flow<NARROW>(lg, uf, vf, pya, pxa, ta, usa, vsa);
        interp_flow<NARROW>(lg, ub, vb, pyb, pxb, tb, usb, vsb);
        pxa = xd - sa * (double)usa;
        pya = yd - sa * (double)vsa;
        pxb = xd - sb * (double)usb;
        pyb = yd - sb * (double)vsb;
    }
    interp_flow<NARROW>(lg, uf, vf, pya, pxa, ta, usa, vsa);
    interp_flow<NARROW>(lg, ub, vb, pyb, pxb, tb, usb, vsb);

    // the frames at the solved points, and the partner flows where those points lie in the other frame
    PairF a0, a1, b0, b1;
    lean_load<NARROW, PIX>(lg, fa, ta, a0, a1);
    lean_load<NARROW, PIX>(lg, fb, tb, b0, b1);
    const LeanTaps qa = lean_taps_at(lg, pya + (double)vsa, pxa + (double)usa);
    const LeanTaps qb = lean_taps_at(lg, pyb + (double)vsb, pxb + (double)usb);
    PairF g0, g1, g2, g3, f0, f1, f2, f3;
    lean_load<NARROW>(lg, ub, qa, g0, g1);
    lean_load<NARROW>(lg, vb, qa, g2, g3);
    lean_load<NARROW>(lg, uf, qb, f0, f1);
    lean_load<NARROW>(lg, vf, qb, f2, f3);
    const float pa = ld_pix<PIX>(fa, (unsigned)cell), pb = ld_pix<PIX>(fb, (unsigned)cell);   // cell < 2^30 (host check)

    float e;
    unsigned char oka, okb;
    fb_finish(usa, vsa, qa, g0, g1, g2, g3, a.alpha, a.beta, e, oka);
    fb_finish(usb, vsb, qb, f0, f1, f2, f3, a.alpha, a.beta, e, okb);
    oka = (oka && ta.inside) ? 1 : 0;
    okb = (okb && tb.inside) ? 1 : 0;
    // + 0: the sum of a sample starts at its first term (lean_finish), map_coordinates' at +0, which shows in the sign of
    // a zero that is written out as it is
    const float va = lean_finish(ta, a0, a1) + 0.0f, vb_ = lean_finish(tb, b0, b1) + 0.0f;
    const float t = (float)tau;
    const float lo = (oka | okb) ? va : pa, hi = (oka | okb) ? vb_ : pb;
    float r = lo + t * (hi - lo);
    if (oka != okb) r = oka ? va : vb_;

    const size_t o = (size_t)z * plane + cell;
    if constexpr (sizeof(PIX) == 1) static_cast<unsigned char *>(a.out)[o] = (unsigned char)rintf(r);
    else static_cast<float *>(a.out)[o] = r;
    if constexpr (STATUS) a.status[o] = (unsigned char)(oka | (okb << 1));
}
}  // namespace oflk
