// Motion-compensated frame interpolation on the dense flows (oflk_interpolate_frames and its packed and NV12 forms): the
// kernels.  Included by oflk.hip after oflk_kernels.hpp, whose sample (lean_taps_at / lean_load / lean_finish) and
// forward-backward test (fb_finish) they use, and after oflk_colour.hpp (ld_tap) and oflk_nv12.hpp (TapPair).
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

// What a pixel's two solves leave behind: the solved points, their taps in the H x W frame, the flows there and the two ok
// bits (the forward-backward test and both inside tests)
struct InterpSolve {
    double pxa, pya, pxb, pyb;
    LeanTaps ta, tb;
    float usa, vsa, usb, vsb;
    unsigned char oka, okb;
};

// The statement's two sides from the start position (xd, yd), up to the ok bits: the fixed-point solves of
// p + s F(p) = (xd, yd), the flows at the solved points, the partner flows where those points lie in the other frame and the
// test.  The grey pixels start at (x, y), the chroma samples of an NV12 frame at their luma position.  gather(s) runs once the
// solved points' taps are known: there the caller issues its frame gathers, which are then in flight together with the
// eight of the partner flows.
template <bool NARROW, class GATHER>
__device__ __forceinline__ InterpSolve interp_solve(const LeanGeom &lg, const float *uf, const float *vf, const float *ub,
                                                    const float *vb, int refine, float alpha, float beta, double tau, double xd,
                                                    double yd, GATHER &&gather)
{
    const double sa = tau, sb = 1.0 - tau;
    InterpSolve s;
    s.pxa = xd; s.pya = yd; s.pxb = xd; s.pyb = yd;
    for (int r = 0; r < refine; r++) {
        interp_flow<NARROW>(lg, uf, vf, s.pya, s.pxa, s.ta, s.usa, s.vsa);
        interp_flow<NARROW>(lg, ub, vb, s.pyb, s.pxb, s.tb, s.usb, s.vsb);
        s.pxa = xd - sa * (double)s.usa;
        s.pya = yd - sa * (double)s.vsa;
        s.pxb = xd - sb * (double)s.usb;
        s.pyb = yd - sb * (double)s.vsb;
    }
    interp_flow<NARROW>(lg, uf, vf, s.pya, s.pxa, s.ta, s.usa, s.vsa);
    interp_flow<NARROW>(lg, ub, vb, s.pyb, s.pxb, s.tb, s.usb, s.vsb);

    gather(s);
    const LeanTaps qa = lean_taps_at(lg, s.pya + (double)s.vsa, s.pxa + (double)s.usa);
    const LeanTaps qb = lean_taps_at(lg, s.pyb + (double)s.vsb, s.pxb + (double)s.usb);
    PairF g0, g1, g2, g3, f0, f1, f2, f3;
    lean_load<NARROW>(lg, ub, qa, g0, g1);
    lean_load<NARROW>(lg, vb, qa, g2, g3);
    lean_load<NARROW>(lg, uf, qb, f0, f1);
    lean_load<NARROW>(lg, vf, qb, f2, f3);

    float e;
    fb_finish(s.usa, s.vsa, qa, g0, g1, g2, g3, alpha, beta, e, s.oka);
    fb_finish(s.usb, s.vsb, qb, f0, f1, f2, f3, alpha, beta, e, s.okb);
    s.oka = (s.oka && s.ta.inside) ? 1 : 0;
    s.okb = (s.okb && s.tb.inside) ? 1 : 0;
    return s;
}

// the statement's blend of the two sides' values va, vb and of the frames' own values pa, pb at the output position
__device__ __forceinline__ float interp_blend(unsigned char oka, unsigned char okb, float va, float vb, float pa, float pb, float t)
{
    const float lo = (oka | okb) ? va : pa, hi = (oka | okb) ? vb : pb;
    float r = lo + t * (hi - lo);
    if (oka != okb) r = oka ? va : vb;
    return r;
}

// One output pixel (x, y) of slice z of a grey plane: the grey kernel's body, and the Y plane's of an NV12 frame.  Frames lie
// `fstride` pixels apart and output slices `ostride`; the flows and the status are H W apart.
template <class PIX, bool STATUS, bool NARROW>
__device__ __forceinline__ void interp_plane(const InterpArgs &a, int x, int y, unsigned z, size_t fstride, size_t ostride)
{
    const unsigned b = z / (unsigned)a.n, j = z - b * (unsigned)a.n;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const size_t fo = (size_t)b * plane, cell = (size_t)y * a.W + x;
    const float *uf = a.uf + fo, *vf = a.vf + fo, *ub = a.ub + fo, *vb = a.vb + fo;
    const PIX *fa = static_cast<const PIX *>(a.frames) + (size_t)b * fstride, *fb = fa + fstride;
    const LeanGeom lg = lean_geom(a.H, a.W);
    const double tau = a.tau[j];

    // the frames at the solved points
    PairF a0, a1, b0, b1;
    const InterpSolve s = interp_solve<NARROW>(lg, uf, vf, ub, vb, a.refine, a.alpha, a.beta, tau, (double)x, (double)y,
                                               [&](const InterpSolve &p) {
                                                   lean_load<NARROW, PIX>(lg, fa, p.ta, a0, a1);
                                                   lean_load<NARROW, PIX>(lg, fb, p.tb, b0, b1);
                                               });
    const float pa = ld_pix<PIX>(fa, (unsigned)cell), pb = ld_pix<PIX>(fb, (unsigned)cell);   // cell < 2^30 (host check)
    // + 0: the sum of a sample starts at its first term (lean_finish), map_coordinates' at +0, which shows in the sign of
    // a zero that is written out as it is
    const float va = lean_finish(s.ta, a0, a1) + 0.0f, vb_ = lean_finish(s.tb, b0, b1) + 0.0f;
    const float r = interp_blend(s.oka, s.okb, va, vb_, pa, pb, (float)tau);

    if constexpr (sizeof(PIX) == 1) static_cast<unsigned char *>(a.out)[(size_t)z * ostride + cell] = (unsigned char)rintf(r);
    else static_cast<float *>(a.out)[(size_t)z * ostride + cell] = r;
    if constexpr (STATUS) a.status[(size_t)z * plane + cell] = (unsigned char)(s.oka | (s.okb << 1));
}

template <class PIX, bool STATUS, bool NARROW>
__global__ __launch_bounds__(256) void k_interp(InterpArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    interp_plane<PIX, STATUS, NARROW>(a, x, y, a.z0 + blockIdx.z, plane, plane);
}

// ---------------------------------------------------------------------------
// Packed colour: frames [B+1][H][W][C] bytes, C = 3 or 4, out [B][n][H][W][C].  Every channel is the uint8 grey statement on
// its plane under the same flows, and ok depends on the flows only: the solve, the ok bits and the two sets of bilinear
// weights are formed once per pixel and lean_finish runs C times on them.  k_interp's grid, lane shape and slice order.  A
// tap is one dword that holds all channels of its pixel (ld_tap, oflk_colour.hpp: the frame's last pixel of C = 3 is read as
// the dword that ends with it, so no load leaves [H][W][C] of its own frame); a tap pair of the grey kernel is the pixels
// off0 / 4 and off0 / 4 + 1, which lean_taps_at keeps inside the frame for H, W >= 2 (the floor is capped at N - 2; a point
// outside reads pixel 0's taps).  Gathers per output pixel: 8 R + 16 pair loads of the flows and 10 dwords of the frames,
// against 3 (8 R + 20) pair loads of three planar calls.
// The store: a pixel a lane.  C = 4 with VEC (out 4-byte aligned): one dword; everything else byte by byte, as the packed
// warp's unaligned form does.
// ---------------------------------------------------------------------------
template <int C, bool STATUS, bool VEC>
__global__ __launch_bounds__(256) void k_interp_packed(InterpArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const unsigned z = a.z0 + blockIdx.z, b = z / (unsigned)a.n, j = z - b * (unsigned)a.n;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const size_t fo = (size_t)b * plane;
    const unsigned cell = (unsigned)y * (unsigned)a.W + (unsigned)x, last = (unsigned)plane - 1u;
    const unsigned char *fa = static_cast<const unsigned char *>(a.frames) + fo * C, *fb = fa + plane * C;
    const LeanGeom lg = lean_geom(a.H, a.W);
    const double tau = a.tau[j];

    unsigned qa[4], qb[4];   // the taps of both sides: row 0 left, right, row 1 left, right
    const InterpSolve s = interp_solve<false>(lg, a.uf + fo, a.vf + fo, a.ub + fo, a.vb + fo, a.refine, a.alpha, a.beta, tau,
                                              (double)x, (double)y, [&](const InterpSolve &p) {
                                                  const unsigned a0 = p.ta.off0 >> 2, a1 = (p.ta.off0 + lg.rowstep) >> 2;
                                                  const unsigned b0 = p.tb.off0 >> 2, b1 = (p.tb.off0 + lg.rowstep) >> 2;
                                                  qa[0] = ld_tap<C>(fa, a0, last); qa[1] = ld_tap<C>(fa, a0 + 1u, last);
                                                  qa[2] = ld_tap<C>(fa, a1, last); qa[3] = ld_tap<C>(fa, a1 + 1u, last);
                                                  qb[0] = ld_tap<C>(fb, b0, last); qb[1] = ld_tap<C>(fb, b0 + 1u, last);
                                                  qb[2] = ld_tap<C>(fb, b1, last); qb[3] = ld_tap<C>(fb, b1 + 1u, last);
                                              });
    const unsigned pa = ld_tap<C>(fa, cell, last), pb = ld_tap<C>(fb, cell, last);
    const float t = (float)tau;
    auto ch = [](unsigned p, int c) { return (float)((p >> (8 * c)) & 0xffu); };
    unsigned px = 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float va = lean_finish(s.ta, PairF{ch(qa[0], c), ch(qa[1], c)}, PairF{ch(qa[2], c), ch(qa[3], c)}) + 0.0f;
        const float vb = lean_finish(s.tb, PairF{ch(qb[0], c), ch(qb[1], c)}, PairF{ch(qb[2], c), ch(qb[3], c)}) + 0.0f;
        px |= (unsigned)(unsigned char)rintf(interp_blend(s.oka, s.okb, va, vb, ch(pa, c), ch(pb, c), t)) << (8 * c);
    }
    const size_t o = (size_t)z * plane + cell;
    unsigned char *dst = static_cast<unsigned char *>(a.out) + o * C;
    if constexpr (VEC && C == 4) {
        *reinterpret_cast<unsigned *>(dst) = px;
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] = (unsigned char)(px >> (8 * c));
    }
    if constexpr (STATUS) a.status[o] = (unsigned char)(s.oka | (s.okb << 1));
}

// ---------------------------------------------------------------------------
// NV12: frames [B+1][H W 3 / 2] (Y[H][W], then UV[H/2][W/2][2]), out [B][n][H W 3 / 2], status [B][n][H][W].  One launch for
// both planes of the slices, k_warp_nv12's block split (oflk_nv12.hpp) at one pixel a lane: blocks with blockIdx.x <
// luma_groups do interp_plane on the Y planes, which lie H W 3 / 2 bytes apart; the blocks above count the (row group,
// column block) pairs of the CH x CW = H/2 x W/2 chroma plane row group first.
// The chroma statement (include/oflk.h): sample (i, j) sits at the luma position (X, Y) = (f64(2 i) + sx, f64(2 j) + sy),
// both exact, and runs the grey solve from there on the luma flows with the luma frame's inside tests, which gives (px, py)
// and ok of both sides.  A side's value for U and for V is sample(P_c, cx, cy) on the CH x CW plane with
// cx = clamp(0.5 * (px - sx), 0, CW - 1), cy = clamp(0.5 * (py - sy), 0, CH - 1): a point inside the luma frame lies up to half
// a chroma sample beyond the chroma plane's last row or column (and before its first for sy = 0.5), and the sample's cval 0
// there would be saturated green.  A chroma lane does that one solve, gathers each tap as one 2-byte load that holds U and V
// (TapPair) and runs lean_finish for U and for V on the one set of weights.  Where (px, py) is not inside the luma frame
// ok is 0, the value is not used and the taps are pair 0's, as an outside point's of the grey kernel.
//
// -0 and lean_taps_at's sign-bit range test.  The start: X = f64(2 i) + sx is +0 or at least 0.5, never -0, so the grey note
// holds as it stands: px = X - t is -0 only for X = -0, and qx = px + f64(us) only when both terms are.  The chroma point, for
// (px, py) inside the luma frame (any other is not used): px >= +0, and sx is +0 or 0.5.  d = px - sx is +0 where the two
// are equal, positive where px > sx, and for px in [0, 0.5) against sx = 0.5 at most -2^-54; so 0.5 * d is exact, never -0,
// and where it is negative the clamp's `v < lo ? lo` makes it lo = +0.  (A -0 would pass the clamp, -0 < 0 being false, and
// read as outside; none reaches it.)  NaN passes the clamp as NaN, but a NaN point is not inside the luma frame.  The same
// holds for cy.
//
// No load leaves its frame: Y taps as in the grey kernel inside [H][W]; the UV plane begins H W bytes into the frame and pair
// p lies 2 p bytes behind that; lean_taps_at on the CH x CW plane (CH, CW >= 2) gives pairs p, p + 1, p + CW, p + CW + 1 with
// p + CW + 1 <= CH CW - 1 (its floors are capped at N - 2, and a point outside gives p = 0), so a 2-byte load ends at the
// frame's last byte at the latest.  Offsets inside a frame are 32-bit (H W < 2^30), across frames 64-bit.
// The stores: a luma lane one byte; a chroma lane its U, V pair as one 2-byte store with VEC (out 2-byte aligned: H W 3 / 2 and
// H W are even, so every pair then is), else as two bytes.
// ---------------------------------------------------------------------------
struct InterpNv12Args {
    InterpArgs g;              // frames [B+1][H W 3 / 2], out [B][n][H W 3 / 2]
    double sx, sy;             // the siting: chroma sample (i, j) sits at luma (2 i + sx, 2 j + sy)
    unsigned luma_groups;      // ceil(H / 4): the blockIdx.x below which a block does luma
    unsigned chroma_cols;      // ceil((W / 2) / 64): column blocks of the chroma plane
};

__device__ __forceinline__ double interp_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the taps of a side's chroma sample on the CH x CW plane; `in`: the solved point is inside the luma frame
__device__ __forceinline__ LeanTaps interp_chroma_taps(const LeanGeom &lc, double px, double py, double sx, double sy, bool in)
{
    const double dx = px - sx, dy = py - sy;
    LeanTaps t = lean_taps_at(lc, interp_clamp(0.5 * dy, 0.0, lc.Hm1), interp_clamp(0.5 * dx, 0.0, lc.Wm1));
    t.inside = t.inside && in;
    t.off0 = t.inside ? t.off0 : 0u;
    return t;
}

template <bool VEC>
__device__ __forceinline__ void interp_nv12_chroma(const InterpNv12Args &n, unsigned z)
{
    const InterpArgs &a = n.g;
    const int CH = a.H / 2, CW = a.W / 2;
    const unsigned cb = (blockIdx.x - n.luma_groups) * gridDim.y + blockIdx.y;
    const int i = (int)(cb % n.chroma_cols) * 64 + (int)(threadIdx.x & 63);
    const int jr = (int)(cb / n.chroma_cols) * 4 + (int)(threadIdx.x >> 6);
    if (i >= CW || jr >= CH) return;
    const unsigned b = z / (unsigned)a.n, j = z - b * (unsigned)a.n;
    const size_t plane = (size_t)a.H * (size_t)a.W, fbytes = plane + plane / 2;
    const size_t fo = (size_t)b * plane;
    const unsigned char *ua = static_cast<const unsigned char *>(a.frames) + (size_t)b * fbytes + plane, *ub_ = ua + fbytes;
    const LeanGeom lg = lean_geom(a.H, a.W), lc = lean_geom(CH, CW);
    const double tau = a.tau[j];
    const double X = (double)(2 * i) + n.sx, Y = (double)(2 * jr) + n.sy;
    const unsigned crow = lc.rowstep >> 2;   // pairs from tap row 0 to tap row 1

    auto tap = [](const unsigned char *uv, unsigned p) { return (unsigned)reinterpret_cast<const TapPair *>(uv + 2u * p)->v; };
    LeanTaps ca, cbt;
    unsigned qa[4], qb[4];   // U in bits 0-7, V in bits 8-15
    const InterpSolve s = interp_solve<false>(lg, a.uf + fo, a.vf + fo, a.ub + fo, a.vb + fo, a.refine, a.alpha, a.beta, tau, X, Y,
                                              [&](const InterpSolve &p) {
                                                  ca = interp_chroma_taps(lc, p.pxa, p.pya, n.sx, n.sy, p.ta.inside);
                                                  cbt = interp_chroma_taps(lc, p.pxb, p.pyb, n.sx, n.sy, p.tb.inside);
                                                  const unsigned a0 = ca.off0 >> 2, b0 = cbt.off0 >> 2;
                                                  qa[0] = tap(ua, a0); qa[1] = tap(ua, a0 + 1u);
                                                  qa[2] = tap(ua, a0 + crow); qa[3] = tap(ua, a0 + crow + 1u);
                                                  qb[0] = tap(ub_, b0); qb[1] = tap(ub_, b0 + 1u);
                                                  qb[2] = tap(ub_, b0 + crow); qb[3] = tap(ub_, b0 + crow + 1u);
                                              });
    const unsigned cell = (unsigned)jr * (unsigned)CW + (unsigned)i;
    const unsigned pa = tap(ua, cell), pb = tap(ub_, cell);
    const float t = (float)tau;
    auto ch = [](unsigned p, int c) { return (float)((p >> (8 * c)) & 0xffu); };
    unsigned px = 0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float va = lean_finish(ca, PairF{ch(qa[0], c), ch(qa[1], c)}, PairF{ch(qa[2], c), ch(qa[3], c)}) + 0.0f;
        const float vb = lean_finish(cbt, PairF{ch(qb[0], c), ch(qb[1], c)}, PairF{ch(qb[2], c), ch(qb[3], c)}) + 0.0f;
        px |= (unsigned)(unsigned char)rintf(interp_blend(s.oka, s.okb, va, vb, ch(pa, c), ch(pb, c), t)) << (8 * c);
    }
    unsigned char *dst = static_cast<unsigned char *>(a.out) + (size_t)z * fbytes + plane + 2u * cell;
    if constexpr (VEC) {
        *reinterpret_cast<unsigned short *>(dst) = (unsigned short)px;
    } else {
        dst[0] = (unsigned char)px;
        dst[1] = (unsigned char)(px >> 8);
    }
}

// ---- grid (ceil(H / 4) + ceil(ceil(H / 8) chroma_cols / gy), gy = ceil(W / 64), slices of this launch), block 256 ----
template <bool STATUS, bool VEC>
__global__ __launch_bounds__(256) void k_interp_nv12(const InterpNv12Args n)
{
    const unsigned z = n.g.z0 + blockIdx.z;
    if (blockIdx.x < n.luma_groups) {
        const int x = blockIdx.y * 64 + (threadIdx.x & 63);
        const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (x >= n.g.W || y >= n.g.H) return;
        const size_t plane = (size_t)n.g.H * (size_t)n.g.W, fbytes = plane + plane / 2;
        interp_plane<unsigned char, STATUS, false>(n.g, x, y, z, fbytes, fbytes);
    } else {
        interp_nv12_chroma<VEC>(n, z);
    }
}
}  // namespace oflk
