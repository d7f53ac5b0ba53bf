// oflk_stabilize.hpp -- gfx950 device code of video stabilisation (oflk_stabilize_trajectory, oflk_warp_affine, the
// sequence call and the online stabiliser made of them): the smoothed trajectory of the global motion's step models, and
// the resampling of whole frames under one 2 x 3 map each.
//
// The statement is tests/stabilize_model.py (include/oflk.h repeats it).  Everything here is float64 in that file's
// operation order, every operation rounded on its own; nothing is contracted and there is no transcendental: the window's
// weights come from the host.
//
//   k_stab_trajectory   one thread per frame: the serial chain of at most 2 x 64 compositions of its window.  A thread
//                       inverts the steps it needs itself, so there is no workspace, no atomics and nothing passes
//                       between threads; the weights travel by value in the launch arguments, so the launch needs no
//                       upload and can be captured
//   k_stab_online       the same trajectory for n consecutive frames whose steps lie in a ring (the online stabiliser's,
//                       oflk_stabilize_trajectory_ring): one block per frame, the inversions of its window side by side,
//                       the two chains on two lanes, the six weighted sums on six
//   k_warp_affine<PIX, VEC>  one launch for F frames.  A lane owns kWarpPx consecutive output pixels of a row.  VEC (the row
//                       length a multiple of kWarpPx and the bases aligned to a lane's store) stores them as one float4
//                       (float) or one dword (bytes, and the inside mask); every other shape and alignment runs the
//                       other instantiation, which stores element by element.  The four taps of a pixel are
//                       bilinear_taps / bilinear_finish, gathered through the cache as k_warp's: an affine image of a
//                       row segment is a row segment
//   k_warp_perspective<PIX, VEC>  the same body under a 3 x 3 map (oflk_warp_perspective, tests/homography_model.py): the
//                       source position divided by w, two float64 divisions per pixel, outside where w <= 0
#pragma once
#include "oflk_kernels.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kStabBlock = 64;   // k_stab_trajectory's block
constexpr int kStabOnlineBlock = 2 * OFLK_STABILIZE_MAX_RADIUS;   // k_stab_online's: one lane per step of the widest window
constexpr int kWarpPx = 4;       // consecutive output pixels of a lane of k_warp_affine

struct StabWeights {
    double w[OFLK_STABILIZE_MAX_RADIUS + 1];
};

__device__ __forceinline__ void stab_identity(double (&a)[6])
{
    a[0] = 1.0; a[1] = 0.0; a[2] = 0.0;
    a[3] = 0.0; a[4] = 1.0; a[5] = 0.0;
}

// b = the inverse of [a00 a01 tx; a10 a11 ty]; false: a zero determinant or a coefficient that is not finite
__device__ __forceinline__ bool stab_invert(const double (&a)[6], double (&b)[6])
{
    const double det = a[0] * a[4] - a[1] * a[3];
    b[0] = a[4] / det;
    b[1] = -a[1] / det;
    b[3] = -a[3] / det;
    b[4] = a[0] / det;
    b[2] = -(b[0] * a[2] + b[1] * a[5]);
    b[5] = -(b[3] * a[2] + b[4] * a[5]);
    bool ok = !(det == 0.0);
    for (int k = 0; k < 6; k++) ok = ok && __builtin_isfinite(b[k]);
    return ok;
}

// step s and its inverse, both the identity when the step is held; returns held
__device__ __forceinline__ bool stab_step(const float *__restrict__ model, const int *__restrict__ counts, size_t s, double (&a)[6],
                                          double (&b)[6])
{
    bool ok = !counts || counts[3 * s + 2] != 0;
    for (int k = 0; k < 6; k++) {
        a[k] = (double)model[6 * s + k];
        ok = ok && __builtin_isfinite(a[k]);
    }
    ok = stab_invert(a, b) && ok;
    if (!ok) {
        stab_identity(a);
        stab_identity(b);
    }
    return !ok;
}

// f = a o f: apply f, then a
__device__ __forceinline__ void stab_compose(const double (&a)[6], double (&f)[6])
{
    const double c0 = a[0] * f[0] + a[1] * f[3];
    const double c1 = a[0] * f[1] + a[1] * f[4];
    const double c2 = (a[0] * f[2] + a[1] * f[5]) + a[2];
    const double c3 = a[3] * f[0] + a[4] * f[3];
    const double c4 = a[3] * f[1] + a[4] * f[4];
    const double c5 = (a[3] * f[2] + a[4] * f[5]) + a[5];
    f[0] = c0; f[1] = c1; f[2] = c2;
    f[3] = c3; f[4] = c4; f[5] = c5;
}

// ---- the trajectory: grid (ceil(T / kStabBlock)), block kStabBlock ----
__global__ __launch_bounds__(kStabBlock) void k_stab_trajectory(const float *__restrict__ model, const int *__restrict__ counts,
                                                                int T, int radius, StabWeights wt, float *__restrict__ correction,
                                                                double *__restrict__ map, unsigned char *__restrict__ held)
{
    const unsigned t = blockIdx.x * (unsigned)kStabBlock + threadIdx.x;
    if (t >= (unsigned)T) return;
    double a[6], b[6];
    if (t + 1 < (unsigned)T) {
        const bool h = stab_step(model, counts, t, a, b);
        if (held) held[t] = h ? 1 : 0;
    }
    const int rt = min(radius, (int)min(t, (unsigned)T - 1u - t));
    const double w0 = wt.w[0];
    double acc[6] = {w0 * 1.0, w0 * 0.0, w0 * 0.0, w0 * 0.0, w0 * 1.0, w0 * 0.0};
    double ws = w0;
    double f[6], g[6];
    stab_identity(f);
    stab_identity(g);
    for (int i = 1; i <= rt; i++) {
        const double w = wt.w[i];
        stab_step(model, counts, (size_t)t + (size_t)i - 1, a, b);   // frame t to frame t + i
        stab_compose(a, f);
        for (int k = 0; k < 6; k++) acc[k] = acc[k] + w * f[k];
        ws = ws + w;
        stab_step(model, counts, (size_t)t - (size_t)i, a, b);       // frame t to frame t - i
        stab_compose(b, g);
        for (int k = 0; k < 6; k++) acc[k] = acc[k] + w * g[k];
        ws = ws + w;
    }
    float c[6];
    double cd[6], m[6];
    bool ok = true;
    for (int k = 0; k < 6; k++) {
        c[k] = __double2float_rn(acc[k] / ws);
        ok = ok && __builtin_isfinite(c[k]);
        cd[k] = (double)c[k];
    }
    ok = stab_invert(cd, m) && ok;
    if (!ok) {
        stab_identity(cd);
        stab_identity(m);
    }
    for (int k = 0; k < 6; k++) {
        correction[6 * (size_t)t + k] = (float)cd[k];
        map[6 * (size_t)t + k] = m[k];
    }
}

// ---- the trajectory of n consecutive frames from a ring of steps: grid (n), block kStabOnlineBlock ----
// Block b owns frame f = f0 + b.  T < 0: the stream is open and the window is min(radius, f); else min(radius, f, T-1-f).
// Step s lives at ring slot s % cap.  The values are k_stab_trajectory's, each formed by the same operations in the same
// order; what does not depend on the chain's order runs side by side:
//   lanes j < 2 r_f   load and invert step f - r_f + j: A and B into LDS
//   lanes 0 and 1     the forward chain F_i = A_{f+i-1} o F_{i-1} and the backward chain G_i = B_{f-i} o G_{i-1}: one
//                     instruction stream on two LDS addresses, every F_i and G_i kept
//   lanes k < 6       coefficient k: acc += w_i F_i[k]; acc += w_i G_i[k] in i's order, ws likewise, the quotient, float32
//   lane 0            the inverse of the correction, or the identity for both
__global__ __launch_bounds__(kStabOnlineBlock) void k_stab_online(const float *__restrict__ model, const int *__restrict__ counts,
                                                                  int cap, int f0, int T, int radius, StabWeights wt,
                                                                  float *__restrict__ correction, double *__restrict__ map)
{
    __shared__ double step[2][kStabOnlineBlock][6];                   // [0]: A, [1]: B, of step f - r_f + j
    __shared__ double chain[2][OFLK_STABILIZE_MAX_RADIUS + 1][6];     // [0][i]: F_i, [1][i]: G_i
    __shared__ float corr[6];
    const int j = (int)threadIdx.x;
    const unsigned f = (unsigned)f0 + blockIdx.x;
    int rf = (int)min((unsigned)radius, f);
    if (T >= 0) rf = (int)min((unsigned)rf, (unsigned)T - 1u - f);
    if (j < 2 * rf) {
        const unsigned s = f - (unsigned)rf + (unsigned)j;
        double a[6], b[6];
        stab_step(model, counts, (size_t)(s % (unsigned)cap), a, b);
        for (int k = 0; k < 6; k++) {
            step[0][j][k] = a[k];
            step[1][j][k] = b[k];
        }
    }
    __syncthreads();
    if (j < 2) {   // lane 0 forward over A at rf + i - 1, lane 1 backward over B at rf - i
        double c[6], a[6];
        stab_identity(c);
        for (int i = 1; i <= rf; i++) {
            const int at = j == 0 ? rf + i - 1 : rf - i;
            for (int k = 0; k < 6; k++) a[k] = step[j][at][k];
            stab_compose(a, c);
            for (int k = 0; k < 6; k++) chain[j][i][k] = c[k];
        }
    }
    __syncthreads();
    if (j < 6) {
        const double w0 = wt.w[0];
        double acc = w0 * ((j == 0 || j == 4) ? 1.0 : 0.0);
        double ws = w0;
        for (int i = 1; i <= rf; i++) {
            const double w = wt.w[i];
            acc = acc + w * chain[0][i][j];
            ws = ws + w;
            acc = acc + w * chain[1][i][j];
            ws = ws + w;
        }
        corr[j] = __double2float_rn(acc / ws);
    }
    __syncthreads();
    if (j == 0) {
        double cd[6], m[6];
        bool ok = true;
        for (int k = 0; k < 6; k++) {
            ok = ok && __builtin_isfinite(corr[k]);
            cd[k] = (double)corr[k];
        }
        ok = stab_invert(cd, m) && ok;
        if (!ok) {
            stab_identity(cd);
            stab_identity(m);
        }
        for (int k = 0; k < 6; k++) {
            correction[6 * (size_t)blockIdx.x + k] = (float)cd[k];
            map[6 * (size_t)blockIdx.x + k] = m[k];
        }
    }
}

// ---- the warp: grid (ceil(H / 4), ceil(W / (64 kWarpPx)), min(F, 65535)), block 256 = 4 rows of 64 lanes ----
template <class PIX>
struct WarpAffineArgs {
    const PIX *in;            // [F][H][W]
    const double *map;        // [F][6]; k_warp_perspective: [F][9]
    PIX *out;                 // [F][H][W]
    unsigned char *inside;    // [F][H][W] or NULL
    int F, H, W;
};

__device__ __forceinline__ float warp_store_value(float v, float) { return v; }
__device__ __forceinline__ unsigned char warp_store_value(float v, unsigned char) { return (unsigned char)rintf(v); }

// ---- the source position of an output pixel: the one statement of it for every frame layout (warp_frames here,
// k_warp_packed in oflk_colour.hpp, nv12_luma and nv12_chroma in oflk_nv12.hpp) ----
// What a map m and a row y fix.  PERSP: the map has a third row and the source position is divided by
// w = (m6 x + m7 y) + m8, two IEEE divisions per pixel (tests/homography_model.py); w <= 0 or a NaN anywhere is outside.
template <bool PERSP>
struct WarpRow {
    double m0, m2, m3, m5, bx, by;
    double m6, m8, bw;   // read under PERSP only
};

template <bool PERSP>
__device__ __forceinline__ WarpRow<PERSP> warp_row(const double *__restrict__ m, double fy)
{
    WarpRow<PERSP> r;
    r.m0 = m[0]; r.m2 = m[2]; r.m3 = m[3]; r.m5 = m[5];
    r.bx = m[1] * fy; r.by = m[4] * fy;
    r.m6 = 0.0; r.m8 = 1.0; r.bw = 0.0;
    if constexpr (PERSP) {
        r.m6 = m[6];
        r.m8 = m[8];
        r.bw = m[7] * fy;
    }
    return r;
}

// A pixel's own: the source position of column fx and whether it lies in the closed interval [0, Wm1] x [0, Hm1]
struct WarpSource {
    double xs, ys;
    bool ok;
};

template <bool PERSP>
__device__ __forceinline__ WarpSource warp_source(const WarpRow<PERSP> &r, double fx, double Wm1, double Hm1)
{
    [[maybe_unused]] const double w = (r.m6 * fx + r.bw) + r.m8;
    const double xa = (r.m0 * fx + r.bx) + r.m2;
    const double ya = (r.m3 * fx + r.by) + r.m5;
    const double xs = PERSP ? xa / w : xa;
    const double ys = PERSP ? ya / w : ya;
    const bool within = xs >= 0.0 && xs <= Wm1 && ys >= 0.0 && ys <= Hm1;
    return {xs, ys, PERSP ? w > 0.0 && within : within};
}

// a lane's kWarpPx bytes (pixels of a uint8 plane, or `inside`) as the one dword it stores, byte 0 at the lowest address
__device__ __forceinline__ unsigned warp_pack(const unsigned char (&b)[4])
{
    return (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
}

// VEC: W % kWarpPx == 0 and out (and inside, when given) aligned to a lane's store, so every lane owns kWarpPx whole pixels
// and stores them at once.  The two forms are two kernels: in one, the compiler folds the wide store into the tail's.
// PERSP: warp_row's.
template <class PIX, bool VEC, bool PERSP>
__device__ __forceinline__ void warp_frames(const WarpAffineArgs<PIX> a)
{
    constexpr int NC = PERSP ? 9 : 6;
    const int x0 = ((int)blockIdx.y * 64 + (int)(threadIdx.x & 63)) * kWarpPx;
    const int y = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (x0 >= a.W || y >= a.H) return;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const size_t row = (size_t)y * (size_t)a.W + (size_t)x0;
    const double fy = (double)y, Wm1 = (double)(a.W - 1), Hm1 = (double)(a.H - 1);
    for (int f = blockIdx.z; f < a.F; f += gridDim.z) {
        const double *__restrict__ m = a.map + NC * (size_t)f;
        const WarpRow<PERSP> r = warp_row<PERSP>(m, fy);
        const PIX *__restrict__ img = a.in + (size_t)f * plane;
        PIX v[kWarpPx];
        unsigned char in[kWarpPx];
#pragma unroll
        for (int k = 0; k < kWarpPx; k++) {   // a pixel past the row's end is computed (its taps are clamped) and not stored
            const double fx = (double)(x0 + k);
            const WarpSource p = warp_source(r, fx, Wm1, Hm1);
            const BilinearTaps t = bilinear_taps(a.H, a.W, p.ys, p.xs);
            const float s = bilinear_finish(t, ld_pix<PIX>(img, (unsigned)t.i00), ld_pix<PIX>(img, (unsigned)t.i01),
                                            ld_pix<PIX>(img, (unsigned)t.i10), ld_pix<PIX>(img, (unsigned)t.i11));
            v[k] = warp_store_value(p.ok ? s : 0.0f, PIX());
            in[k] = p.ok ? 1 : 0;
        }
        PIX *__restrict__ dst = a.out + (size_t)f * plane + row;
        if constexpr (VEC) {
            if constexpr (sizeof(PIX) == 4) {
                *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                *reinterpret_cast<unsigned *>(dst) = warp_pack(v);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kWarpPx; k++)
                if (x0 + k < a.W) dst[k] = v[k];
        }
        if (a.inside) {
            unsigned char *__restrict__ di = a.inside + (size_t)f * plane + row;
            if constexpr (VEC) {
                *reinterpret_cast<unsigned *>(di) = warp_pack(in);
            } else {
#pragma unroll
                for (int k = 0; k < kWarpPx; k++)
                    if (x0 + k < a.W) di[k] = in[k];
            }
        }
    }
}

template <class PIX, bool VEC>
__global__ __launch_bounds__(256) void k_warp_affine(WarpAffineArgs<PIX> a)
{
    warp_frames<PIX, VEC, false>(a);
}

template <class PIX, bool VEC>
__global__ __launch_bounds__(256) void k_warp_perspective(WarpAffineArgs<PIX> a)
{
    warp_frames<PIX, VEC, true>(a);
}

}  // namespace oflk
