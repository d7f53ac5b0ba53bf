// oflk_sparse.hpp -- gfx950 device code of the sparse pyramidal Lucas-Kanade tracker (oflk_sparse_lk,
// oflk_plan_sparse_tracks): points in, points + status + residual out, no dense flow field anywhere.
//
// The statement (include/oflk.h, tests/sparse_model.py) is built from the reference's own operations: per pyramid level
// the (w+2)^2 template patch P around the point in frame A and, per iteration, the patch Q around the displaced point in
// frame B are bilinear samples (map_coordinates, order 1, cval 0: bilinear_taps / bilinear_finish); the displacement
// update is the centre pixel of lucas_kanade_single_scale(P, Q, w): (P + Q) / 2, Sobel / 8 in convolve2d's order (as
// k_lk_generic), It = P - Q, five np.sum of w*w float32 products, lk_solve.
//
// Shape: one wave per point, one-wave blocks.  A point's chain (L levels x up to K iterations, twice per pair for the
// forward-backward test) is serial; inside an iteration the wave spreads
//   the (w+2)^2 <= 169 samples over its lanes (at most 3 per lane: fp64 taps, four loads, fp64 accumulate),
//   the w*w <= 121 gradients over its lanes (at most 2 per lane, from the averaged patch in LDS),
//   the five sums over 40 lanes: np.sum of 9 <= n <= 121 contiguous values keeps eight interleaved accumulators, adds them
//   in the fixed tree ((0+1)+(2+3))+((4+5)+(6+7)) and then the tail serially (np_pairwise_leaf); accumulator j of sum s
//   is lane 8 s + j, the tree is three xor-shuffles (float addition commutes, so both partners form the same value), and
//   the tail of an odd square is its one last element,
// and every lane solves the same 2x2 system from the five broadcast sums (cheaper than one lane and a broadcast of the
// result, and it keeps the loop conditions wave-uniform).  LDS per block: 3 (w+2)^2 + 3 w^2 floats (3.4 KiB at 11x11).
// All loops are bounded by B * L * K; no spin, no communication between blocks, no atomics.
#pragma once
#include "oflk_kernels.hpp"

#pragma clang fp contract(off)

namespace oflk {

struct SparseArgs {
    const void *frames;                   // [B+1][H][W], the kernel's PIX: the finest level
    const float *pyr[OFLK_MAX_LEVELS];    // l < L-1: [B+1][h_l][w_l] (the plan's pyramid)
    int dims[2 * OFLK_MAX_LEVELS];        // (h_l, w_l), l = 0 coarsest
    float sx[OFLK_MAX_LEVELS], sy[OFLK_MAX_LEVELS];   // l > 0: f32(w_l / w_{l-1}), f32(h_l / h_{l-1}) (upsample_flow's ratios)
    int L, K, B, H, W, N, t0;
    // tracks (k_sparse_track): as TrackArgs
    const int *qt;
    const float *qxy;
    float *tracks;
    unsigned char *visible;
    float alpha, beta, max_residual;
    // one pair (k_sparse_lk): frames 0 -> 1
    const float *pts;                     // [N][2]
    float *next_pts;                      // [N][2]
    unsigned char *status;                // [N]
    float *residual;                      // [N]
};

template <int HW>
struct SparseLds {
    static constexpr int S = 2 * HW + 3, NP = S * S;    // patch side and size
    static constexpr int WD = 2 * HW + 1, NW = WD * WD;  // window side and size
    float P[NP];                // template patch of the level
    float avg[NP], dif[NP];     // (P + Q) / 2 and P - Q of the iteration
    float gx[NW], gy[NW], gt[NW];   // the window's Ix, Iy, It (gx: |Pc - Qc| for the residual)
};

template <class T>
__device__ __forceinline__ float sparse_sample(const void *img, int h, int w, double y, double x)
{
    const BilinearTaps t = bilinear_taps(h, w, y, x);   // offsets are clamped into the plane for every coordinate
    // cval at a point outside, a NaN coordinate included (a displacement is NaN where a window sum overflowed to
    // inf - inf, on finite frames too)
    if (!t.inside) return 0.0f;
    return bilinear_finish(t, ld_pix<T>(img, (unsigned)t.i00), ld_pix<T>(img, (unsigned)t.i01), ld_pix<T>(img, (unsigned)t.i10),
                           ld_pix<T>(img, (unsigned)t.i11));
}

// np.sum of NW contiguous float32 values (9 <= NW <= 128), `nsums` sums at once: lane 8 s + j is accumulator j of sum s,
// elem(s, i) its i-th value.  Every lane of group s returns sum s.  Called by the whole wave.
template <int NW, class ELEM>
__device__ __forceinline__ float wave_np_sum(int lane, int nsums, ELEM elem)
{
    static_assert(NW >= 8 && NW <= 128, "one block of np.sum's pairwise order");
    const int s = lane >> 3, j = lane & 7;
    const bool on = s < nsums;
    float acc = 0.0f;
    if (on) {
        acc = elem(s, j);
        for (int i = 8; i < NW - NW % 8; i += 8) acc = acc + elem(s, i + j);
    }
    acc = acc + __shfl_xor(acc, 1);
    acc = acc + __shfl_xor(acc, 2);
    acc = acc + __shfl_xor(acc, 4);
    if (on)
        for (int i = NW - NW % 8; i < NW; i++) acc = acc + elem(s, i);
    return acc;
}

__device__ __forceinline__ bool wave_uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

// the iterations of one level: A, B the level's two images (h x w elements of T); g is updated, `solved` is the last
// evaluated iteration's abs(det) > 1e-4
template <int HW, class T>
__device__ __forceinline__ void sparse_level(SparseLds<HW> &m, int lane, const void *A, const void *B, int h, int w, int K,
                                             double xl, double yl, float &gx, float &gy, bool &solved)
{
    using M = SparseLds<HW>;
    for (int k = lane; k < M::NP; k += 64) {
        const int j = k / M::S, i = k - j * M::S;
        m.P[k] = sparse_sample<T>(A, h, w, yl + (double)(j - (HW + 1)), xl + (double)(i - (HW + 1)));
    }
    __syncthreads();
    for (int it = 0; it < K; it++) {
        const double cx = xl + (double)gx, cy = yl + (double)gy;
        for (int k = lane; k < M::NP; k += 64) {
            const int j = k / M::S, i = k - j * M::S;
            const float q = sparse_sample<T>(B, h, w, cy + (double)(j - (HW + 1)), cx + (double)(i - (HW + 1)));
            const float p = m.P[k];
            m.avg[k] = (p + q) * 0.5f;   // (prev + curr) / 2
            m.dif[k] = p - q;            // It
        }
        __syncthreads();
        for (int e = lane; e < M::NW; e += 64) {
            const int r = e / M::WD, c = e - r * M::WD;
            const float *a = m.avg + (r + 1) * M::S + (c + 1);   // the window element's patch position
            const float a_mm = a[-M::S - 1], a_m0 = a[-M::S], a_mp = a[-M::S + 1];
            const float a_0m = a[-1], a_0p = a[1];
            const float a_pm = a[M::S - 1], a_p0 = a[M::S], a_pp = a[M::S + 1];
            // Sobel / 8 in convolve2d's order, as k_lk_generic.  The products by powers of two are exact unless the product is
            // subnormal; there every product of two gradients underflows to 0, det = 0 and nothing is solved either way.
            float ix, iy;
            ix = a_pp * -0.125f;
            ix = fmaf(a_pm, 0.125f, ix);
            ix = fmaf(a_0p, -0.25f, ix);
            ix = fmaf(a_0m, 0.25f, ix);
            ix = fmaf(a_mp, -0.125f, ix);
            ix = fmaf(a_mm, 0.125f, ix);
            iy = a_pp * -0.125f;
            iy = fmaf(a_p0, -0.25f, iy);
            iy = fmaf(a_pm, -0.125f, iy);
            iy = fmaf(a_mp, 0.125f, iy);
            iy = fmaf(a_m0, 0.25f, iy);
            iy = fmaf(a_mm, 0.125f, iy);
            m.gx[e] = ix;
            m.gy[e] = iy;
            m.gt[e] = m.dif[(r + 1) * M::S + (c + 1)];
        }
        __syncthreads();
        const float acc = wave_np_sum<M::NW>(lane, 5, [&](int s, int i) -> float {
            const float ix = m.gx[i], iy = m.gy[i], gt = m.gt[i];
            const float f0 = (s == 1 || s == 4) ? iy : ix;
            const float f1 = s == 0 ? ix : (s == 1 || s == 2) ? iy : gt;
            return f0 * f1;   // xx, yy, xy, xt, yt
        });
        // np.sum starts from the identity 0
        const float Sxx = 0.0f + __shfl(acc, 0), Syy = 0.0f + __shfl(acc, 8), Sxy = 0.0f + __shfl(acc, 16);
        const float Sxt = 0.0f + __shfl(acc, 24), Syt = 0.0f + __shfl(acc, 32);
        const float m0 = Sxx * Syy, m1 = Sxy * Sxy;
        solved = wave_uniform(fabsf(m0 - m1) > 1e-4f);   // lk_solve's own test
        float du, dv;
        lk_solve(Sxx, Syy, Sxy, Sxt, Syt, du, dv);
        gx = gx + du;
        gy = gy + dv;
        if (wave_uniform(fabsf(du) < 0.01f && fabsf(dv) < 0.01f)) break;   // the reference's exit threshold, on the point
    }
}

struct SparseStep {
    double qx, qy;
    float gx, gy, residual;
    bool ok;
};

// step(A, B, x, y) of the statement: frames ia -> ib of the launch's buffer; (x, y) inside the frame.  Called by the
// whole wave with wave-uniform arguments; every lane returns the same values.
template <int HW, class PIX>
__device__ __forceinline__ SparseStep sparse_step(const SparseArgs &a, SparseLds<HW> &m, int lane, int ia, int ib, float x, float y)
{
    using M = SparseLds<HW>;
    const double x64 = (double)x, y64 = (double)y;
    float gx = 0.0f, gy = 0.0f;
    bool solved = false;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const char *fine = static_cast<const char *>(a.frames);
    for (int l = 0; l < a.L; l++) {
        const int h = a.dims[2 * l], w = a.dims[2 * l + 1];
        if (l > 0) {
            gx = gx * a.sx[l];
            gy = gy * a.sy[l];
        }
        if (l == a.L - 1) {   // the frame itself: the caller's pixels, no arithmetic on the position
            sparse_level<HW, PIX>(m, lane, fine + (size_t)ia * plane * sizeof(PIX), fine + (size_t)ib * plane * sizeof(PIX), h, w, a.K,
                                  x64, y64, gx, gy, solved);
        } else {              // linspace geometry of the resampled level: multiply, then divide (float64)
            const double xl = x64 * (double)(w - 1) / (double)(a.W - 1), yl = y64 * (double)(h - 1) / (double)(a.H - 1);
            const size_t n = (size_t)h * (size_t)w;
            sparse_level<HW, float>(m, lane, a.pyr[l] + (size_t)ia * n, a.pyr[l] + (size_t)ib * n, h, w, a.K, xl, yl, gx, gy, solved);
        }
        __syncthreads();   // the next level's template overwrites P
    }
    SparseStep r;
    r.gx = gx;
    r.gy = gy;
    r.qx = x64 + (double)gx;
    r.qy = y64 + (double)gy;
    r.ok = solved && isfinite(r.qx) && isfinite(r.qy) && r.qx >= 0.0 && r.qx <= (double)(a.W - 1) && r.qy >= 0.0 &&
           r.qy <= (double)(a.H - 1);
    // residual: mean |Pc - Qc| over the window, Pc the centre of the finest level's template, Qc sampled around q
    const void *Bf = fine + (size_t)ib * plane * sizeof(PIX);
    for (int e = lane; e < M::NW; e += 64) {
        const int rr = e / M::WD, c = e - rr * M::WD;
        const float q = sparse_sample<PIX>(Bf, a.H, a.W, r.qy + (double)(rr - HW), r.qx + (double)(c - HW));
        m.gx[e] = fabsf(m.P[(rr + 1) * M::S + (c + 1)] - q);
    }
    __syncthreads();
    const float acc = wave_np_sum<M::NW>(lane, 1, [&](int, int i) -> float { return m.gx[i]; });
    r.residual = (0.0f + __shfl(acc, 0)) / (float)M::NW;
    __syncthreads();   // the next step overwrites P and gx
    return r;
}

// a point inside [0, W-1] x [0, H-1] (NaN: false), compared in float32 as k_track
__device__ __forceinline__ bool sparse_inside(const SparseArgs &a, float x, float y)
{
    return x >= 0.0f && x <= (float)(a.W - 1) && y >= 0.0f && y <= (float)(a.H - 1);
}

// oflk_sparse_lk: grid (N), one wave per point
template <int HW, class PIX>
__global__ __launch_bounds__(64) void k_sparse_lk(SparseArgs a)
{
    __shared__ SparseLds<HW> m;
    const size_t n = blockIdx.x;
    const int lane = threadIdx.x;
    const float x = a.pts[2 * n], y = a.pts[2 * n + 1];
    const float nan = __builtin_nanf("");
    float ox = nan, oy = nan, res = nan;
    unsigned char ok = 0;
    if (wave_uniform(sparse_inside(a, x, y))) {
        const SparseStep s = sparse_step<HW, PIX>(a, m, lane, 0, 1, x, y);
        ox = __double2float_rn(s.qx);
        oy = __double2float_rn(s.qy);
        res = s.residual;
        ok = s.ok ? 1 : 0;
    }
    if (lane == 0) {
        a.next_pts[2 * n] = ox;
        a.next_pts[2 * n + 1] = oy;
        a.status[n] = ok;
        a.residual[n] = res;
    }
}

// oflk_plan_sparse_tracks: grid (N), one wave per query, looping over the launch's pairs as k_track does.  A step of an
// alive point is the forward step, then (if it is ok) the backward step from the rounded target, the forward-backward
// test on the two displacements (fb_finish's expressions) and the residual test.
// RES (oflk_plan_sparse_klt_replenish): step_residual [B+1][N], row r of query n = the forward step's residual of pair r - 1
// where the point was alive on row r - 1 and that step was ok, whether or not the track survives it; NaN otherwise.  Row 0
// is written (NaN) by the launch with t0 == 0 only: in a later launch it is the earlier launch's last row.
template <int HW, class PIX, bool RES>
__device__ __forceinline__ void sparse_track(const SparseArgs &a, SparseLds<HW> &m, float *step_residual)
{
    const size_t n = blockIdx.x, N = (size_t)a.N;
    const int lane = threadIdx.x;
    const int qt = a.qt ? a.qt[n] : 0;
    const float qx = a.qxy[2 * n], qy = a.qxy[2 * n + 1];
    const bool q_in = sparse_inside(a, qx, qy);
    const bool earlier = qt < a.t0;
    const long long r_q = earlier ? -1 : (long long)qt - a.t0;   // the query's row in this launch (> B: a later launch)
    bool alive = false;
    float x = 0.0f, y = 0.0f;
    if (earlier) {   // a track of an earlier launch: row 0 is its state
        alive = a.visible[n] != 0;
        x = a.tracks[2 * n];
        y = a.tracks[2 * n + 1];
    }
    const float nan = __builtin_nanf("");
    for (int r = 0; r <= a.B; r++) {
        if (r > 0 && wave_uniform(alive)) {   // pair r - 1
            SparseStep f{};
            float nx = 0.0f, ny = 0.0f;
            bool keep = false;
            for (int d = 0; d < 2; d++) {   // forward, then backward from the forward step's target (one copy of the step)
                const SparseStep s = sparse_step<HW, PIX>(a, m, lane, d ? r : r - 1, d ? r - 1 : r, d ? nx : x, d ? ny : y);
                if (d == 0) {
                    f = s;
                    nx = __double2float_rn(s.qx);
                    ny = __double2float_rn(s.qy);
                    if (!wave_uniform(s.ok)) break;
                } else {
                    const float us = f.gx, vs = f.gy, bu = s.gx, bv = s.gy;
                    const float eu = us + bu, ev = vs + bv;
                    const float e2 = eu * eu + ev * ev;
                    const float m2 = (us * us + vs * vs) + (bu * bu + bv * bv);
                    keep = s.ok && e2 <= a.alpha * m2 + a.beta && f.residual <= a.max_residual;
                }
            }
            if constexpr (RES)
                if (lane == 0) step_residual[(size_t)r * N + n] = f.ok ? f.residual : nan;
            alive = keep;
            x = nx;
            y = ny;
        } else if constexpr (RES) {
            if (lane == 0 && (r > 0 || a.t0 == 0)) step_residual[(size_t)r * N + n] = nan;
        }
        if (r == r_q) {
            alive = q_in;
            x = qx + 0.0f;   // -0 -> +0
            y = qy + 0.0f;
        }
        if (r == 0 && earlier) continue;   // row 0 is the caller's
        if (lane == 0) {
            const size_t i = (size_t)r * N + n;
            a.tracks[2 * i] = alive ? x : nan;
            a.tracks[2 * i + 1] = alive ? y : nan;
            a.visible[i] = alive ? 1 : 0;
        }
    }
}

template <int HW, class PIX>
__global__ __launch_bounds__(64) void k_sparse_track(SparseArgs a)
{
    __shared__ SparseLds<HW> m;
    sparse_track<HW, PIX, false>(a, m, nullptr);
}

// the same with the residual rows: a kernel of its own, so that the launches without them keep their arguments and code
template <int HW, class PIX>
__global__ __launch_bounds__(64) void k_sparse_track_residual(SparseArgs a, float *step_residual)
{
    __shared__ SparseLds<HW> m;
    sparse_track<HW, PIX, true>(a, m, step_residual);
}

// oflk_plan_sparse_klt_replenish: born [nb] and detected [nd] zeroed ahead of the pass's detections.  A launch, so that a
// captured pass is a chain of kernels only.
__global__ __launch_bounds__(256) void k_sparse_rows_clear(unsigned char *born, size_t nb, int *detected, size_t nd)
{
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = first; i < nb; i += stride) born[i] = 0;
    for (size_t i = first; i < nd; i += stride) detected[i] = 0;
}

}  // namespace oflk
