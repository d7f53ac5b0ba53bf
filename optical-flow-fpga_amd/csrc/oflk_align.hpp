// oflk_align.hpp -- gfx950 device code of direct image alignment (oflk_align_refine, oflk_align_sequence, their _photo and
// _robust forms, their host forms and oflk_align_weights): inverse-compositional Lucas-Kanade registration of frame B to the
// template A over the whole frame, coarse to fine, from a given affine (NP = 6) or homography (NP = 8) step model.
//
// There are four forms of one arithmetic, chosen by two template flags.  With sd the NP steepest-descent values of a pixel, a
// the template's value and v the sample of B under the model:
//
//   form                   statement                      residual r             columns c (NQ of them)       sums
//   plain                  tests/align_model.py           f64(v - a)             sd                     (NP)  29 / 46
//   PHOTO                  tests/align_photo_model.py     f64(v) - (g a + b)     [g sd, a, 1.0]     (NP + 2)  46 / 67
//   ROBUST                 tests/align_robust_model.py    the plain one          sd                     (NP)  31 / 48
//   PHOTO and ROBUST       tests/align_robust_model.py    the photometric one    [g sd, a, 1.0]     (NP + 2)  48 / 69
//
// The sums of a form, each in the statement's order over the counted pixels: the upper triangle of l[i] c[j], then l[i] r,
// r r and the count, where the left factor l is c itself or, under ROBUST, w c with the Huber weight
// w = |r| > delta ? delta / |r| : 1.0; ROBUST adds rho and w behind them, and rho, not r r, then decides the rejection.  PHOTO
// carries a step's gain and bias (g, b) beside its AlignState, in an array of their own (photo [S][2], begun at (1, 0)).
// include/oflk.h repeats the statements.
//
// Everything here is the statements' operation in their order, every operation rounded on its own; nothing is contracted,
// there is no atomic and no result depends on the launch geometry.  One chain of launches on one stream, nothing passes
// through the host between iterations:
//
//   k_align_begin          one thread per step: the input model widened into the step's state, or the step marked dead
//   k_align_photo_begin    PHOTO: one thread per step, (g, b) = (1, 0)
//   k_align_reduce<PIX, NP, PHOTO, ROBUST>  grid (tiles, steps), one wave per tile of 64 columns x 32 rows.  A lane owns a
//                          column and walks it top to bottom with its float64 sums in registers.  The template is read
//                          coalesced, three values per row (the pixel and its two neighbours: a 3 x 3 window slides down the
//                          column in registers and gives the Sobel gradients, so no gradient plane is written or read); B's
//                          four taps are gathered through the cache as k_warp_perspective's.  The wave combines the 64
//                          columns by the stated tree with shuffles and lane 0 writes the tile's sums.  The photometric
//                          homography is a block of two waves on the same tile: each walks all 64 columns and keeps one half
//                          of the 67 or 69 sums, so that a wave stays within 256 registers.  Which wave holds a sum does not
//                          change the sum's order; the sampling and the sd row are computed twice.  No LDS, no barrier, no
//                          scratch: each wave's lane 0 writes its own sums
//   k_align_update<NP, PHOTO, ROBUST>  one block of 64 per step: lane k adds sums k, k + 64 of the tiles in raster order;
//                          then every lane runs the step's serial part in registers (the refusals, the homography refit's
//                          elimination on NQ rows, the update's conjugation, the adjugate, the product, the corner test, the
//                          g, b update, the level's conjugations) and lane 0 writes the state.  mode 0 records the first
//                          full-resolution residual, mode 2 the last one and writes the outputs; both read the sums of the
//                          same reduce kernel
//   k_align_weights<PIX, NP, PHOTO>  the robust forms' map, one thread per pixel of the frame: f32(w) at counted pixels,
//                          0.0f elsewhere
#pragma once
#include "oflk_kernels.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kAlignTileW = 64;   // a tile's columns: one per lane
constexpr int kAlignTileH = 32;   // a tile's rows
constexpr int kAlignLive = 0, kAlignFrozen = 1, kAlignDead = 2;
constexpr int kAlignFirst = 0, kAlignIterate = 1, kAlignLast = 2;   // k_align_update's modes

// a form's columns, its sums per tile and the waves of a block of its reduce kernel
__host__ __device__ constexpr int align_columns(int NP, bool PHOTO) { return NP + (PHOTO ? 2 : 0); }
__host__ __device__ constexpr int align_sums(int NP, bool PHOTO = false, bool ROBUST = false)
{
    return align_columns(NP, PHOTO) * (align_columns(NP, PHOTO) + 1) / 2 + align_columns(NP, PHOTO) + 2 + (ROBUST ? 2 : 0);
}
constexpr int align_waves(int NP, bool PHOTO) { return NP == 8 && PHOTO ? 2 : 1; }
// the place of c[i] c[j], i <= j, among the sums: row after row of the upper triangle of NQ columns
__host__ __device__ constexpr int align_pair(int NQ, int i, int j) { return i * (2 * NQ - i + 1) / 2 + (j - i); }

// a step's state between launches.  m is in frame coordinates between levels and in the level's inside one
struct AlignState {
    double m[9];
    double before;   // the first full-resolution mean squared residual (ROBUST: mean rho)
    int flag, accepted;
};

__device__ __forceinline__ void align_to_level(double (&m)[9], double sx, double sy)
{
    m[1] = (m[1] * sx) / sy; m[2] = m[2] * sx;
    m[3] = (m[3] * sy) / sx; m[5] = m[5] * sy;
    m[6] = m[6] / sx;        m[7] = m[7] / sy;
}

__device__ __forceinline__ void align_from_level(double (&m)[9], double sx, double sy)
{
    m[1] = (m[1] * sy) / sx; m[2] = m[2] / sx;
    m[3] = (m[3] * sx) / sy; m[5] = m[5] / sy;
    m[6] = m[6] * sx;        m[7] = m[7] * sy;
}

// Gaussian elimination without pivoting on the N x (N + 1) array [G | b], then the back substitution into h: the procedure of
// the homography's branch of k_motion_refit (tests/homography_model.py, solve8) on N rows, fully unrolled so that no indexed array is left.  A function of its
// own: sharing one with that kernel changed its register allocation.  false: a pivot is zero or not finite
template <int N>
__device__ __forceinline__ bool align_eliminate(double (&G)[N][N + 1], double (&h)[N])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const double piv = G[k][k];
        ok = ok && !(piv == 0.0) && __builtin_isfinite(piv);
#pragma unroll
        for (int i = k + 1; i < N; i++) {
            const double f = G[i][k] / piv;
#pragma unroll
            for (int j = k + 1; j < N + 1; j++) G[i][j] = G[i][j] - f * G[k][j];
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double t = G[i][N];
#pragma unroll
        for (int j = i + 1; j < N; j++) t = t - G[i][j] * h[j];
        h[i] = t / G[i][i];
    }
    return ok;
}

// ---- begin: grid (ceil(S / 64)), block 64 ----
__global__ __launch_bounds__(64) void k_align_begin(const float *__restrict__ model, const int *__restrict__ status, int S, int nc,
                                                    AlignState *__restrict__ state)
{
    const unsigned s = blockIdx.x * 64u + threadIdx.x;
    if (s >= (unsigned)S) return;
    AlignState *__restrict__ st = state + s;
    bool ok = !status || status[s] != 0;
    for (int k = 0; k < 9; k++) {
        const float c = k < nc ? model[(size_t)nc * s + k] : (k == 8 ? 1.0f : 0.0f);
        ok = ok && __builtin_isfinite(c);
        st->m[k] = (double)c;
    }
    st->before = 0.0;
    st->flag = ok ? kAlignLive : kAlignDead;
    st->accepted = 0;
}

__global__ __launch_bounds__(64) void k_align_photo_begin(int S, double *__restrict__ photo)
{
    const unsigned s = blockIdx.x * 64u + threadIdx.x;
    if (s >= (unsigned)S) return;
    photo[2 * (size_t)s] = 1.0;
    photo[2 * (size_t)s + 1] = 0.0;
}

// ---- the sums: grid (tiles, min(S, 65535)), block 64 * align_waves(NP, PHOTO) ----
struct AlignReduceArgs {
    const void *a, *b;         // the level's template and image of step 0
    size_t stride;             // elements from a step's image to the next step's
    int H, W, tiles_x, S;
    int skip_frozen;           // an iteration's sums: a frozen step has none
    const AlignState *state;   // [S]
    double *partial;           // [S][pstride]: a tile's NS sums at tile * NS
    size_t pstride;
    const double *photo;       // PHOTO: [S][2]
    double delta;              // ROBUST: f64(f32(robust_delta))
};

// one wave's walk over its tile for the sums K0 .. K1-1 of step s
template <class PIX, int NP, bool PHOTO, bool ROBUST, int K0, int K1>
__device__ __forceinline__ void align_tile(const AlignReduceArgs &a, int s, int lane, int tile)
{
    constexpr int NQ = align_columns(NP, PHOTO);
    constexpr int NH = NQ * (NQ + 1) / 2;
    constexpr int NS = align_sums(NP, PHOTO, ROBUST);
    constexpr int NK = K1 - K0;
    static_assert(K0 >= 0 && K0 < K1 && K1 <= NS, "a wave's share of the sums");
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int H = a.H, W = a.W;
    const int x = tx * kAlignTileW + lane;
    const bool col = x < W;
    const int xc = min(x, W - 1), xl = max(xc - 1, 0), xr = min(xc + 1, W - 1);
    const int y0 = ty * kAlignTileH, rows = min(kAlignTileH, H - y0);
    const double Wm1 = (double)(W - 1), Hm1 = (double)(H - 1);
    const double cx = Wm1 / 2.0, cy = Hm1 / 2.0, sc = (double)max(W, H) / 2.0;
    const double fx = (double)x;
    const double xh = (fx - cx) / sc;
    [[maybe_unused]] double delta = 0.0;
    if constexpr (ROBUST) delta = a.delta;
    const AlignState *__restrict__ st = a.state + s;
    const double m0 = st->m[0], m1 = st->m[1], m2 = st->m[2], m3 = st->m[3], m4 = st->m[4], m5 = st->m[5];
    [[maybe_unused]] double m6 = 0.0, m7 = 0.0, m8 = 1.0;
    if constexpr (NP == 8) {
        m6 = st->m[6]; m7 = st->m[7]; m8 = st->m[8];
    }
    [[maybe_unused]] double g = 1.0, b = 0.0;
    if constexpr (PHOTO) {
        g = a.photo[2 * (size_t)s];
        b = a.photo[2 * (size_t)s + 1];
    }
    const PIX *__restrict__ A = static_cast<const PIX *>(a.a) + (size_t)s * a.stride;
    const PIX *__restrict__ B = static_cast<const PIX *>(a.b) + (size_t)s * a.stride;
    double acc[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) acc[k] = 0.0;
    // sum k, when it is this wave's; k is a constant once the loops are unrolled, so no indexed array is left
    auto add = [&](int k, double v) {
        if (k >= K0 && k < K1) acc[k - K0] = acc[k - K0] + v;
    };
    // the 3 x 3 window of the template about (x, y), border clamped; k_gradients' average of a frame with itself
    auto load3 = [&](int yy, float (&v)[3], float &centre) {
        const unsigned r = (unsigned)yy * (unsigned)W;
        const float l = ld_pix<PIX>(A, r + (unsigned)xl), c = ld_pix<PIX>(A, r + (unsigned)xc), q = ld_pix<PIX>(A, r + (unsigned)xr);
        centre = c;
        v[0] = (l + l) * 0.5f; v[1] = (c + c) * 0.5f; v[2] = (q + q) * 0.5f;
    };
    float am[3], a0[3], ap[3], t0 = 0.0f, tn = 0.0f, unused = 0.0f;
    load3(max(y0 - 1, 0), am, unused);
    load3(y0, a0, t0);
    for (int i = 0; i < rows; i++) {
        const int y = y0 + i;
        load3(min(y + 1, H - 1), ap, tn);
        // compute_gradients' Sobel / 8 (k_gradients: the same taps in the same order, each product rounded on its own --
        // exact unless it is subnormal -- and then added; the kernels' zero taps last).  Two roundings a tap only because the
        // translation unit is built with -ffp-contract=off, as at k_gradients.
        float ix = ap[2] * -0.125f;
        ix = ix + ap[0] * 0.125f;
        ix = ix + a0[2] * -0.25f;
        ix = ix + a0[0] * 0.25f;
        ix = ix + am[2] * -0.125f;
        ix = ix + am[0] * 0.125f;
        float iy = ap[2] * -0.125f;
        iy = iy + ap[1] * -0.25f;
        iy = iy + ap[0] * -0.125f;
        iy = iy + am[2] * 0.125f;
        iy = iy + am[1] * 0.25f;
        iy = iy + am[0] * 0.125f;
        ix = fmaf(ap[1], 0.0f, ix);
        ix = fmaf(a0[1], 0.0f, ix);
        ix = fmaf(am[1], 0.0f, ix);
        iy = fmaf(a0[2], 0.0f, iy);
        iy = fmaf(a0[1], 0.0f, iy);
        iy = fmaf(a0[0], 0.0f, iy);
        // the source position: the expressions of warp_row and warp_source (oflk_stabilize.hpp), repeated here with the row
        // products formed per pixel; the kernel is kept off the helper so that its generated code stays what was measured
        const double fy = (double)y;
        [[maybe_unused]] const double w = (m6 * fx + m7 * fy) + m8;
        const double xa = (m0 * fx + m1 * fy) + m2;
        const double ya = (m3 * fx + m4 * fy) + m5;
        const double xs = NP == 8 ? xa / w : xa;
        const double ys = NP == 8 ? ya / w : ya;
        const bool within = xs >= 0.0 && xs <= Wm1 && ys >= 0.0 && ys <= Hm1;
        const bool ok = (NP == 8 ? w > 0.0 && within : within) && col;
        const BilinearTaps t = bilinear_taps(H, W, ys, xs);
        const float smp = bilinear_finish(t, ld_pix<PIX>(B, (unsigned)t.i00), ld_pix<PIX>(B, (unsigned)t.i01),
                                          ld_pix<PIX>(B, (unsigned)t.i10), ld_pix<PIX>(B, (unsigned)t.i11));
        if (ok) {
            [[maybe_unused]] const double av = (double)t0;
            double r;
            if constexpr (PHOTO)
                r = (double)smp - (g * av + b);
            else
                r = (double)(smp - t0);
            const double gx = (double)ix, gy = (double)iy;
            const double yh = (fy - cy) / sc;
            double sd[NP], c[NQ];
            sd[0] = gx * xh; sd[1] = gx * yh; sd[2] = gx;
            sd[3] = gy * xh; sd[4] = gy * yh; sd[5] = gy;
            if constexpr (NP == 8) {
                const double tt = sd[0] + sd[4];
                sd[6] = -(tt * xh);
                sd[7] = -(tt * yh);
            }
#pragma unroll
            for (int p = 0; p < NP; p++) c[p] = PHOTO ? g * sd[p] : sd[p];
            if constexpr (PHOTO) {
                c[NP] = av;
                c[NP + 1] = 1.0;
            }
            // the Huber weight and loss; a NaN r fails the comparison
            [[maybe_unused]] double wt = 1.0, rho = 0.0;
            if constexpr (ROBUST) {
                const double ar = __builtin_fabs(r);
                const bool big = ar > delta;
                wt = big ? delta / ar : 1.0;
                rho = big ? delta * (ar - delta * 0.5) : (r * r) * 0.5;
            }
#pragma unroll
            for (int p = 0; p < NQ; p++) {
                double lc = c[p];
                if constexpr (ROBUST) lc = wt * c[p];
#pragma unroll
                for (int q = p; q < NQ; q++) add(align_pair(NQ, p, q), lc * c[q]);
                add(NH + p, lc * r);
            }
            add(NH + NQ, r * r);
            add(NH + NQ + 1, 1.0);
            if constexpr (ROBUST) {
                add(NH + NQ + 2, rho);
                add(NH + NQ + 3, wt);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            am[k] = a0[k];
            a0[k] = ap[k];
        }
        t0 = tn;
    }
    // the 64 columns by the stated tree: partial[c] += partial[c + stride] for c < stride
#pragma unroll
    for (int stride = kAlignTileW / 2; stride >= 1; stride >>= 1)
#pragma unroll
        for (int k = 0; k < NK; k++) acc[k] = acc[k] + __shfl_down(acc[k], (unsigned)stride, 64);
    if (lane == 0) {
        double *__restrict__ out = a.partial + (size_t)s * a.pstride + (size_t)tile * NS + K0;
#pragma unroll
        for (int k = 0; k < NK; k++) out[k] = acc[k];
    }
}

template <class PIX, int NP, bool PHOTO, bool ROBUST>
__global__ __launch_bounds__(64 * align_waves(NP, PHOTO)) void k_align_reduce(AlignReduceArgs a)
{
    constexpr int NS = align_sums(NP, PHOTO, ROBUST);
    const int lane = (int)(threadIdx.x & 63);
    [[maybe_unused]] const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)blockIdx.x;
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        const int flag = a.state[s].flag;
        if (flag == kAlignDead || (flag == kAlignFrozen && a.skip_frozen)) continue;
        if constexpr (align_waves(NP, PHOTO) == 1) {
            align_tile<PIX, NP, PHOTO, ROBUST, 0, NS>(a, s, lane, tile);
        } else {
            constexpr int cut = (NS + 1) / 2;
            if (wave == 0)
                align_tile<PIX, NP, PHOTO, ROBUST, 0, cut>(a, s, lane, tile);
            else
                align_tile<PIX, NP, PHOTO, ROBUST, cut, NS>(a, s, lane, tile);
        }
    }
}

// ---- the update: grid (min(S, 65535)), block 64 ----
struct AlignUpdateArgs {
    AlignState *state;        // [S]
    const double *partial;    // [S][pstride]
    size_t pstride;
    int tiles, S, mode;
    int H, W;                 // the frame
    int h, w;                 // the level of the sums
    int last;                 // kAlignIterate: the level's last iteration, the model goes back to the frame
    int nh, nw;               // the level of the next sums (0: there is none)
    double min_count;         // f64(f32(min_share)) * f64(w h)
    double *photo;            // PHOTO: [S][2]
    double *first;            // ROBUST: [S][2], r r / count and sum(w) / count of the first pass
    // kAlignLast
    const float *model_in;    // [S][nc]
    float *model_out;         // [S][nc]
    int *status_out;          // [S]
    double *stats;            // [S][4], ROBUST: [S][8]
    float *photo_out;         // PHOTO: [S][2]
};

template <int NP, bool PHOTO, bool ROBUST>
__global__ __launch_bounds__(64) void k_align_update(AlignUpdateArgs a)
{
    constexpr int NQ = align_columns(NP, PHOTO);
    constexpr int NS = align_sums(NP, PHOTO, ROBUST);
    constexpr int NH = NQ * (NQ + 1) / 2;
    constexpr int NC = NP == 8 ? 9 : 6;
    __shared__ double sum[NS];
    const int lane = (int)threadIdx.x;
    for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
        AlignState *__restrict__ st = a.state + s;
        const int flag = st->flag;
        const bool summed = flag == kAlignLive || (flag == kAlignFrozen && a.mode != kAlignIterate);
        __syncthreads();   // sum is rewritten
        if (summed)
            for (int k = lane; k < NS; k += 64) {
                const double *__restrict__ p = a.partial + (size_t)s * a.pstride + k;
                double t = 0.0;
                for (int i = 0; i < a.tiles; i++) t = t + p[(size_t)i * NS];
                sum[k] = t;
            }
        __syncthreads();
        double m[9];
        for (int k = 0; k < 9; k++) m[k] = st->m[k];
        [[maybe_unused]] double g = 1.0, b = 0.0;
        if constexpr (PHOTO) {
            g = a.photo[2 * (size_t)s];
            b = a.photo[2 * (size_t)s + 1];
        }
        int accepted = st->accepted;
        const double e = summed ? sum[NH + NQ] : 0.0, cnt = summed ? sum[NH + NQ + 1] : 0.0;
        [[maybe_unused]] double rho = 0.0, wsum = 0.0;
        if constexpr (ROBUST) {
            rho = summed ? sum[NH + NQ + 2] : 0.0;
            wsum = summed ? sum[NH + NQ + 3] : 0.0;
        }
        const double loss = (ROBUST ? rho : e) / cnt;   // what decides the rejection
        if (a.mode == kAlignLast) {
            if (lane != 0) continue;
            const float *__restrict__ in = a.model_in + (size_t)NC * s;
            float *__restrict__ out = a.model_out + (size_t)NC * s;
            double *__restrict__ stats = a.stats + (ROBUST ? 8 : 4) * (size_t)s;
            const double before = st->before, after = loss;
            int status = 1;
            if (flag == kAlignDead || accepted == 0) status = 0;
            else if (!(after <= before)) status = 2;   // a NaN on either side: rejected
            for (int k = 0; k < NC; k++) {
                const float v = __double2float_rn(NP == 8 ? m[k] / m[8] : m[k]);
                out[k] = status == 1 ? v : in[k];
            }
            if constexpr (PHOTO) {
                a.photo_out[2 * (size_t)s] = status == 1 ? __double2float_rn(g) : 1.0f;
                a.photo_out[2 * (size_t)s + 1] = status == 1 ? __double2float_rn(b) : 0.0f;
            }
            a.status_out[s] = status;
            const bool dead = flag == kAlignDead;
            stats[0] = dead ? 0.0 : before;
            stats[1] = dead ? 0.0 : after;
            stats[2] = dead ? 0.0 : cnt / (double)((long long)a.W * (long long)a.H);
            stats[3] = (double)accepted;
            if constexpr (ROBUST) {
                stats[4] = dead ? 0.0 : a.first[2 * (size_t)s];
                stats[5] = dead ? 0.0 : e / cnt;
                stats[6] = dead ? 0.0 : a.first[2 * (size_t)s + 1];
                stats[7] = dead ? 0.0 : wsum / cnt;
            }
            continue;
        }
        if (flag != kAlignLive) continue;
        const double sx = (double)a.w / (double)a.W, sy = (double)a.h / (double)a.H;
        bool frozen = false;
        if (a.mode == kAlignFirst) {
            if (lane == 0) {
                st->before = loss;
                if constexpr (ROBUST) {
                    a.first[2 * (size_t)s] = e / cnt;
                    a.first[2 * (size_t)s + 1] = wsum / cnt;
                }
            }
        } else {
            frozen = cnt < a.min_count;
            // [G | b] of the sums, eliminated without pivoting; every index is a constant once unrolled
            double G[NQ][NQ + 1], q[NQ];
#pragma unroll
            for (int i = 0; i < NQ; i++) {
#pragma unroll
                for (int j = i; j < NQ; j++) {
                    G[i][j] = sum[align_pair(NQ, i, j)];
                    G[j][i] = G[i][j];
                }
                G[i][NQ] = sum[NH + i];
            }
            frozen = !align_eliminate<NQ>(G, q) || frozen;
            // the update in normalised coordinates, conjugated to the level's pixels
            const double Wm1 = (double)(a.w - 1), Hm1 = (double)(a.h - 1);
            const double cx = Wm1 / 2.0, cy = Hm1 / 2.0, sc = (double)max(a.w, a.h) / 2.0;
            double P[9];
#pragma unroll
            for (int k = 0; k < 9; k++) P[k] = 0.0;
#pragma unroll
            for (int k = 0; k < NP; k++) P[k] = -(q[k] / sc);
            double A[9], D[9];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                A[3 * r] = P[3 * r] / sc;
                A[3 * r + 1] = P[3 * r + 1] / sc;
                A[3 * r + 2] = P[3 * r + 2] - (A[3 * r] * cx + A[3 * r + 1] * cy);
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                D[c] = sc * A[c] + cx * A[6 + c];
                D[3 + c] = sc * A[3 + c] + cy * A[6 + c];
                D[6 + c] = A[6 + c];
            }
            D[0] = D[0] + 1.0;
            D[4] = D[4] + 1.0;
            D[8] = D[8] + 1.0;
            const double adj[9] = {D[4] * D[8] - D[5] * D[7], D[2] * D[7] - D[1] * D[8], D[1] * D[5] - D[2] * D[4],
                                   D[5] * D[6] - D[3] * D[8], D[0] * D[8] - D[2] * D[6], D[2] * D[3] - D[0] * D[5],
                                   D[3] * D[7] - D[4] * D[6], D[1] * D[6] - D[0] * D[7], D[0] * D[4] - D[1] * D[3]};
            double I[9], N[9];
#pragma unroll
            for (int k = 0; k < 9; k++) I[k] = adj[k] / adj[8];
            bool ok = true;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    N[3 * r + c] = (m[3 * r] * I[c] + m[3 * r + 1] * I[3 + c]) + m[3 * r + 2] * I[6 + c];
                    ok = ok && __builtin_isfinite(N[3 * r + c]);
                }
            ok = ok && (N[6] * 0.0 + N[7] * 0.0) + N[8] > 0.0 && (N[6] * Wm1 + N[7] * 0.0) + N[8] > 0.0 &&
                 (N[6] * Wm1 + N[7] * Hm1) + N[8] > 0.0 && (N[6] * 0.0 + N[7] * Hm1) + N[8] > 0.0;
            // the last two entries of the solution move g and b; a g' or b' that is not finite or a g' <= 0 freezes the step
            [[maybe_unused]] double gn = g, bn = b;
            if constexpr (PHOTO) {
                gn = g + q[NP];
                bn = b + q[NP + 1];
                ok = ok && __builtin_isfinite(gn) && __builtin_isfinite(bn) && gn > 0.0;
            }
            frozen = frozen || !ok;
            if (!frozen) {
#pragma unroll
                for (int k = 0; k < 9; k++) m[k] = N[k];
                g = gn;
                b = bn;
                accepted++;
            }
            if (frozen || a.last) align_from_level(m, sx, sy);
        }
        if (!frozen && a.nh > 0) align_to_level(m, (double)a.nw / (double)a.W, (double)a.nh / (double)a.H);
        if (lane == 0) {
            for (int k = 0; k < 9; k++) st->m[k] = m[k];
            st->accepted = accepted;
            st->flag = frozen ? kAlignFrozen : kAlignLive;
            if constexpr (PHOTO) {
                a.photo[2 * (size_t)s] = g;
                a.photo[2 * (size_t)s + 1] = b;
            }
        }
    }
}

// ---- the weight map: grid (ceil(H W / 256), min(S, 65535)), block 256 ----
struct AlignWeightsArgs {
    const void *a, *b;      // [S][H][W]
    int H, W, S;
    const float *model;     // [S][6 | 9]
    const float *photo;     // [S][2] gain, bias; NULL without PHOTO
    double delta;
    float *weights;         // [S][H][W]
};

template <class PIX, int NP, bool PHOTO>
__global__ __launch_bounds__(256) void k_align_weights(AlignWeightsArgs a)
{
    constexpr int NC = NP == 8 ? 9 : 6;
    const int H = a.H, W = a.W;
    const unsigned n = (unsigned)H * (unsigned)W;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
    const double Wm1 = (double)(W - 1), Hm1 = (double)(H - 1);
    const double fx = (double)x, fy = (double)y;
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        const float *__restrict__ mf = a.model + (size_t)NC * s;
        const double m0 = (double)mf[0], m1 = (double)mf[1], m2 = (double)mf[2], m3 = (double)mf[3], m4 = (double)mf[4], m5 = (double)mf[5];
        [[maybe_unused]] double m6 = 0.0, m7 = 0.0, m8 = 1.0;
        if constexpr (NP == 8) {
            m6 = (double)mf[6]; m7 = (double)mf[7]; m8 = (double)mf[8];
        }
        const PIX *__restrict__ A = static_cast<const PIX *>(a.a) + (size_t)s * n;
        const PIX *__restrict__ B = static_cast<const PIX *>(a.b) + (size_t)s * n;
        [[maybe_unused]] const double w = (m6 * fx + m7 * fy) + m8;
        const double xa = (m0 * fx + m1 * fy) + m2;
        const double ya = (m3 * fx + m4 * fy) + m5;
        const double xs = NP == 8 ? xa / w : xa;
        const double ys = NP == 8 ? ya / w : ya;
        const bool within = xs >= 0.0 && xs <= Wm1 && ys >= 0.0 && ys <= Hm1;
        const bool ok = NP == 8 ? w > 0.0 && within : within;
        const BilinearTaps t = bilinear_taps(H, W, ys, xs);
        const float smp = bilinear_finish(t, ld_pix<PIX>(B, (unsigned)t.i00), ld_pix<PIX>(B, (unsigned)t.i01),
                                          ld_pix<PIX>(B, (unsigned)t.i10), ld_pix<PIX>(B, (unsigned)t.i11));
        const float t0 = ld_pix<PIX>(A, i);
        double r;
        if constexpr (PHOTO) {
            const double g = (double)a.photo[2 * (size_t)s], b = (double)a.photo[2 * (size_t)s + 1];
            r = (double)smp - (g * (double)t0 + b);
        } else {
            r = (double)(smp - t0);
        }
        const double ar = __builtin_fabs(r);
        const double wt = ar > a.delta ? a.delta / ar : 1.0;
        a.weights[(size_t)s * n + i] = ok ? __double2float_rn(wt) : 0.0f;
    }
}

}  // namespace oflk
