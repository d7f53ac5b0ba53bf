// oflk_align.hpp -- gfx950 device code of direct image alignment (oflk_align_refine, oflk_align_sequence and their host
// forms): inverse-compositional Lucas-Kanade registration of frame B to the template A over the whole frame, coarse to fine,
// from a given affine or homography step model.
//
// The statement is tests/align_model.py (include/oflk.h repeats it).  Everything here is that file's operation in its order,
// every operation rounded on its own; nothing is contracted, there is no atomic and no result depends on the launch
// geometry.  One chain of launches on one stream, nothing passes through the host between iterations:
//
//   k_align_begin          one thread per step: the input model widened into the step's state, or the step marked dead
//   k_align_reduce<PIX, NP>  grid (tiles, steps), one wave per tile of 64 columns x 32 rows.  A lane owns a column and walks
//                          it top to bottom with its NS = 29 (NP = 6) or 46 (NP = 8) float64 sums in registers.  The
//                          template is read coalesced, three values per row (the pixel and its two neighbours: a 3 x 3
//                          window slides down the column in registers and gives the Sobel gradients, so no gradient plane
//                          is written or read); B's four taps are gathered through the cache as k_warp_perspective's.  The
//                          wave combines the 64 columns by the stated tree with shuffles and lane 0 writes the tile's NS
//                          sums.  No LDS, no scratch
//   k_align_update<NP>     one block of 64 per step: lane k adds sum k of the tiles in raster order; then every lane runs the
//                          step's serial part in registers (the refusals, k_homog_refit's elimination on NP rows, the update's
//                          conjugation, the adjugate, the product, the corner test, the level's conjugations) and lane 0
//                          writes the state.  mode 0 records the first full-resolution residual, mode 2 the last one and
//                          writes the outputs; both read the sums of the same reduce kernel
#pragma once
#include "oflk_kernels.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kAlignTileW = 64;   // a tile's columns: one per lane
constexpr int kAlignTileH = 32;   // a tile's rows
constexpr int kAlignLive = 0, kAlignFrozen = 1, kAlignDead = 2;
constexpr int kAlignFirst = 0, kAlignIterate = 1, kAlignLast = 2;   // k_align_update's modes

__host__ __device__ constexpr int align_sums(int NP) { return NP * (NP + 1) / 2 + NP + 2; }
// the place of sd[i] sd[j], i <= j, among the sums: row after row of the upper triangle
__host__ __device__ constexpr int align_pair(int NP, int i, int j) { return i * (2 * NP - i + 1) / 2 + (j - i); }

// a step's state between launches.  m is in frame coordinates between levels and in the level's inside one
struct AlignState {
    double m[9];
    double before;   // the first full-resolution mean squared residual
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

// Gaussian elimination without pivoting on the N x (N + 1) array [G | b], then the back substitution into h: k_homog_refit's
// procedure (tests/homography_model.py, solve8) on N rows, fully unrolled so that no indexed array is left.  A function of its
// own: sharing one with k_homog_refit changed that kernel's register allocation.  false: a pivot is zero or not finite
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

// ---- the sums: grid (tiles, min(S, 65535)), block 64 ----
struct AlignReduceArgs {
    const void *a, *b;         // the level's template and image of step 0
    size_t stride;             // elements from a step's image to the next step's
    int H, W, tiles_x, S;
    int skip_frozen;           // an iteration's sums: a frozen step has none
    const AlignState *state;   // [S]
    double *partial;           // [S][pstride]: a tile's NS sums at tile * NS
    size_t pstride;
};

template <class PIX, int NP>
__global__ __launch_bounds__(64) void k_align_reduce(AlignReduceArgs a)
{
    constexpr int NS = align_sums(NP);
    constexpr int NH = NP * (NP + 1) / 2;
    const int lane = (int)threadIdx.x;
    const int tile = (int)blockIdx.x;
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
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        const AlignState *__restrict__ st = a.state + s;
        const int flag = st->flag;
        if (flag == kAlignDead || (flag == kAlignFrozen && a.skip_frozen)) continue;
        const double m0 = st->m[0], m1 = st->m[1], m2 = st->m[2], m3 = st->m[3], m4 = st->m[4], m5 = st->m[5];
        [[maybe_unused]] double m6 = 0.0, m7 = 0.0, m8 = 1.0;
        if constexpr (NP == 8) {
            m6 = st->m[6]; m7 = st->m[7]; m8 = st->m[8];
        }
        const PIX *__restrict__ A = static_cast<const PIX *>(a.a) + (size_t)s * a.stride;
        const PIX *__restrict__ B = static_cast<const PIX *>(a.b) + (size_t)s * a.stride;
        double acc[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) acc[k] = 0.0;
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
            // compute_gradients' Sobel / 8 (k_gradients: the same taps in the same order, the kernels' zero taps last)
            float ix = ap[2] * -0.125f;
            ix = fmaf(ap[0], 0.125f, ix);
            ix = fmaf(a0[2], -0.25f, ix);
            ix = fmaf(a0[0], 0.25f, ix);
            ix = fmaf(am[2], -0.125f, ix);
            ix = fmaf(am[0], 0.125f, ix);
            float iy = ap[2] * -0.125f;
            iy = fmaf(ap[1], -0.25f, iy);
            iy = fmaf(ap[0], -0.125f, iy);
            iy = fmaf(am[2], 0.125f, iy);
            iy = fmaf(am[1], 0.25f, iy);
            iy = fmaf(am[0], 0.125f, iy);
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
                const double r = (double)(smp - t0);
                const double gx = (double)ix, gy = (double)iy;
                const double yh = (fy - cy) / sc;
                double sd[NP];
                sd[0] = gx * xh; sd[1] = gx * yh; sd[2] = gx;
                sd[3] = gy * xh; sd[4] = gy * yh; sd[5] = gy;
                if constexpr (NP == 8) {
                    const double tt = sd[0] + sd[4];
                    sd[6] = -(tt * xh);
                    sd[7] = -(tt * yh);
                }
#pragma unroll
                for (int p = 0; p < NP; p++)
#pragma unroll
                    for (int q = p; q < NP; q++) acc[align_pair(NP, p, q)] = acc[align_pair(NP, p, q)] + sd[p] * sd[q];
#pragma unroll
                for (int p = 0; p < NP; p++) acc[NH + p] = acc[NH + p] + sd[p] * r;
                acc[NH + NP] = acc[NH + NP] + r * r;
                acc[NH + NP + 1] = acc[NH + NP + 1] + 1.0;
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
            for (int k = 0; k < NS; k++) acc[k] = acc[k] + __shfl_down(acc[k], (unsigned)stride, 64);
        if (lane == 0) {
            double *__restrict__ out = a.partial + (size_t)s * a.pstride + (size_t)tile * NS;
#pragma unroll
            for (int k = 0; k < NS; k++) out[k] = acc[k];
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
    // kAlignLast
    const float *model_in;    // [S][nc]
    float *model_out;         // [S][nc]
    int *status_out;          // [S]
    double *stats;            // [S][4]
};

template <int NP>
__global__ __launch_bounds__(64) void k_align_update(AlignUpdateArgs a)
{
    constexpr int NS = align_sums(NP);
    constexpr int NH = NP * (NP + 1) / 2;
    constexpr int NC = NP == 8 ? 9 : 6;
    __shared__ double sum[NS];
    const int lane = (int)threadIdx.x;
    for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
        AlignState *__restrict__ st = a.state + s;
        const int flag = st->flag;
        const bool summed = flag == kAlignLive || (flag == kAlignFrozen && a.mode != kAlignIterate);
        __syncthreads();   // sum is rewritten
        if (summed && lane < NS) {
            const double *__restrict__ p = a.partial + (size_t)s * a.pstride + lane;
            double t = 0.0;
            for (int i = 0; i < a.tiles; i++) t = t + p[(size_t)i * NS];
            sum[lane] = t;
        }
        __syncthreads();
        double m[9];
        for (int k = 0; k < 9; k++) m[k] = st->m[k];
        int accepted = st->accepted;
        const double e = summed ? sum[NH + NP] : 0.0, cnt = summed ? sum[NH + NP + 1] : 0.0;
        if (a.mode == kAlignLast) {
            if (lane != 0) continue;
            const float *__restrict__ in = a.model_in + (size_t)NC * s;
            float *__restrict__ out = a.model_out + (size_t)NC * s;
            double *__restrict__ stats = a.stats + 4 * (size_t)s;
            const double before = st->before, after = e / cnt;
            int status = 1;
            if (flag == kAlignDead || accepted == 0) status = 0;
            else if (!(after <= before)) status = 2;   // a NaN on either side: rejected
            for (int k = 0; k < NC; k++) {
                const float v = __double2float_rn(NP == 8 ? m[k] / m[8] : m[k]);
                out[k] = status == 1 ? v : in[k];
            }
            a.status_out[s] = status;
            const bool dead = flag == kAlignDead;
            stats[0] = dead ? 0.0 : before;
            stats[1] = dead ? 0.0 : after;
            stats[2] = dead ? 0.0 : cnt / (double)((long long)a.W * (long long)a.H);
            stats[3] = (double)accepted;
            continue;
        }
        if (flag != kAlignLive) continue;
        const double sx = (double)a.w / (double)a.W, sy = (double)a.h / (double)a.H;
        bool frozen = false;
        if (a.mode == kAlignFirst) {
            if (lane == 0) st->before = e / cnt;
        } else {
            frozen = cnt < a.min_count;
            // [G | b] of the sums, eliminated without pivoting; every index is a constant once unrolled
            double G[NP][NP + 1], q[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) {
#pragma unroll
                for (int j = i; j < NP; j++) {
                    G[i][j] = sum[align_pair(NP, i, j)];
                    G[j][i] = G[i][j];
                }
                G[i][NP] = sum[NH + i];
            }
            frozen = !align_eliminate<NP>(G, q) || frozen;
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
            frozen = frozen || !ok;
            if (!frozen) {
#pragma unroll
                for (int k = 0; k < 9; k++) m[k] = N[k];
                accepted++;
            }
            if (frozen || a.last) align_from_level(m, sx, sy);
        }
        if (!frozen && a.nh > 0) align_to_level(m, (double)a.nw / (double)a.W, (double)a.nh / (double)a.H);
        if (lane == 0) {
            for (int k = 0; k < 9; k++) st->m[k] = m[k];
            st->accepted = accepted;
            st->flag = frozen ? kAlignFrozen : kAlignLive;
        }
    }
}

// =============================================================================
// the photometric form (oflk_align_refine_photo, oflk_align_sequence_photo): B under the model looks like g A + b
// =============================================================================
// The statement is tests/align_photo_model.py.  A step carries g and b beside its AlignState, in an array of their own
// (photo [S][2], begun at (1, 0)), so that the kernels above keep their code.  The residual is r = f64(v) - (g a + b) and the
// columns are c = [g sd[0], .., g sd[NP-1], a, 1.0]: NQ = NP + 2 of them, align_sums(NQ) = 46 (affine) or 67 (homography) sums
// in the order of the plain form.
//
//   k_align_photo_begin        one thread per step: (g, b) = (1, 0)
//   k_align_reduce_photo<PIX, NP>  k_align_reduce's tile, column walk, Sobel window and gather.  NP = 6 is one wave with its 46
//                              sums.  NP = 8 is a block of two waves on the same tile: each walks all 64 columns and keeps
//                              one half of the 67 sums (34 and 33), so that a wave stays within 256 registers.  Which wave
//                              holds a sum does not change the sum's order; the sampling and the sd row are computed twice.
//                              No LDS, no barrier: each wave's lane 0 writes its own sums
//   k_align_update_photo<NP>   k_align_update on NQ rows: the first NP entries of the solution move the model as before, the
//                              last two are added to g and b; a g' or b' that is not finite or a g' <= 0 freezes the step.
//                              kAlignLast also writes photo_out

constexpr int align_photo_waves(int NP) { return NP == 8 ? 2 : 1; }

__global__ __launch_bounds__(64) void k_align_photo_begin(int S, double *__restrict__ photo)
{
    const unsigned s = blockIdx.x * 64u + threadIdx.x;
    if (s >= (unsigned)S) return;
    photo[2 * (size_t)s] = 1.0;
    photo[2 * (size_t)s + 1] = 0.0;
}

struct AlignPhotoReduceArgs {
    AlignReduceArgs r;
    const double *photo;   // [S][2]
};

// one wave's walk over its tile for the sums K0 .. K1-1 of step s
template <class PIX, int NP, int K0, int K1>
__device__ __forceinline__ void align_photo_tile(const AlignPhotoReduceArgs &pa, int s, int lane, int tile)
{
    constexpr int NQ = NP + 2;
    constexpr int NH = NQ * (NQ + 1) / 2;
    constexpr int NS = align_sums(NQ);
    constexpr int NK = K1 - K0;
    static_assert(K0 >= 0 && K0 < K1 && K1 <= NS, "a wave's share of the sums");
    const AlignReduceArgs &a = pa.r;
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
    const AlignState *__restrict__ st = a.state + s;
    const double m0 = st->m[0], m1 = st->m[1], m2 = st->m[2], m3 = st->m[3], m4 = st->m[4], m5 = st->m[5];
    [[maybe_unused]] double m6 = 0.0, m7 = 0.0, m8 = 1.0;
    if constexpr (NP == 8) {
        m6 = st->m[6]; m7 = st->m[7]; m8 = st->m[8];
    }
    const double g = pa.photo[2 * (size_t)s], b = pa.photo[2 * (size_t)s + 1];
    const PIX *__restrict__ A = static_cast<const PIX *>(a.a) + (size_t)s * a.stride;
    const PIX *__restrict__ B = static_cast<const PIX *>(a.b) + (size_t)s * a.stride;
    double acc[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) acc[k] = 0.0;
    // sum k, when it is this wave's; k is a constant once the loops are unrolled, so no indexed array is left
    auto add = [&](int k, double v) {
        if (k >= K0 && k < K1) acc[k - K0] = acc[k - K0] + v;
    };
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
        float ix = ap[2] * -0.125f;
        ix = fmaf(ap[0], 0.125f, ix);
        ix = fmaf(a0[2], -0.25f, ix);
        ix = fmaf(a0[0], 0.25f, ix);
        ix = fmaf(am[2], -0.125f, ix);
        ix = fmaf(am[0], 0.125f, ix);
        float iy = ap[2] * -0.125f;
        iy = fmaf(ap[1], -0.25f, iy);
        iy = fmaf(ap[0], -0.125f, iy);
        iy = fmaf(am[2], 0.125f, iy);
        iy = fmaf(am[1], 0.25f, iy);
        iy = fmaf(am[0], 0.125f, iy);
        ix = fmaf(ap[1], 0.0f, ix);
        ix = fmaf(a0[1], 0.0f, ix);
        ix = fmaf(am[1], 0.0f, ix);
        iy = fmaf(a0[2], 0.0f, iy);
        iy = fmaf(a0[1], 0.0f, iy);
        iy = fmaf(a0[0], 0.0f, iy);
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
            const double av = (double)t0;
            const double r = (double)smp - (g * av + b);
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
            for (int p = 0; p < NP; p++) c[p] = g * sd[p];
            c[NP] = av;
            c[NP + 1] = 1.0;
#pragma unroll
            for (int p = 0; p < NQ; p++) {
#pragma unroll
                for (int q = p; q < NQ; q++) add(align_pair(NQ, p, q), c[p] * c[q]);
                add(NH + p, c[p] * r);
            }
            add(NH + NQ, r * r);
            add(NH + NQ + 1, 1.0);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            am[k] = a0[k];
            a0[k] = ap[k];
        }
        t0 = tn;
    }
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

// ---- the photometric sums: grid (tiles, min(S, 65535)), block 64 * align_photo_waves(NP) ----
template <class PIX, int NP>
__global__ __launch_bounds__(64 * align_photo_waves(NP)) void k_align_reduce_photo(AlignPhotoReduceArgs pa)
{
    constexpr int NS = align_sums(NP + 2);
    constexpr int NW = align_photo_waves(NP);
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)blockIdx.x;
    for (int s = blockIdx.y; s < pa.r.S; s += gridDim.y) {
        const int flag = pa.r.state[s].flag;
        if (flag == kAlignDead || (flag == kAlignFrozen && pa.r.skip_frozen)) continue;
        if constexpr (NW == 1) {
            align_photo_tile<PIX, NP, 0, NS>(pa, s, lane, tile);
        } else {
            constexpr int cut = (NS + 1) / 2;
            if (wave == 0)
                align_photo_tile<PIX, NP, 0, cut>(pa, s, lane, tile);
            else
                align_photo_tile<PIX, NP, cut, NS>(pa, s, lane, tile);
        }
    }
}

// ---- the photometric update: grid (min(S, 65535)), block 64 ----
// k_align_update is to stay instruction for instruction what it is, so its serial part is repeated here, not shared with it
struct AlignPhotoUpdateArgs {
    AlignUpdateArgs u;
    double *photo;       // [S][2]
    float *photo_out;    // [S][2], kAlignLast
};

template <int NP>
__global__ __launch_bounds__(64) void k_align_update_photo(AlignPhotoUpdateArgs pa)
{
    constexpr int NQ = NP + 2;
    constexpr int NS = align_sums(NQ);
    constexpr int NH = NQ * (NQ + 1) / 2;
    constexpr int NC = NP == 8 ? 9 : 6;
    __shared__ double sum[NS];
    const AlignUpdateArgs &a = pa.u;
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
        double g = pa.photo[2 * (size_t)s], b = pa.photo[2 * (size_t)s + 1];
        int accepted = st->accepted;
        const double e = summed ? sum[NH + NQ] : 0.0, cnt = summed ? sum[NH + NQ + 1] : 0.0;
        if (a.mode == kAlignLast) {
            if (lane != 0) continue;
            const float *__restrict__ in = a.model_in + (size_t)NC * s;
            float *__restrict__ out = a.model_out + (size_t)NC * s;
            double *__restrict__ stats = a.stats + 4 * (size_t)s;
            const double before = st->before, after = e / cnt;
            int status = 1;
            if (flag == kAlignDead || accepted == 0) status = 0;
            else if (!(after <= before)) status = 2;
            for (int k = 0; k < NC; k++) {
                const float v = __double2float_rn(NP == 8 ? m[k] / m[8] : m[k]);
                out[k] = status == 1 ? v : in[k];
            }
            pa.photo_out[2 * (size_t)s] = status == 1 ? __double2float_rn(g) : 1.0f;
            pa.photo_out[2 * (size_t)s + 1] = status == 1 ? __double2float_rn(b) : 0.0f;
            a.status_out[s] = status;
            const bool dead = flag == kAlignDead;
            stats[0] = dead ? 0.0 : before;
            stats[1] = dead ? 0.0 : after;
            stats[2] = dead ? 0.0 : cnt / (double)((long long)a.W * (long long)a.H);
            stats[3] = (double)accepted;
            continue;
        }
        if (flag != kAlignLive) continue;
        const double sx = (double)a.w / (double)a.W, sy = (double)a.h / (double)a.H;
        bool frozen = false;
        if (a.mode == kAlignFirst) {
            if (lane == 0) st->before = e / cnt;
        } else {
            frozen = cnt < a.min_count;
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
            const double gn = g + q[NP], bn = b + q[NP + 1];
            ok = ok && __builtin_isfinite(gn) && __builtin_isfinite(bn) && gn > 0.0;
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
            pa.photo[2 * (size_t)s] = g;
            pa.photo[2 * (size_t)s + 1] = b;
        }
    }
}

// =============================================================================
// the robust form (oflk_align_refine_robust, oflk_align_sequence_robust, oflk_align_weights): Huber weights on the residuals
// =============================================================================
// The statement is tests/align_robust_model.py.  It is the plain form (PHOTO false: c = sd, NQ = NP) or the photometric one
// (PHOTO true: c = [g sd, a, 1.0], NQ = NP + 2) with one weight per counted pixel, w = |r| > delta ? delta / |r| : 1.0, on the
// left factor of every product of the normal equations, and two more sums behind the base form's: rho and w.  That is
// align_sums(NQ) + 2 sums: 31 / 48 (plain affine / homography) and 48 / 69 (photometric).  rho, not r r, decides the rejection.
//
//   k_align_reduce_robust<PIX, NP, PHOTO>  k_align_reduce's tile, column walk, Sobel window and gather.  w, rho and w c[i] are
//                              formed once per pixel per wave; the division delta / |r| is the only new one.  The
//                              photometric homography's 69 sums are split over two waves of a block as
//                              k_align_reduce_photo's are (35 and 34); the other three forms are one wave
//   k_align_update_robust<NP, PHOTO>  k_align_update_photo's serial part on the new sum layout: before and after are
//                              sum(rho) / count, and the first pass keeps r r / count and sum(w) / count of the input model
//                              in first [S][2] for the eight stats.  PHOTO false carries no g, b
//   k_align_weights<PIX, NP, PHOTO>  one thread per pixel of the frame: f32(w) at counted pixels, 0.0f elsewhere
// k_align_begin, k_align_photo_begin and AlignState are the other forms'.

constexpr int align_robust_columns(int NP, bool PHOTO) { return NP + (PHOTO ? 2 : 0); }
__host__ __device__ constexpr int align_robust_sums(int NP, bool PHOTO) { return align_sums(NP + (PHOTO ? 2 : 0)) + 2; }
constexpr int align_robust_waves(int NP, bool PHOTO) { return NP == 8 && PHOTO ? 2 : 1; }

struct AlignRobustReduceArgs {
    AlignReduceArgs r;
    const double *photo;   // [S][2]; NULL without PHOTO
    double delta;          // f64(f32(robust_delta))
};

// one wave's walk over its tile for the sums K0 .. K1-1 of step s
template <class PIX, int NP, bool PHOTO, int K0, int K1>
__device__ __forceinline__ void align_robust_tile(const AlignRobustReduceArgs &pa, int s, int lane, int tile)
{
    constexpr int NQ = align_robust_columns(NP, PHOTO);
    constexpr int NH = NQ * (NQ + 1) / 2;
    constexpr int NS = align_robust_sums(NP, PHOTO);
    constexpr int NK = K1 - K0;
    static_assert(K0 >= 0 && K0 < K1 && K1 <= NS, "a wave's share of the sums");
    const AlignReduceArgs &a = pa.r;
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
    const double delta = pa.delta;
    const AlignState *__restrict__ st = a.state + s;
    const double m0 = st->m[0], m1 = st->m[1], m2 = st->m[2], m3 = st->m[3], m4 = st->m[4], m5 = st->m[5];
    [[maybe_unused]] double m6 = 0.0, m7 = 0.0, m8 = 1.0;
    if constexpr (NP == 8) {
        m6 = st->m[6]; m7 = st->m[7]; m8 = st->m[8];
    }
    [[maybe_unused]] double g = 1.0, b = 0.0;
    if constexpr (PHOTO) {
        g = pa.photo[2 * (size_t)s];
        b = pa.photo[2 * (size_t)s + 1];
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
        float ix = ap[2] * -0.125f;
        ix = fmaf(ap[0], 0.125f, ix);
        ix = fmaf(a0[2], -0.25f, ix);
        ix = fmaf(a0[0], 0.25f, ix);
        ix = fmaf(am[2], -0.125f, ix);
        ix = fmaf(am[0], 0.125f, ix);
        float iy = ap[2] * -0.125f;
        iy = fmaf(ap[1], -0.25f, iy);
        iy = fmaf(ap[0], -0.125f, iy);
        iy = fmaf(am[2], 0.125f, iy);
        iy = fmaf(am[1], 0.25f, iy);
        iy = fmaf(am[0], 0.125f, iy);
        ix = fmaf(ap[1], 0.0f, ix);
        ix = fmaf(a0[1], 0.0f, ix);
        ix = fmaf(am[1], 0.0f, ix);
        iy = fmaf(a0[2], 0.0f, iy);
        iy = fmaf(a0[1], 0.0f, iy);
        iy = fmaf(a0[0], 0.0f, iy);
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
            const double ar = __builtin_fabs(r);
            const bool big = ar > delta;
            const double wt = big ? delta / ar : 1.0;
            const double rho = big ? delta * (ar - delta * 0.5) : (r * r) * 0.5;
#pragma unroll
            for (int p = 0; p < NQ; p++) {
                const double wc = wt * c[p];
#pragma unroll
                for (int q = p; q < NQ; q++) add(align_pair(NQ, p, q), wc * c[q]);
                add(NH + p, wc * r);
            }
            add(NH + NQ, r * r);
            add(NH + NQ + 1, 1.0);
            add(NH + NQ + 2, rho);
            add(NH + NQ + 3, wt);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            am[k] = a0[k];
            a0[k] = ap[k];
        }
        t0 = tn;
    }
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

// ---- the robust sums: grid (tiles, min(S, 65535)), block 64 * align_robust_waves(NP, PHOTO) ----
template <class PIX, int NP, bool PHOTO>
__global__ __launch_bounds__(64 * align_robust_waves(NP, PHOTO)) void k_align_reduce_robust(AlignRobustReduceArgs pa)
{
    constexpr int NS = align_robust_sums(NP, PHOTO);
    constexpr int NW = align_robust_waves(NP, PHOTO);
    const int lane = (int)(threadIdx.x & 63);
    [[maybe_unused]] const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)blockIdx.x;
    for (int s = blockIdx.y; s < pa.r.S; s += gridDim.y) {
        const int flag = pa.r.state[s].flag;
        if (flag == kAlignDead || (flag == kAlignFrozen && pa.r.skip_frozen)) continue;
        if constexpr (NW == 1) {
            align_robust_tile<PIX, NP, PHOTO, 0, NS>(pa, s, lane, tile);
        } else {
            constexpr int cut = (NS + 1) / 2;
            if (wave == 0)
                align_robust_tile<PIX, NP, PHOTO, 0, cut>(pa, s, lane, tile);
            else
                align_robust_tile<PIX, NP, PHOTO, cut, NS>(pa, s, lane, tile);
        }
    }
}

// ---- the robust update: grid (min(S, 65535)), block 64 ----
// the other updates are to stay instruction for instruction what they are, so the serial part is repeated here once more
struct AlignRobustUpdateArgs {
    AlignUpdateArgs u;   // stats [S][8]
    double *photo;       // [S][2]; NULL without PHOTO
    float *photo_out;    // [S][2], kAlignLast; NULL without PHOTO
    double *first;       // [S][2]: r r / count and sum(w) / count of the first pass
};

template <int NP, bool PHOTO>
__global__ __launch_bounds__(64) void k_align_update_robust(AlignRobustUpdateArgs pa)
{
    constexpr int NQ = align_robust_columns(NP, PHOTO);
    constexpr int NS = align_robust_sums(NP, PHOTO);
    constexpr int NH = NQ * (NQ + 1) / 2;
    constexpr int NC = NP == 8 ? 9 : 6;
    __shared__ double sum[NS];
    const AlignUpdateArgs &a = pa.u;
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
            g = pa.photo[2 * (size_t)s];
            b = pa.photo[2 * (size_t)s + 1];
        }
        int accepted = st->accepted;
        const double e = summed ? sum[NH + NQ] : 0.0, cnt = summed ? sum[NH + NQ + 1] : 0.0;
        const double rho = summed ? sum[NH + NQ + 2] : 0.0, wsum = summed ? sum[NH + NQ + 3] : 0.0;
        if (a.mode == kAlignLast) {
            if (lane != 0) continue;
            const float *__restrict__ in = a.model_in + (size_t)NC * s;
            float *__restrict__ out = a.model_out + (size_t)NC * s;
            double *__restrict__ stats = a.stats + 8 * (size_t)s;
            const double before = st->before, after = rho / cnt;
            int status = 1;
            if (flag == kAlignDead || accepted == 0) status = 0;
            else if (!(after <= before)) status = 2;
            for (int k = 0; k < NC; k++) {
                const float v = __double2float_rn(NP == 8 ? m[k] / m[8] : m[k]);
                out[k] = status == 1 ? v : in[k];
            }
            if constexpr (PHOTO) {
                pa.photo_out[2 * (size_t)s] = status == 1 ? __double2float_rn(g) : 1.0f;
                pa.photo_out[2 * (size_t)s + 1] = status == 1 ? __double2float_rn(b) : 0.0f;
            }
            a.status_out[s] = status;
            const bool dead = flag == kAlignDead;
            stats[0] = dead ? 0.0 : before;
            stats[1] = dead ? 0.0 : after;
            stats[2] = dead ? 0.0 : cnt / (double)((long long)a.W * (long long)a.H);
            stats[3] = (double)accepted;
            stats[4] = dead ? 0.0 : pa.first[2 * (size_t)s];
            stats[5] = dead ? 0.0 : e / cnt;
            stats[6] = dead ? 0.0 : pa.first[2 * (size_t)s + 1];
            stats[7] = dead ? 0.0 : wsum / cnt;
            continue;
        }
        if (flag != kAlignLive) continue;
        const double sx = (double)a.w / (double)a.W, sy = (double)a.h / (double)a.H;
        bool frozen = false;
        if (a.mode == kAlignFirst) {
            if (lane == 0) {
                st->before = rho / cnt;
                pa.first[2 * (size_t)s] = e / cnt;
                pa.first[2 * (size_t)s + 1] = wsum / cnt;
            }
        } else {
            frozen = cnt < a.min_count;
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
                pa.photo[2 * (size_t)s] = g;
                pa.photo[2 * (size_t)s + 1] = b;
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
