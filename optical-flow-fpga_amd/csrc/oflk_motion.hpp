// oflk_motion.hpp -- gfx950 device code of the global fits (oflk_estimate_motion, oflk_tracks_motion, the tracker's motion
// row; oflk_estimate_homography, oflk_tracks_homography): a deterministic RANSAC over point correspondences and a
// least-squares refit, batched over steps, as one kernel family over four models.
//
// The statements are tests/motion_model.py (translation, similarity, affine) and tests/homography_model.py (include/oflk.h
// repeats both): compaction in slot order, counter-based sampling, a minimal solve in float64 rounded to float32, a float32
// score, arg-max with ties to the lowest hypothesis, a centred refit in float64 whose sums have a stated order, and the mask
// of the returned model.  Every operation here is those files', in their order; nothing is contracted.
//
// Three launches on one stream, no atomics, no spin, no communication between blocks:
//   k_motion_compact         one block of 1024 per step: the valid correspondences (px, py, qx, qy) in slot order (ballot and
//                            prefix count) and their number M
//   k_motion_score<MODEL>    grid (ceil(Hn / 4), steps), one wave per hypothesis: every lane draws the sample and solves it
//                            (the same values on all lanes: cheaper than one lane and a broadcast, and the control flow
//                            stays wave-uniform), then the wave walks the M correspondences 64 at a time, four loads in
//                            flight, and counts with ballot and popcount
//   k_motion_refit<MODEL>    one block of 256 per step: arg-max, the refit's sums (thread l holds partial l of the statement,
//                            the tree runs in LDS), the solve on every thread, the final mask and the counts
// Every buffer that is read was written by one of these kernels in the same call; none relies on a memset.
//
// What a model brings is MotionModel<MODEL> (coefficients, sample size, refit sums), motion_inlier and motion_round for its
// coefficient count, motion_minimal<MODEL> (the homography's is a specialisation in oflk_homography.hpp, which every user of
// these kernels includes) and its branch of the refit between the centroids and the rounding.  That branch stands in the
// kernel behind `if constexpr`, not in a function per model: as a function the homography's needed 169 VGPRs instead of
// 159 and lost its third wave per SIMD.
#pragma once
#include "oflk_kernels.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kMotionTranslation = 0, kMotionSimilarity = 1, kMotionAffine = 2;   // = OFLK_MOTION_*
constexpr int kMotionHomography = 3;   // internal: the homography fit has entry points of its own
constexpr int kMotionLanes = 256;      // the refit's partials (LANES of the statement) = k_motion_refit's block
constexpr int kMotionCompact = 1024;   // k_motion_compact's block
constexpr int kMotionWaves = 4;        // hypotheses per block of k_motion_score

// what the kernels need to know of a model at compile time
template <int MODEL>
struct MotionModel {
    static constexpr int coeffs = MODEL == kMotionHomography ? 9 : 6;   // per model, row-major; hmodel's and model's stride
    static constexpr int sample = MODEL + 1;                            // points of a minimal sample
    static constexpr int sums = MODEL == kMotionHomography ? 22 : 7;    // sums of the refit's largest group: rows of `red`
};
constexpr int motion_coeffs(int model) { return model == kMotionHomography ? 9 : 6; }

struct MotionArgs {
    const float2 *src, *dst;                // [S][N]
    const unsigned char *va, *vb, *born;    // [S][N] or NULL: valid = va && vb && !born (a NULL array does not decide)
    int S, N, Hn;
    unsigned index0, seed;                  // step s draws with index index0 + s
    float thr2;                             // threshold * threshold in float32
    int *M;                                 // [S]          workspace
    float4 *pts;                            // [S][N]       (the first M[s] of a step are written and read)
    int *score;                             // [S][Hn]
    float *hmodel;                          // [S][Hn][coeffs]
    float *model;                           // [S][coeffs]  outputs
    unsigned char *inlier;                  // [S][N]
    int *counts;                            // [S][3]
};

__device__ __forceinline__ bool motion_valid(const MotionArgs &a, size_t i, float2 &p, float2 &q)
{
    p = a.src[i];
    q = a.dst[i];
    bool ok = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(q.x) && __builtin_isfinite(q.y);
    if (a.va) ok = ok && a.va[i] != 0;
    if (a.vb) ok = ok && a.vb[i] != 0;
    if (a.born) ok = ok && a.born[i] == 0;
    return ok;
}

__device__ __forceinline__ unsigned motion_fmix(unsigned x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    return x ^ (x >> 16);
}

__device__ __forceinline__ unsigned motion_draw(unsigned seed, unsigned index, unsigned h, unsigned j)
{
    unsigned x = motion_fmix(seed ^ 0x9E3779B9u);
    x = motion_fmix(x + index);
    x = motion_fmix(x + h);
    return motion_fmix(x + j);
}

// the float32 test of the statement, one operation at a time: six coefficients, then nine (the divisions are IEEE)
__device__ __forceinline__ bool motion_inlier(const float (&c)[6], float px, float py, float qx, float qy, float thr2)
{
    const float ex = ((c[0] * px + c[1] * py) + c[2]) - qx;
    const float ey = ((c[3] * px + c[4] * py) + c[5]) - qy;
    const float r2 = ex * ex + ey * ey;
    return r2 <= thr2;
}

__device__ __forceinline__ bool motion_inlier(const float (&c)[9], float px, float py, float qx, float qy, float thr2)
{
    const float w = (c[6] * px + c[7] * py) + c[8];
    const float ex = ((c[0] * px + c[1] * py) + c[2]) / w - qx;
    const float ey = ((c[3] * px + c[4] * py) + c[5]) / w - qy;
    const float r2 = ex * ex + ey * ey;
    return w > 0.0f && r2 <= thr2;
}

// float64 coefficients to float32 -- nine are divided by the last first; false when one is not finite
template <int NC>
__device__ __forceinline__ bool motion_round(const double (&d)[NC], float (&c)[NC])
{
    bool ok = true;
    for (int k = 0; k < NC; k++) {
        c[k] = __double2float_rn(NC == 9 ? d[k] / d[8] : d[k]);
        ok = ok && __builtin_isfinite(c[k]);
    }
    return ok;
}

// the minimal solve of m = MODEL + 1 points; false: degenerate
template <int MODEL>
__device__ __forceinline__ bool motion_minimal(const float4 (&pt)[MODEL + 1], float (&c)[MotionModel<MODEL>::coeffs])
{
    static_assert(MODEL <= kMotionAffine, "the homography's is a specialisation: include oflk_homography.hpp");
    const double p0x = (double)pt[0].x, p0y = (double)pt[0].y, q0x = (double)pt[0].z, q0y = (double)pt[0].w;
    double d[6];
    bool ok = true;
    if constexpr (MODEL == kMotionTranslation) {
        d[0] = 1.0; d[1] = 0.0; d[2] = q0x - p0x;
        d[3] = 0.0; d[4] = 1.0; d[5] = q0y - p0y;
    } else if constexpr (MODEL == kMotionSimilarity) {
        const double dx = (double)pt[1].x - p0x, dy = (double)pt[1].y - p0y;
        const double ex = (double)pt[1].z - q0x, ey = (double)pt[1].w - q0y;
        const double den = dx * dx + dy * dy;
        const double a = (dx * ex + dy * ey) / den;
        const double b = (dx * ey - dy * ex) / den;
        d[0] = a; d[1] = -b; d[2] = q0x - (a * p0x - b * p0y);
        d[3] = b; d[4] = a;  d[5] = q0y - (b * p0x + a * p0y);
        ok = !(den == 0.0);
    } else {
        const double d1x = (double)pt[1].x - p0x, d1y = (double)pt[1].y - p0y, d2x = (double)pt[2].x - p0x, d2y = (double)pt[2].y - p0y;
        const double e1x = (double)pt[1].z - q0x, e1y = (double)pt[1].w - q0y, e2x = (double)pt[2].z - q0x, e2y = (double)pt[2].w - q0y;
        const double det = d1x * d2y - d1y * d2x;
        const double a00 = (e1x * d2y - e2x * d1y) / det;
        const double a01 = (e2x * d1x - e1x * d2x) / det;
        const double a10 = (e1y * d2y - e2y * d1y) / det;
        const double a11 = (e2y * d1x - e1y * d2x) / det;
        d[0] = a00; d[1] = a01; d[2] = q0x - (a00 * p0x + a01 * p0y);
        d[3] = a10; d[4] = a11; d[5] = q0y - (a10 * p0x + a11 * p0y);
        ok = !(det == 0.0);
    }
    return motion_round(d, c) && ok;
}

// ---- 1. compaction: grid (min(S, 65535)), block kMotionCompact ----
__global__ __launch_bounds__(kMotionCompact) void k_motion_compact(MotionArgs a)
{
    constexpr int NW = kMotionCompact / 64;
    __shared__ int wtot[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
        const size_t row = (size_t)s * (size_t)a.N;
        int running = 0;
        for (long base = 0; base < (long)a.N; base += kMotionCompact) {
            const long n = base + tid;
            float2 p = make_float2(0.0f, 0.0f), q = p;
            const bool ok = n < (long)a.N && motion_valid(a, row + (size_t)n, p, q);
            const unsigned long long b = __ballot(ok);
            if (lane == 0) wtot[wave] = __popcll(b);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < NW; w++) {
                const int c = wtot[w];
                before += w < wave ? c : 0;
                total += c;
            }
            if (ok) a.pts[row + (size_t)(running + before + __popcll(b & ((1ull << lane) - 1)))] = make_float4(p.x, p.y, q.x, q.y);
            running += total;
            __syncthreads();   // wtot is rewritten by the next piece
        }
        if (tid == 0) a.M[s] = running;
    }
}

// Pick j of a sample of m <= 4 out of M positions: r = draw % (M - j) is the r-th position not yet picked, so it is bumped
// past the j earlier picks in ascending order.  `asc` holds those sorted and takes the new one in (j is a constant once the
// caller's loop is unrolled: at most three compares and three min / max pairs)
template <int m>
__device__ __forceinline__ int motion_pick(int (&asc)[m], int j, unsigned draw, int M)
{
    int r = (int)(draw % (unsigned)(M - j));
    for (int k = 0; k < j; k++) r += r >= asc[k] ? 1 : 0;
    int x = r;
    for (int k = 0; k < j; k++) {
        const int lo = min(asc[k], x);
        x = max(asc[k], x);
        asc[k] = lo;
    }
    asc[j] = x;
    return r;
}

// ---- 2. scoring: grid (ceil(Hn / kMotionWaves), min(S, 65535)), block 64 * kMotionWaves; no barrier ----
template <int MODEL>
__global__ __launch_bounds__(64 * kMotionWaves) void k_motion_score(MotionArgs a)
{
    constexpr int m = MotionModel<MODEL>::sample, NC = MotionModel<MODEL>::coeffs;
    const int lane = threadIdx.x & 63;
    const int h = (int)blockIdx.x * kMotionWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (h >= a.Hn) return;
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        const int M = a.M[s];
        const float4 *pts = a.pts + (size_t)s * (size_t)a.N;
        const float nan = __builtin_nanf("");
        float c[NC];
        for (int k = 0; k < NC; k++) c[k] = nan;
        int count = -1;
        bool ok = M >= m;
        if (ok) {
            int asc[m];
            float4 pt[m];
#pragma unroll
            for (int j = 0; j < m; j++)
                pt[j] = pts[motion_pick(asc, j, motion_draw(a.seed, a.index0 + (unsigned)s, (unsigned)h, (unsigned)j), M)];
            ok = motion_minimal<MODEL>(pt, c);
        }
        if (ok) {
            count = 0;
            for (int i0 = 0; i0 < M; i0 += 256) {
                float4 v[4];
                bool in[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + 64 * u + lane;
                    in[u] = i < M;
                    v[u] = in[u] ? pts[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    count += __popcll(__ballot(in[u] && motion_inlier(c, v[u].x, v[u].y, v[u].z, v[u].w, a.thr2)));
            }
        }
        if (lane == 0) {
            const size_t o = (size_t)s * (size_t)a.Hn + (size_t)h;
            a.score[o] = count;
            for (int k = 0; k < NC; k++) a.hmodel[NC * o + k] = ok ? c[k] : nan;
        }
    }
}

// the fixed tree of the statement over `rows` arrays of kMotionLanes doubles; all threads call it, the sums end in red[k][0]
template <int ROWS, int CAP>
__device__ __forceinline__ void motion_tree(double (&red)[CAP][kMotionLanes], int tid)
{
    __syncthreads();
    for (int st = kMotionLanes / 2; st >= 1; st >>= 1) {
        if (tid < st)
            for (int k = 0; k < ROWS; k++) red[k][tid] = red[k][tid] + red[k][tid + st];
        __syncthreads();
    }
}

__device__ __forceinline__ int motion_int_sum(int (&ired)[kMotionLanes], int tid, int v)
{
    __syncthreads();   // earlier readers of ired are done
    ired[tid] = v;
    __syncthreads();
    for (int st = kMotionLanes / 2; st >= 1; st >>= 1) {
        if (tid < st) ired[tid] += ired[tid + st];
        __syncthreads();
    }
    return ired[0];
}

// the largest of a step's Hn scores into bs and its hypothesis into bh, ties to the lowest h: a thread meets its h
// ascending, the tree compares (score, h).  All threads call it
__device__ __forceinline__ void motion_argmax(const int *score, int Hn, int (&ired)[kMotionLanes], int (&ibest)[kMotionLanes], int tid,
                                              int &bs, int &bh)
{
    bs = -1;
    bh = 0x7fffffff;
    for (int h = tid; h < Hn; h += kMotionLanes) {
        const int sc = score[h];
        if (sc > bs) {
            bs = sc;
            bh = h;
        }
    }
    __syncthreads();   // the previous step's readers of ired are done
    ired[tid] = bs;
    ibest[tid] = bh;
    __syncthreads();
    for (int st = kMotionLanes / 2; st >= 1; st >>= 1) {
        if (tid < st) {
            const int os = ired[tid + st], oh = ibest[tid + st];
            if (os > ired[tid] || (os == ired[tid] && oh < ibest[tid])) {
                ired[tid] = os;
                ibest[tid] = oh;
            }
        }
        __syncthreads();
    }
    bs = ired[0];
    bh = ibest[0];
}

// ---- 3. select and refit: grid (min(S, 65535)), block kMotionLanes ----
template <int MODEL>
__global__ __launch_bounds__(kMotionLanes) void k_motion_refit(MotionArgs a)
{
    constexpr int NC = MotionModel<MODEL>::coeffs, SUMS = MotionModel<MODEL>::sums;
    __shared__ double red[SUMS][kMotionLanes];
    __shared__ int ired[kMotionLanes], ibest[kMotionLanes];
    const int tid = threadIdx.x;
    const float nan = __builtin_nanf("");
    for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
        const size_t row = (size_t)s * (size_t)a.N;
        const int M = a.M[s];
        const float4 *pts = a.pts + row;
        int bs, bh;
        motion_argmax(a.score + (size_t)s * (size_t)a.Hn, a.Hn, ired, ibest, tid, bs, bh);
        if (bs < 0) {   // M < m, or every hypothesis degenerate (uniform over the block)
            for (long n = tid; n < (long)a.N; n += kMotionLanes) a.inlier[row + (size_t)n] = 0;
            if (tid < NC) a.model[NC * (size_t)s + tid] = nan;
            if (tid < 3) a.counts[3 * (size_t)s + tid] = tid == 1 ? M : 0;
            continue;
        }
        float c[NC];
        for (int k = 0; k < NC; k++) c[k] = a.hmodel[NC * ((size_t)s * (size_t)a.Hn + (size_t)bh) + k];

        // the count and the coordinate sums over the best hypothesis's inliers: partial tid, positions ascending
        double acc[SUMS];
        for (int k = 0; k < 4; k++) acc[k] = 0.0;
        int cnt = 0;
        for (int i = tid; i < M; i += kMotionLanes) {
            const float4 v = pts[i];
            if (motion_inlier(c, v.x, v.y, v.z, v.w, a.thr2)) {
                cnt++;
                acc[0] = acc[0] + (double)v.x;
                acc[1] = acc[1] + (double)v.y;
                acc[2] = acc[2] + (double)v.z;
                acc[3] = acc[3] + (double)v.w;
            }
        }
        const int n = motion_int_sum(ired, tid, cnt);
        for (int k = 0; k < 4; k++) red[k][tid] = acc[k];
        motion_tree<4>(red, tid);
        const double nn = (double)n;
        const double cpx = red[0][0] / nn, cpy = red[1][0] / nn, cqx = red[2][0] / nn, cqy = red[3][0] / nn;
        __syncthreads();   // red is rewritten

        // the model's own sums, in the same order, and its solve in float64
        double d[NC];
        bool ok = n > 0;
        if constexpr (MODEL == kMotionHomography) {
            // (b) the L1 spreads about the centroids
            acc[0] = 0.0;
            acc[1] = 0.0;
            for (int i = tid; i < M; i += kMotionLanes) {
                const float4 v = pts[i];
                if (motion_inlier(c, v.x, v.y, v.z, v.w, a.thr2)) {
                    acc[0] = acc[0] + (fabs((double)v.x - cpx) + fabs((double)v.y - cpy));
                    acc[1] = acc[1] + (fabs((double)v.z - cqx) + fabs((double)v.w - cqy));
                }
            }
            for (int k = 0; k < 2; k++) red[k][tid] = acc[k];
            motion_tree<2>(red, tid);
            const double lp = red[0][0], lq = red[1][0];
            const double sp = nn / lp, sq = nn / lq;
            __syncthreads();   // red is rewritten

            // (c), (d) the 22 sums of the normal equations over the normalised coordinates
#pragma unroll
            for (int k = 0; k < SUMS; k++) acc[k] = 0.0;
            for (int i = tid; i < M; i += kMotionLanes) {
                const float4 p = pts[i];
                if (motion_inlier(c, p.x, p.y, p.z, p.w, a.thr2)) {
                    const double x = ((double)p.x - cpx) * sp, y = ((double)p.y - cpy) * sp;
                    const double u = ((double)p.z - cqx) * sq, v = ((double)p.w - cqy) * sq;
                    const double xx = x * x, xy = x * y, yy = y * y, r = u * u + v * v;
                    acc[0] = acc[0] + xx;       acc[1] = acc[1] + xy;       acc[2] = acc[2] + yy;
                    acc[3] = acc[3] + x;        acc[4] = acc[4] + y;
                    acc[5] = acc[5] + xx * u;   acc[6] = acc[6] + xy * u;   acc[7] = acc[7] + yy * u;
                    acc[8] = acc[8] + x * u;    acc[9] = acc[9] + y * u;
                    acc[10] = acc[10] + xx * v; acc[11] = acc[11] + xy * v; acc[12] = acc[12] + yy * v;
                    acc[13] = acc[13] + x * v;  acc[14] = acc[14] + y * v;
                    acc[15] = acc[15] + xx * r; acc[16] = acc[16] + xy * r; acc[17] = acc[17] + yy * r;
                    acc[18] = acc[18] + u;      acc[19] = acc[19] + v;
                    acc[20] = acc[20] + x * r;  acc[21] = acc[21] + y * r;
                }
            }
#pragma unroll
            for (int k = 0; k < SUMS; k++) red[k][tid] = acc[k];
            motion_tree<SUMS>(red, tid);
            const double Sxx = red[0][0], Sxy = red[1][0], Syy = red[2][0], Sx = red[3][0], Sy = red[4][0];
            const double Sxxu = red[5][0], Sxyu = red[6][0], Syyu = red[7][0], Sxu = red[8][0], Syu = red[9][0];
            const double Sxxv = red[10][0], Sxyv = red[11][0], Syyv = red[12][0], Sxv = red[13][0], Syv = red[14][0];
            const double Sxxr = red[15][0], Sxyr = red[16][0], Syyr = red[17][0];
            const double Su = red[18][0], Sv = red[19][0], Sxr = red[20][0], Syr = red[21][0];

            // (e) [G | b], eliminated without pivoting; every index is a constant once unrolled
            double G[8][9] = {{Sxx, Sxy, Sx, 0.0, 0.0, 0.0, -Sxxu, -Sxyu, Sxu},
                              {Sxy, Syy, Sy, 0.0, 0.0, 0.0, -Sxyu, -Syyu, Syu},
                              {Sx, Sy, nn, 0.0, 0.0, 0.0, -Sxu, -Syu, Su},
                              {0.0, 0.0, 0.0, Sxx, Sxy, Sx, -Sxxv, -Sxyv, Sxv},
                              {0.0, 0.0, 0.0, Sxy, Syy, Sy, -Sxyv, -Syyv, Syv},
                              {0.0, 0.0, 0.0, Sx, Sy, nn, -Sxv, -Syv, Sv},
                              {-Sxxu, -Sxyu, -Sxu, -Sxxv, -Sxyv, -Sxv, Sxxr, Sxyr, -Sxr},
                              {-Sxyu, -Syyu, -Syu, -Sxyv, -Syyv, -Syv, Sxyr, Syyr, -Syr}};
            ok = ok && !(lp == 0.0) && !(lq == 0.0);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const double piv = G[k][k];
                ok = ok && !(piv == 0.0) && __builtin_isfinite(piv);
#pragma unroll
                for (int i = k + 1; i < 8; i++) {
                    const double g = G[i][k] / piv;
#pragma unroll
                    for (int j = k + 1; j < 9; j++) G[i][j] = G[i][j] - g * G[k][j];
                }
            }
            double hn[9];
            hn[8] = 1.0;
#pragma unroll
            for (int i = 7; i >= 0; i--) {
                double t = G[i][8];
#pragma unroll
                for (int j = i + 1; j < 8; j++) t = t - G[i][j] * hn[j];
                hn[i] = t / G[i][i];
            }

            // (f) d = T_q^-1 (Hn T_p), entry by entry
            const double tx = sp * cpx, ty = sp * cpy;
            double A[9];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                A[3 * r] = hn[3 * r] * sp;
                A[3 * r + 1] = hn[3 * r + 1] * sp;
                A[3 * r + 2] = hn[3 * r + 2] - (hn[3 * r] * tx + hn[3 * r + 1] * ty);
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                d[k] = A[k] / sq + cqx * A[6 + k];
                d[3 + k] = A[3 + k] / sq + cqy * A[6 + k];
                d[6 + k] = A[6 + k];
            }
            ok = ok && !(d[8] == 0.0);
        } else {
            if (MODEL != kMotionTranslation) {
                for (int k = 0; k < 7; k++) acc[k] = 0.0;
                for (int i = tid; i < M; i += kMotionLanes) {
                    const float4 v = pts[i];
                    if (motion_inlier(c, v.x, v.y, v.z, v.w, a.thr2)) {
                        const double ux = (double)v.x - cpx, uy = (double)v.y - cpy, vx = (double)v.z - cqx, vy = (double)v.w - cqy;
                        acc[0] = acc[0] + ux * ux;
                        acc[1] = acc[1] + ux * uy;
                        acc[2] = acc[2] + uy * uy;
                        acc[3] = acc[3] + ux * vx;
                        acc[4] = acc[4] + uy * vx;
                        acc[5] = acc[5] + ux * vy;
                        acc[6] = acc[6] + uy * vy;
                    }
                }
                for (int k = 0; k < 7; k++) red[k][tid] = acc[k];
                motion_tree<7>(red, tid);
            }
            const double suu = red[0][0], suv = red[1][0], svv = red[2][0], sux = red[3][0], svx = red[4][0], suy = red[5][0],
                         svy = red[6][0];
            if constexpr (MODEL == kMotionTranslation) {
                d[0] = 1.0; d[1] = 0.0; d[2] = cqx - cpx;
                d[3] = 0.0; d[4] = 1.0; d[5] = cqy - cpy;
            } else if constexpr (MODEL == kMotionSimilarity) {
                const double den = suu + svv;
                const double sa = (sux + svy) / den;
                const double sb = (suy - svx) / den;
                d[0] = sa; d[1] = -sb; d[2] = cqx - (sa * cpx - sb * cpy);
                d[3] = sb; d[4] = sa;  d[5] = cqy - (sb * cpx + sa * cpy);
                ok = ok && !(den == 0.0);
            } else {
                const double det = suu * svv - suv * suv;
                const double a00 = (sux * svv - svx * suv) / det;
                const double a01 = (svx * suu - sux * suv) / det;
                const double a10 = (suy * svv - svy * suv) / det;
                const double a11 = (svy * suu - suy * suv) / det;
                d[0] = a00; d[1] = a01; d[2] = cqx - (a00 * cpx + a01 * cpy);
                d[3] = a10; d[4] = a11; d[5] = cqy - (a10 * cpx + a11 * cpy);
                ok = ok && !(det == 0.0);
            }
        }
        float f[NC];
        ok = motion_round(d, f) && ok;
        if (!ok)   // the refit is singular: the best hypothesis's model stays
            for (int k = 0; k < NC; k++) f[k] = c[k];

        // the mask of the returned model over the valid correspondences, and the counts
        cnt = 0;
        for (long j = tid; j < (long)a.N; j += kMotionLanes) {
            float2 p, q;
            const bool in = motion_valid(a, row + (size_t)j, p, q) && motion_inlier(f, p.x, p.y, q.x, q.y, a.thr2);
            a.inlier[row + (size_t)j] = in ? 1 : 0;
            cnt += in ? 1 : 0;
        }
        const int ni = motion_int_sum(ired, tid, cnt);
        if (tid == 0) {
            for (int k = 0; k < NC; k++) a.model[NC * (size_t)s + k] = f[k];
            a.counts[3 * (size_t)s] = ni;
            a.counts[3 * (size_t)s + 1] = M;
            a.counts[3 * (size_t)s + 2] = 1;
        }
    }
}

// the motion row of a tracker that has no step yet (frame 0, or the first frame after a reset): the M < m result of M = 0
__global__ __launch_bounds__(256) void k_motion_none(float *model, unsigned char *inlier, int *counts, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) inlier[i] = 0;
    if (i < 6) model[i] = __builtin_nanf("");
    if (i < 3) counts[i] = 0;
}

}  // namespace oflk
