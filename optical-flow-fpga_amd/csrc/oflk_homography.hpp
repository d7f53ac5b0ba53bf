// oflk_homography.hpp -- gfx950 device code of the homography fit (oflk_estimate_homography, oflk_tracks_homography) and of
// the perspective warp's coordinates (oflk_warp_perspective; its kernel is k_warp_perspective in oflk_stabilize.hpp, beside
// the affine one whose layout and sampler it shares).
//
// The statement is tests/homography_model.py (include/oflk.h repeats it): the motion fit's compaction and sampling with a
// four-point sample, a closed-form minimal solve in float64 (two unit-square-to-quadrilateral maps, an adjugate and a
// product), a float32 score with one division per coordinate, arg-max with ties to the lowest hypothesis, a normalised
// linear refit in float64 whose 28 sums have the motion fit's stated order and whose 8 x 8 normal equations are eliminated
// without pivoting, and the mask of the returned model.  Every operation here is that file's, in its order; nothing is
// contracted.
//
// Three launches on one stream, no atomics, no spin, no communication between blocks; the arguments are MotionArgs with
// nine coefficients per model (hmodel [S][Hn][9], model [S][9]):
//   k_motion_compact   unchanged (oflk_motion.hpp)
//   k_homog_score      grid (ceil(Hn / 4), steps), one wave per hypothesis, the shape of k_motion_score: every lane draws the
//                      four picks and solves them (the compiler orders the solve so that 56 VGPRs suffice: eight waves per
//                      SIMD, no scratch), then the wave walks the M correspondences 64 at a time, four loads in flight, and
//                      counts with ballot and popcount
//   k_homog_refit      one block of 256 per step: arg-max, then three passes over the correspondences with thread l
//                      holding partial l of the statement and the tree in LDS -- the count and four coordinate sums, the
//                      two L1 spreads, the 22 sums of the normal equations in one group (22 x 256 doubles = 44 KB of static
//                      LDS) --, the elimination in registers on every thread (fully unrolled: no indexed array is left;
//                      159 VGPRs, no scratch, three waves per SIMD), the final mask and the counts
#pragma once
#include "oflk_motion.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kHomogSample = 4;   // points of a minimal sample
constexpr int kHomogSums = 22;    // distinct sums of the refit's normal equations

// the float32 test of the statement, one operation at a time; the divisions are IEEE
__device__ __forceinline__ bool homog_inlier(const float (&c)[9], float px, float py, float qx, float qy, float thr2)
{
    const float w = (c[6] * px + c[7] * py) + c[8];
    const float ex = ((c[0] * px + c[1] * py) + c[2]) / w - qx;
    const float ey = ((c[3] * px + c[4] * py) + c[5]) / w - qy;
    const float r2 = ex * ex + ey * ey;
    return w > 0.0f && r2 <= thr2;
}

// nine float64 entries divided by the last and rounded to float32; false when one is not finite
__device__ __forceinline__ bool homog_round(const double (&d)[9], float (&c)[9])
{
    bool ok = true;
    for (int k = 0; k < 9; k++) {
        c[k] = __double2float_rn(d[k] / d[8]);
        ok = ok && __builtin_isfinite(c[k]);
    }
    return ok;
}

// the map of the unit square onto the quadrilateral (x0, y0) .. (x3, y3), row-major in Q; returns its denominator
__device__ __forceinline__ double homog_square_to_quad(const double (&x)[4], const double (&y)[4], double (&Q)[9])
{
    const double sx = (x[0] - x[1]) + (x[2] - x[3]);
    const double sy = (y[0] - y[1]) + (y[2] - y[3]);
    const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], dy1 = y[1] - y[2], dy2 = y[3] - y[2];
    const double den = dx1 * dy2 - dy1 * dx2;
    const double g = (sx * dy2 - sy * dx2) / den;
    const double h = (dx1 * sy - dy1 * sx) / den;
    Q[0] = (x[1] - x[0]) + g * x[1]; Q[1] = (x[3] - x[0]) + h * x[3]; Q[2] = x[0];
    Q[3] = (y[1] - y[0]) + g * y[1]; Q[4] = (y[3] - y[0]) + h * y[3]; Q[5] = y[0];
    Q[6] = g;                        Q[7] = h;                        Q[8] = 1.0;
    return den;
}

// the minimal solve of four points (x, y) -> (z, w); false: degenerate
__device__ __forceinline__ bool homog_minimal(const float4 (&pt)[kHomogSample], float (&c)[9])
{
    double px[4], py[4], qx[4], qy[4];
    for (int k = 0; k < 4; k++) {
        px[k] = (double)pt[k].x; py[k] = (double)pt[k].y;
        qx[k] = (double)pt[k].z; qy[k] = (double)pt[k].w;
    }
    double S[9], D[9];
    const double dens = homog_square_to_quad(px, py, S);
    const double dend = homog_square_to_quad(qx, qy, D);
    // the adjugate of S: nine cofactors, transposed
    const double A[9] = {S[4] * S[8] - S[5] * S[7], S[2] * S[7] - S[1] * S[8], S[1] * S[5] - S[2] * S[4],
                         S[5] * S[6] - S[3] * S[8], S[0] * S[8] - S[2] * S[6], S[2] * S[3] - S[0] * S[5],
                         S[3] * S[7] - S[4] * S[6], S[1] * S[6] - S[0] * S[7], S[0] * S[4] - S[1] * S[3]};
    double Hm[9];
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) Hm[3 * r + k] = (D[3 * r] * A[k] + D[3 * r + 1] * A[3 + k]) + D[3 * r + 2] * A[6 + k];
    const bool ok = !(dens == 0.0) && !(dend == 0.0) && !(Hm[8] == 0.0);
    return homog_round(Hm, c) && ok;
}

// ---- 2. scoring: grid (ceil(Hn / kMotionWaves), min(S, 65535)), block 64 * kMotionWaves; no barrier ----
__global__ __launch_bounds__(64 * kMotionWaves) void k_homog_score(MotionArgs a)
{
    constexpr int m = kHomogSample;
    const int lane = threadIdx.x & 63;
    const int h = (int)blockIdx.x * kMotionWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (h >= a.Hn) return;
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        const int M = a.M[s];
        const float4 *pts = a.pts + (size_t)s * (size_t)a.N;
        const float nan = __builtin_nanf("");
        float c[9] = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
        int count = -1;
        bool ok = M >= m;
        if (ok) {
            // pick j: r = draw % (M - j), the r-th position not yet picked, ascending
            int pos[m] = {0, 0, 0, 0};
            for (int j = 0; j < m; j++) {
                int r = (int)(motion_draw(a.seed, a.index0 + (unsigned)s, (unsigned)h, (unsigned)j) % (unsigned)(M - j));
                if (j == 1) {
                    r += r >= pos[0] ? 1 : 0;
                } else if (j == 2) {
                    const int lo = min(pos[0], pos[1]), hi = max(pos[0], pos[1]);
                    r += r >= lo ? 1 : 0;
                    r += r >= hi ? 1 : 0;
                } else if (j == 3) {
                    const int lo2 = min(pos[0], pos[1]), hi2 = max(pos[0], pos[1]);
                    const int lo = min(lo2, pos[2]), mid = max(lo2, min(hi2, pos[2])), hi = max(hi2, pos[2]);
                    r += r >= lo ? 1 : 0;
                    r += r >= mid ? 1 : 0;
                    r += r >= hi ? 1 : 0;
                }
                pos[j] = r;
            }
            float4 pt[m];
            for (int j = 0; j < m; j++) pt[j] = pts[pos[j]];
            ok = homog_minimal(pt, c);
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
                    count += __popcll(__ballot(in[u] && homog_inlier(c, v[u].x, v[u].y, v[u].z, v[u].w, a.thr2)));
            }
        }
        if (lane == 0) {
            const size_t o = (size_t)s * (size_t)a.Hn + (size_t)h;
            a.score[o] = count;
            for (int k = 0; k < 9; k++) a.hmodel[9 * o + k] = ok ? c[k] : nan;
        }
    }
}

// ---- 3. select and refit: grid (min(S, 65535)), block kMotionLanes ----
__global__ __launch_bounds__(kMotionLanes) void k_homog_refit(MotionArgs a)
{
    __shared__ double red[kHomogSums][kMotionLanes];
    __shared__ int ired[kMotionLanes], ibest[kMotionLanes];
    const int tid = threadIdx.x;
    const float nan = __builtin_nanf("");
    for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
        const size_t row = (size_t)s * (size_t)a.N;
        const int M = a.M[s];
        const float4 *pts = a.pts + row;
        int bs, bh;
        motion_argmax(a.score + (size_t)s * (size_t)a.Hn, a.Hn, ired, ibest, tid, bs, bh);
        if (bs < 0) {   // M < 4, or every hypothesis degenerate (uniform over the block)
            for (long n = tid; n < (long)a.N; n += kMotionLanes) a.inlier[row + (size_t)n] = 0;
            if (tid < 9) a.model[9 * (size_t)s + tid] = nan;
            if (tid < 3) a.counts[3 * (size_t)s + tid] = tid == 1 ? M : 0;
            continue;
        }
        float c[9];
        for (int k = 0; k < 9; k++) c[k] = a.hmodel[9 * ((size_t)s * (size_t)a.Hn + (size_t)bh) + k];

        // (a) the count and the coordinate sums over the best hypothesis's inliers: partial tid, positions ascending
        double acc[kHomogSums];
        for (int k = 0; k < 4; k++) acc[k] = 0.0;
        int cnt = 0;
        for (int i = tid; i < M; i += kMotionLanes) {
            const float4 v = pts[i];
            if (homog_inlier(c, v.x, v.y, v.z, v.w, a.thr2)) {
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

        // (b) the L1 spreads about the centroids
        acc[0] = 0.0;
        acc[1] = 0.0;
        for (int i = tid; i < M; i += kMotionLanes) {
            const float4 v = pts[i];
            if (homog_inlier(c, v.x, v.y, v.z, v.w, a.thr2)) {
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
        for (int k = 0; k < kHomogSums; k++) acc[k] = 0.0;
        for (int i = tid; i < M; i += kMotionLanes) {
            const float4 p = pts[i];
            if (homog_inlier(c, p.x, p.y, p.z, p.w, a.thr2)) {
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
        for (int k = 0; k < kHomogSums; k++) red[k][tid] = acc[k];
        motion_tree<kHomogSums>(red, tid);
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
        bool ok = n > 0 && !(lp == 0.0) && !(lq == 0.0);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double piv = G[k][k];
            ok = ok && !(piv == 0.0) && __builtin_isfinite(piv);
#pragma unroll
            for (int i = k + 1; i < 8; i++) {
                const double f = G[i][k] / piv;
#pragma unroll
                for (int j = k + 1; j < 9; j++) G[i][j] = G[i][j] - f * G[k][j];
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

        // (f) B = T_q^-1 (Hn T_p), entry by entry
        const double tx = sp * cpx, ty = sp * cpy;
        double A[9], B[9];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            A[3 * r] = hn[3 * r] * sp;
            A[3 * r + 1] = hn[3 * r + 1] * sp;
            A[3 * r + 2] = hn[3 * r + 2] - (hn[3 * r] * tx + hn[3 * r + 1] * ty);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            B[k] = A[k] / sq + cqx * A[6 + k];
            B[3 + k] = A[3 + k] / sq + cqy * A[6 + k];
            B[6 + k] = A[6 + k];
        }
        float f[9];
        ok = homog_round(B, f) && ok && !(B[8] == 0.0);
        if (!ok)   // the refit is singular: the best hypothesis's model stays
            for (int k = 0; k < 9; k++) f[k] = c[k];

        // the mask of the returned model over the valid correspondences, and the counts
        cnt = 0;
        for (long j = tid; j < (long)a.N; j += kMotionLanes) {
            float2 p, q;
            const bool in = motion_valid(a, row + (size_t)j, p, q) && homog_inlier(f, p.x, p.y, q.x, q.y, a.thr2);
            a.inlier[row + (size_t)j] = in ? 1 : 0;
            cnt += in ? 1 : 0;
        }
        const int ni = motion_int_sum(ired, tid, cnt);
        if (tid == 0) {
            for (int k = 0; k < 9; k++) a.model[9 * (size_t)s + k] = f[k];
            a.counts[3 * (size_t)s] = ni;
            a.counts[3 * (size_t)s + 1] = M;
            a.counts[3 * (size_t)s + 2] = 1;
        }
    }
}

}  // namespace oflk
