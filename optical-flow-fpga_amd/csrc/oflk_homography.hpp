// oflk_homography.hpp -- what the homography brings to the fit's kernel family (oflk_motion.hpp) from outside it: only its
// minimal solve, the kMotionHomography specialisation of motion_minimal.  The kernels (k_motion_compact,
// k_motion_score<MODEL>, k_motion_refit<MODEL>), the nine-coefficient inlier test, the rounding and the homography's branch
// of the refit are oflk_motion.hpp's.  The perspective warp's coordinates (oflk_warp_perspective) belong to the same
// models; their kernel is k_warp_perspective in oflk_stabilize.hpp, beside the affine one whose layout and sampler it shares.
//
// The statement is tests/homography_model.py (include/oflk.h repeats it): the motion fit's compaction and sampling with a
// four-point sample, a closed-form minimal solve in float64 (two unit-square-to-quadrilateral maps, an adjugate and a
// product), a float32 score with one division per coordinate, arg-max with ties to the lowest hypothesis, a normalised
// linear refit in float64 whose 28 sums have the motion fit's stated order and whose 8 x 8 normal equations are eliminated
// without pivoting, and the mask of the returned model.  Every operation here is that file's, in its order; nothing is
// contracted.
//
// In k_motion_score<kMotionHomography> every lane draws the four picks and solves them here (the compiler orders the solve
// so that 56 VGPRs suffice: eight waves per SIMD, no scratch) before the shared walk with the dividing test.
#pragma once
#include "oflk_motion.hpp"

#pragma clang fp contract(off)

namespace oflk {

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
template <>
__device__ __forceinline__ bool motion_minimal<kMotionHomography>(const float4 (&pt)[4], float (&c)[9])
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
    return motion_round(Hm, c) && ok;
}

}  // namespace oflk
