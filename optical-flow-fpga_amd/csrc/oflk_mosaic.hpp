// oflk_mosaic.hpp -- gfx950 device code of the video mosaic (oflk_mosaic_chain, oflk_mosaic_accumulate, oflk_mosaic_resolve and
// the host and sequence calls made of them): the step homographies composed from an anchor frame, every frame gathered onto
// one canvas under its chained map, and the canvas reduced to one picture.
//
// The statement is tests/mosaic_model.py (include/oflk.h repeats it).  Everything here is float64 in that file's operation
// order, every operation rounded on its own; nothing is contracted, there is no transcendental and no atomic, and no result
// depends on the launch geometry or on how the frames are cut into calls.
//
//   k_mosaic_chain      one block, two working lanes: lane 0 walks from the anchor to frame T-1, lane 1 from the anchor to
//                       frame 0, each composing P and Q of its side, boxing the frame's corners and carrying its side's drop
//                       flag.  No workspace; the launch can be captured
//   k_mosaic_accumulate<PIX, BLEND>  a gather.  A lane owns kMosaicPx consecutive canvas pixels of a row and keeps their
//                       sum / wsum / count in registers: read once, every frame of the call added in ascending order, written
//                       once.  No two lanes touch one canvas pixel, so there is no atomic and the order is the statement's.  A
//                       wave owns a tile of 64 x 4 canvas pixels (16 lanes across, 4 rows), a block of 256 four such tiles
//                       stacked: 64 x 16.  Frames go in groups of 64: lane l tests frame 64 g + l against the wave's tile
//                       (mosaic_touches: a few dozen float64 operations, the price of two pixels, for a tile of 256), one ballot
//                       gives the set of frames that may touch the tile, and the walk over its set bits is wave-uniform, so a
//                       frame's nine coefficients come through the scalar cache.  The per-pixel body is warp_frames' under a
//                       3 x 3 map (bilinear_taps / bilinear_finish), with the state update in place of the store
//   k_mosaic_resolve<PIX, VEC>  streaming: a lane reads the state of kMosaicPx pixels, divides, and stores them at once (VEC:
//                       the row length a multiple of kMosaicPx and the outputs aligned to a lane's store) or one by one;
//                       bytes through mosaic_store_value, which saturates: the one uint8 store here whose value can leave
//                       [0, 255]
//   k_mosaic_median<PIX, EXPOSURE>  the temporal median (oflk_mosaic_median; the statement is tests/mosaic_median_model.py): all
//                       frames resident, one launch, no state: a pixel's samples as sortable keys in a column of LDS and a
//                       bitwise selection there.  Its comment is at the end of this file
//
// The state (private to this file and to mosaic_state in oflk.hip): three planes of pitch Wp = Wc rounded up to kMosaicPx,
// [Hc][Wp] float64 sum, [Hc][Wp] float64 wsum, [Hc][Wp] int32 count, each plane on a 256-byte boundary.  A lane's pixels are
// therefore aligned to its 32-byte (16-byte) access in every row whatever Wc is; the pad columns are read and written like
// pixels and never resolved.  All-zero bytes are the empty canvas.
//
// The cull (DESIGN.md section 4 has the argument).  w, xa, ya, xa - (W-1) w and ya - (H-1) w are affine in (fx, fy), so their
// extremes over the tile's rectangle are at its corners.  The float64 evaluation of one of them, at any point of the
// rectangle, differs from its exact value by less than 2^-50 S, S the sum of the magnitudes of its terms at the rectangle's
// largest |fx|, |fy|.  A frame is skipped only when S < 2^500 for all of them, w >= 2^-47 S_w + 2^-400 at all four corners, and
// one of xa <= -m, ya <= -m, xa - (W-1) w >= m, ya - (H-1) w >= m holds at all four corners with m = 2^-47 S + 2^-400 of that
// expression.  Then every pixel of the tile has w > 0 and a quotient on the outer side of the frame's edge by more than the
// division's rounding, which is what the statement calls outside.  Anything else -- a corner with w <= 0, a NaN (every
// comparison with it is false), coefficients that large -- is not skipped, and not skipping is always right.
#pragma once
#include "oflk_stabilize.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kMosaicPx = 4;          // consecutive canvas pixels of a lane
constexpr int kMosaicTileW = 64;      // a wave's tile: 16 lanes x kMosaicPx across ...
constexpr int kMosaicTileH = 4;       // ... and 4 rows
constexpr int kMosaicBlockH = 16;     // a block's: four waves stacked
constexpr int kMosaicChainBlock = 64; // k_mosaic_chain's block: one wave, two lanes at work

__device__ __forceinline__ void mosaic_identity(double (&m)[9])
{
    m[0] = 1.0; m[1] = 0.0; m[2] = 0.0;
    m[3] = 0.0; m[4] = 1.0; m[5] = 0.0;
    m[6] = 0.0; m[7] = 0.0; m[8] = 1.0;
}

__device__ __forceinline__ bool mosaic_finite(const double (&m)[9])
{
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && __builtin_isfinite(m[k]);
    return ok;
}

// step s and its inverse (the adjugate over its last entry), both the identity when the step is held; returns held
__device__ __forceinline__ bool mosaic_step(const float *__restrict__ model, const int *__restrict__ counts, size_t s, double (&a)[9],
                                            double (&b)[9])
{
    bool ok = !counts || counts[3 * s + 2] != 0;
    for (int k = 0; k < 9; k++) a[k] = (double)model[9 * s + k];
    ok = ok && mosaic_finite(a);
    const double adj[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    for (int k = 0; k < 9; k++) b[k] = adj[k] / adj[8];
    ok = ok && !(adj[8] == 0.0) && mosaic_finite(b);
    if (!ok) {
        mosaic_identity(a);
        mosaic_identity(b);
    }
    return !ok;
}

// c = x o y (y first), the nine entries divided by the last
__device__ __forceinline__ void mosaic_compose(const double (&x)[9], const double (&y)[9], double (&c)[9])
{
    double t[9];
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) t[3 * r + k] = (x[3 * r] * y[k] + x[3 * r + 1] * y[3 + k]) + x[3 * r + 2] * y[6 + k];
    for (int k = 0; k < 9; k++) c[k] = t[k] / t[8];
}

// ---- the chain: grid (1), block kMosaicChainBlock ----
// Lane 0: frames a, a+1 .. T-1.  Lane 1: frames a-1 .. 0.  One instruction stream, the side a parameter.
__global__ __launch_bounds__(kMosaicChainBlock) void k_mosaic_chain(const float *__restrict__ model, const int *__restrict__ counts,
                                                                   int T, int anchor, int H, int W, double extent,
                                                                   double *__restrict__ from_anchor, double *__restrict__ to_anchor,
                                                                   double *__restrict__ box, unsigned char *__restrict__ held,
                                                                   unsigned char *__restrict__ dropped)
{
    const int side = (int)threadIdx.x;
    if (side > 1) return;
    const bool fwd = side == 0;
    const int n = fwd ? T - 1 - anchor : anchor;   // frames beyond the anchor on this side
    const double Wm1 = (double)(W - 1), Hm1 = (double)(H - 1);
    const double cx[4] = {0.0, Wm1, Wm1, 0.0}, cy[4] = {0.0, 0.0, Hm1, Hm1};
    double P[9], Q[9], a[9], b[9], t[9];
    mosaic_identity(P);
    mosaic_identity(Q);
    bool gone = false;
    for (int i = fwd ? 0 : 1; i <= n; i++) {
        const int f = fwd ? anchor + i : anchor - i;
        if (i > 0) {
            const size_t s = (size_t)(fwd ? f - 1 : f);
            const bool h = mosaic_step(model, counts, s, a, b);
            if (held) held[s] = h ? 1 : 0;
            if (fwd) {   // P_t = A_{t-1} o P_{t-1};  Q_t = Q_{t-1} o B_{t-1}
                mosaic_compose(a, P, t);
                for (int k = 0; k < 9; k++) P[k] = t[k];
                mosaic_compose(Q, b, t);
                for (int k = 0; k < 9; k++) Q[k] = t[k];
            } else {     // P_t = B_t o P_{t+1};  Q_t = Q_{t+1} o A_t
                mosaic_compose(b, P, t);
                for (int k = 0; k < 9; k++) P[k] = t[k];
                mosaic_compose(Q, a, t);
                for (int k = 0; k < 9; k++) Q[k] = t[k];
            }
        }
        double X[4], Y[4];
        bool bad = !(mosaic_finite(P) && mosaic_finite(Q));
        for (int c = 0; c < 4; c++) {
            const double w = (Q[6] * cx[c] + Q[7] * cy[c]) + Q[8];
            X[c] = ((Q[0] * cx[c] + Q[1] * cy[c]) + Q[2]) / w;
            Y[c] = ((Q[3] * cx[c] + Q[4] * cy[c]) + Q[5]) / w;
            bad = bad || !(w > 0.0) || !__builtin_isfinite(w) || !__builtin_isfinite(X[c]) || !__builtin_isfinite(Y[c]) ||
                  fabs(X[c]) > extent || fabs(Y[c]) > extent;
        }
        gone = (gone || bad) && i > 0;
        const double nan = __builtin_nan("");
        const size_t o = (size_t)f;
        for (int k = 0; k < 9; k++) {
            from_anchor[9 * o + k] = P[k];
            to_anchor[9 * o + k] = Q[k];
        }
        box[4 * o] = gone ? nan : fmin(fmin(X[0], X[1]), fmin(X[2], X[3]));
        box[4 * o + 1] = gone ? nan : fmin(fmin(Y[0], Y[1]), fmin(Y[2], Y[3]));
        box[4 * o + 2] = gone ? nan : fmax(fmax(X[0], X[1]), fmax(X[2], X[3]));
        box[4 * o + 3] = gone ? nan : fmax(fmax(Y[0], Y[1]), fmax(Y[2], Y[3]));
        dropped[o] = gone ? 1 : 0;
    }
}

// ---- the canvas state ----
struct MosaicState {
    double *sum, *wsum;   // [Hc][Wp]
    int *count;           // [Hc][Wp]
    int Wp;               // the pitch: Wc rounded up to kMosaicPx
};

template <class PIX>
struct MosaicArgs {
    const PIX *in;               // [F][H][W]
    const double *map;           // [F][9]
    const unsigned char *skip;   // [F] or NULL
    MosaicState st;
    int F, H, W;
    int x0, y0, Hc, Wc;
    int tiles_x;                 // blocks across the canvas
};

// May frame m touch the rectangle [X0, X1] x [Y0, Y1] of map coordinates?  false (the frame is skipped) only when the argument
// at the head of this file shows that every point of it is outside.
__device__ __forceinline__ bool mosaic_touches(const double *__restrict__ m, double X0, double X1, double Y0, double Y1, double Wm1,
                                            double Hm1)
{
    constexpr double kRel = 0x1p-47, kAbs = 0x1p-400, kBig = 0x1p500;
    const double ax = fmax(fabs(X0), fabs(X1)), ay = fmax(fabs(Y0), fabs(Y1));
    const double Sw = (fabs(m[6]) * ax + fabs(m[7]) * ay) + fabs(m[8]);
    const double Sx = (fabs(m[0]) * ax + fabs(m[1]) * ay) + fabs(m[2]);
    const double Sy = (fabs(m[3]) * ax + fabs(m[4]) * ay) + fabs(m[5]);
    const double Sr = Sx + Wm1 * Sw, Sb = Sy + Hm1 * Sw;
    if (!(Sr < kBig && Sb < kBig)) return true;   // also a NaN or an infinity among the coefficients
    const double mw = kRel * Sw + kAbs, mx = kRel * Sx + kAbs, my = kRel * Sy + kAbs, mr = kRel * Sr + kAbs, mb = kRel * Sb + kAbs;
    bool front = true, left = true, right = true, top = true, bottom = true;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double fx = (c & 1) ? X1 : X0, fy = (c & 2) ? Y1 : Y0;
        const double w = (m[6] * fx + m[7] * fy) + m[8];
        const double xa = (m[0] * fx + m[1] * fy) + m[2];
        const double ya = (m[3] * fx + m[4] * fy) + m[5];
        front = front && w >= mw;
        left = left && xa <= -mx;
        top = top && ya <= -my;
        right = right && xa - Wm1 * w >= mr;
        bottom = bottom && ya - Hm1 * w >= mb;
    }
    return !(front && (left || right || top || bottom));
}

enum { kMosaicMean = 0, kMosaicFeather = 1, kMosaicFirst = 2, kMosaicLast = 3 };

// the exposure-compensated form's arguments: frame f's sample s enters the blend as eg_f * f64(s) + eb_f
template <class PIX>
struct MosaicExposureArgs : MosaicArgs<PIX> {
    const double *exposure;   // [F][2]: (eg, eb)
};

// ---- accumulate: grid (tiles_x * ceil(Hc / kMosaicBlockH)), block 256 ----
// EXPOSURE: ARGS is MosaicExposureArgs and the sample is taken to the anchor's exposure first, one multiply and one add, each
// rounded; everything else is the plain form's, whose instantiations keep their code and their kernel arguments
template <class PIX, int BLEND, bool EXPOSURE = false, class ARGS = MosaicArgs<PIX>>
__global__ __launch_bounds__(256) void k_mosaic_accumulate(ARGS a)
{
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int bx = (int)(blockIdx.x % (unsigned)a.tiles_x), by = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int tx = bx * kMosaicTileW, ty = by * kMosaicBlockH + wave * kMosaicTileH;
    if (ty >= a.Hc) return;   // the whole wave
    const int x = tx + (lane & 15) * kMosaicPx, y = ty + (lane >> 4);
    const bool live = y < a.Hc && x < a.st.Wp;   // a lane that is not computes (its taps are clamped) and touches no state
    const size_t at = (size_t)(live ? y : 0) * (size_t)a.st.Wp + (size_t)(live ? x : 0);
    double sum[kMosaicPx], wsum[kMosaicPx];
    int cnt[kMosaicPx];
    {
        const double4 s4 = live ? *reinterpret_cast<const double4 *>(a.st.sum + at) : make_double4(0.0, 0.0, 0.0, 0.0);
        const double4 w4 = live ? *reinterpret_cast<const double4 *>(a.st.wsum + at) : make_double4(0.0, 0.0, 0.0, 0.0);
        const int4 c4 = live ? *reinterpret_cast<const int4 *>(a.st.count + at) : make_int4(0, 0, 0, 0);
        sum[0] = s4.x; sum[1] = s4.y; sum[2] = s4.z; sum[3] = s4.w;
        wsum[0] = w4.x; wsum[1] = w4.y; wsum[2] = w4.z; wsum[3] = w4.w;
        cnt[0] = c4.x; cnt[1] = c4.y; cnt[2] = c4.z; cnt[3] = c4.w;
    }
    const double Wm1 = (double)(a.W - 1), Hm1 = (double)(a.H - 1);
    // the tile's rectangle in map coordinates (the whole tile, also where it hangs over the canvas) and the lane's own
    const double X0 = (double)((long)a.x0 + (long)tx), X1 = (double)((long)a.x0 + (long)(tx + kMosaicTileW - 1));
    const double Y0 = (double)((long)a.y0 + (long)ty), Y1 = (double)((long)a.y0 + (long)(ty + kMosaicTileH - 1));
    const double fy = (double)((long)a.y0 + (long)y);
    double fxk[kMosaicPx];
#pragma unroll
    for (int k = 0; k < kMosaicPx; k++) fxk[k] = (double)((long)a.x0 + (long)(x + k));
    const size_t plane = (size_t)a.H * (size_t)a.W;

    for (int f0 = 0; f0 < a.F; f0 += 64) {
        const int fl = f0 + lane;
        bool keep = fl < a.F;
        if (keep && a.skip) keep = a.skip[fl] == 0;
        if (keep) keep = mosaic_touches(a.map + 9 * (size_t)fl, X0, X1, Y0, Y1, Wm1, Hm1);
        unsigned long long todo = __ballot(keep);
        while (todo) {
            const int f = f0 + (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            // the source position: the expressions of warp_row<true> and warp_source<true> (oflk_stabilize.hpp), repeated here:
            // through the helper two instantiations of this kernel went from 100 / 102 to 114 VGPRs
            const double *__restrict__ m = a.map + 9 * (size_t)f;
            const double m0 = m[0], m2 = m[2], m3 = m[3], m5 = m[5], m6 = m[6], m8 = m[8];
            const double bx1 = m[1] * fy, by1 = m[4] * fy, bw = m[7] * fy;
            const PIX *__restrict__ img = a.in + (size_t)f * plane;
            [[maybe_unused]] double eg = 1.0, eb = 0.0;
            if constexpr (EXPOSURE) {
                eg = a.exposure[2 * (size_t)f];
                eb = a.exposure[2 * (size_t)f + 1];
            }
#pragma unroll
            for (int k = 0; k < kMosaicPx; k++) {
                const double fx = fxk[k];
                const double w = (m6 * fx + bw) + m8;
                const double xa = (m0 * fx + bx1) + m2;
                const double ya = (m3 * fx + by1) + m5;
                const double xs = xa / w;
                const double ys = ya / w;
                const bool ok = w > 0.0 && xs >= 0.0 && xs <= Wm1 && ys >= 0.0 && ys <= Hm1;
                const BilinearTaps t = bilinear_taps(a.H, a.W, ys, xs);
                const float s = bilinear_finish(t, ld_pix<PIX>(img, (unsigned)t.i00), ld_pix<PIX>(img, (unsigned)t.i01),
                                                ld_pix<PIX>(img, (unsigned)t.i10), ld_pix<PIX>(img, (unsigned)t.i11));
                double sd = (double)s;
                if constexpr (EXPOSURE) sd = eg * sd + eb;
                if constexpr (BLEND == kMosaicMean) {
                    sum[k] = ok ? sum[k] + sd : sum[k];
                    wsum[k] = ok ? wsum[k] + 1.0 : wsum[k];
                } else if constexpr (BLEND == kMosaicFeather) {
                    const double g = fmin(fmin(xs, Wm1 - xs), fmin(ys, Hm1 - ys)) + 1.0;
                    sum[k] = ok ? sum[k] + g * sd : sum[k];
                    wsum[k] = ok ? wsum[k] + g : wsum[k];
                } else if constexpr (BLEND == kMosaicFirst) {
                    const bool set = ok && cnt[k] == 0;
                    sum[k] = set ? sd : sum[k];
                    wsum[k] = set ? 1.0 : wsum[k];
                } else {
                    sum[k] = ok ? sd : sum[k];
                    wsum[k] = ok ? 1.0 : wsum[k];
                }
                cnt[k] += ok ? 1 : 0;
            }
        }
    }
    if (live) {
        *reinterpret_cast<double4 *>(a.st.sum + at) = make_double4(sum[0], sum[1], sum[2], sum[3]);
        *reinterpret_cast<double4 *>(a.st.wsum + at) = make_double4(wsum[0], wsum[1], wsum[2], wsum[3]);
        *reinterpret_cast<int4 *>(a.st.count + at) = make_int4(cnt[0], cnt[1], cnt[2], cnt[3]);
    }
}

// ---- resolve: grid (ceil(Hc * (Wp / kMosaicPx) / 256)), block 256 ----
template <class PIX>
struct MosaicResolveArgs {
    MosaicState st;
    PIX *out;     // [Hc][Wc]
    int *count;   // [Hc][Wc] or NULL
    int Hc, Wc;
};

// The resolve's own conversion.  What a warp or an interpolation stores is a convex combination of bytes and lies in [0, 255];
// sum / wsum does not: an exposure takes a sample anywhere, and a state accumulated from float32 frames can be resolved to
// bytes.  uint8: 0 for a NaN (r >= 0 is false), otherwise rint(v), half to even, held to [0, 255]; -0 converts to 0
__device__ __forceinline__ float mosaic_store_value(float v, float) { return v; }
__device__ __forceinline__ unsigned char mosaic_store_value(float v, unsigned char)
{
    const float r = rintf(v);
    return (unsigned char)(r >= 0.0f ? (r <= 255.0f ? r : 255.0f) : 0.0f);
}

template <class PIX, bool VEC>
__global__ __launch_bounds__(256) void k_mosaic_resolve(MosaicResolveArgs<PIX> a)
{
    const unsigned quads = (unsigned)(a.st.Wp / kMosaicPx);
    const size_t q = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= (size_t)a.Hc * quads) return;
    const int y = (int)(q / quads), x = (int)(q % quads) * kMosaicPx;
    const size_t at = (size_t)y * (size_t)a.st.Wp + (size_t)x;
    const double4 s4 = *reinterpret_cast<const double4 *>(a.st.sum + at);
    const double4 w4 = *reinterpret_cast<const double4 *>(a.st.wsum + at);
    const int4 c4 = *reinterpret_cast<const int4 *>(a.st.count + at);
    const double s[kMosaicPx] = {s4.x, s4.y, s4.z, s4.w}, w[kMosaicPx] = {w4.x, w4.y, w4.z, w4.w};
    const int c[kMosaicPx] = {c4.x, c4.y, c4.z, c4.w};
    PIX v[kMosaicPx];
#pragma unroll
    for (int k = 0; k < kMosaicPx; k++) v[k] = mosaic_store_value(c[k] > 0 ? __double2float_rn(s[k] / w[k]) : 0.0f, PIX());
    const size_t o = (size_t)y * (size_t)a.Wc + (size_t)x;
    if constexpr (VEC) {
        if constexpr (sizeof(PIX) == 4) {
            *reinterpret_cast<float4 *>(a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            *reinterpret_cast<unsigned *>(a.out + o) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
        }
        if (a.count) *reinterpret_cast<int4 *>(a.count + o) = c4;
    } else {
#pragma unroll
        for (int k = 0; k < kMosaicPx; k++)
            if (x + k < a.Wc) {
                a.out[o + k] = v[k];
                if (a.count) a.count[o + k] = c[k];
            }
    }
}

// ---- the temporal median: grid (tiles_x * ceil(Hc / kMedianTileH)), block 256 ----
// The statement is tests/mosaic_median_model.py.  A lane owns one canvas pixel, a wave a tile of 16 x 4, a block four such
// tiles side by side: 64 x 4.  The walk over the frames is k_mosaic_accumulate's (the cull on the wave's tile, 64 frames a
// ballot, the per-pixel source expressions repeated once more); what a covering frame leaves is not a sum but the uint32 key
// of its value, which goes to the lane's column of LDS, keys[wave][slot][lane]: the bank is the lane, so no access
// conflicts, no lane reads another's and no barrier is needed.  A lane indexes no private array, so nothing goes to scratch.
//
// The column is kept sorted: a key is inserted where it belongs, the larger ones moving up one slot (one straight-line sweep
// of min and max over the slots, whose LDS reads do not depend on one another), and once the column is full a key enters only
// by pushing the largest out.  After one walk the column therefore holds the kMedianCap smallest keys of the pixel; the ranks (n-1)/2 and n/2 are read off when they are below kMedianCap, which they are for every pixel that up
// to 2 kMedianCap - 1 frames cover.  Otherwise the walk is repeated (the gather is deterministic) for the keys above the
// largest one held, T: the pass counts the keys <= T -- those beyond the column's are all equal to T, so a rank below the
// count is T itself -- and collects the kMedianCap smallest keys above T, and so on: ceil((n/2 + 1) / kMedianCap) walks, and
// only in the waves that have such a pixel.  Equal keys are equal bytes, so where a tie lands does not show, and neither does
// the order the keys came in.
//
// kMedianCap keys a pixel is 32 KiB a block: 5 blocks a CU by LDS, all of its 160 KiB.  The kernel has 114 VGPRs, which is 4
// waves a SIMD: the sweep unrolled over all 32 slots keeps its reads in flight together.  Unrolled by 8 it has fewer registers and 5 waves
// and is 11 - 14 % slower on both scenes of tools/mosaic_bench.py.
constexpr int kMedianCap = 32;     // keys of a pixel in LDS (oflk_mosaic_median_capacity)
constexpr int kMedianTileW = 16;   // a wave's tile: 16 lanes across ...
constexpr int kMedianTileH = 4;    // ... and 4 rows
constexpr int kMedianBlockW = 64;  // a block's: four waves side by side

template <class PIX>
struct MosaicMedianArgs {
    const PIX *in;               // [F][H][W], all resident
    const double *map;           // [F][9]
    const unsigned char *skip;   // [F] or NULL
    const double *exposure;      // [F][2] (EXPOSURE) or unused
    PIX *out;                    // [Hc][Wc]
    int *count;                  // [Hc][Wc] or NULL
    int F, H, W;
    int x0, y0, Hc, Wc;
    int tiles_x;                 // blocks across the canvas
};

// the order of the statement: ascending keys are -NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN
__device__ __forceinline__ unsigned median_key(float e)
{
    const unsigned b = __float_as_uint(e);
    return (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
}

__device__ __forceinline__ float median_value(unsigned key)
{
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

// every frame that may touch the wave's tile, ascending: sink(covers, key) once per such frame for the lane's pixel (fx, fy)
template <class PIX, bool EXPOSURE, class SINK>
__device__ __forceinline__ void mosaic_median_walk(const MosaicMedianArgs<PIX> &a, int lane, double X0, double X1, double Y0, double Y1,
                                                   double fx, double fy, SINK &&sink)
{
    const double Wm1 = (double)(a.W - 1), Hm1 = (double)(a.H - 1);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    for (int f0 = 0; f0 < a.F; f0 += 64) {
        const int fl = f0 + lane;
        bool keep = fl < a.F;
        if (keep && a.skip) keep = a.skip[fl] == 0;
        if (keep) keep = mosaic_touches(a.map + 9 * (size_t)fl, X0, X1, Y0, Y1, Wm1, Hm1);
        unsigned long long todo = __ballot(keep);
        while (todo) {
            const int f = f0 + (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            // the source position: k_mosaic_accumulate's expressions, repeated here as they are there
            const double *__restrict__ m = a.map + 9 * (size_t)f;
            const double m0 = m[0], m2 = m[2], m3 = m[3], m5 = m[5], m6 = m[6], m8 = m[8];
            const double bx1 = m[1] * fy, by1 = m[4] * fy, bw = m[7] * fy;
            const PIX *__restrict__ img = a.in + (size_t)f * plane;
            const double w = (m6 * fx + bw) + m8;
            const double xa = (m0 * fx + bx1) + m2;
            const double ya = (m3 * fx + by1) + m5;
            const double xs = xa / w;
            const double ys = ya / w;
            const bool ok = w > 0.0 && xs >= 0.0 && xs <= Wm1 && ys >= 0.0 && ys <= Hm1;
            const BilinearTaps t = bilinear_taps(a.H, a.W, ys, xs);
            float e = bilinear_finish(t, ld_pix<PIX>(img, (unsigned)t.i00), ld_pix<PIX>(img, (unsigned)t.i01),
                                      ld_pix<PIX>(img, (unsigned)t.i10), ld_pix<PIX>(img, (unsigned)t.i11));
            if constexpr (EXPOSURE) {
                const double eg = a.exposure[2 * (size_t)f], eb = a.exposure[2 * (size_t)f + 1];
                e = __double2float_rn(eg * (double)e + eb);
            }
            sink(ok, median_key(e));
        }
    }
}

template <class PIX, bool EXPOSURE>
__global__ __launch_bounds__(256) void k_mosaic_median(MosaicMedianArgs<PIX> a)
{
    __shared__ unsigned keys[4][kMedianCap][64];
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int bx = (int)(blockIdx.x % (unsigned)a.tiles_x), by = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int tx = bx * kMedianBlockW + wave * kMedianTileW, ty = by * kMedianTileH;
    if (tx >= a.Wc) return;   // the whole wave; there is no barrier below
    const int x = tx + (lane & 15), y = ty + (lane >> 4);
    const bool live = y < a.Hc && x < a.Wc;   // a lane that is not computes (its taps are clamped) and stores nothing
    // the tile's rectangle in map coordinates (the whole tile, also where it hangs over the canvas) and the lane's own pixel
    const double X0 = (double)((long)a.x0 + (long)tx), X1 = (double)((long)a.x0 + (long)(tx + kMedianTileW - 1));
    const double Y0 = (double)((long)a.y0 + (long)ty), Y1 = (double)((long)a.y0 + (long)(ty + kMedianTileH - 1));
    const double fx = (double)((long)a.x0 + (long)x), fy = (double)((long)a.y0 + (long)y);
    unsigned(*col)[64] = keys[wave];

    int n = 0;
    unsigned k_lo = 0u, k_hi = 0u, T = 0u;
    bool got_lo = false, got_hi = false;
    bool above = false;   // wave-uniform: this is a later walk, for the keys above T
    for (;;) {
        int m = 0, le = 0, seen = 0;   // keys in the column, keys <= T, covering frames
        unsigned top = 0xFFFFFFFFu;    // the column's last slot
        const bool idle = got_lo && got_hi;
#pragma unroll
        for (int j = 0; j < kMedianCap; j++) col[j][lane] = 0xFFFFFFFFu;   // an empty slot holds the largest key there is
        mosaic_median_walk<PIX, EXPOSURE>(a, lane, X0, X1, Y0, Y1, fx, fy, [&](bool ok, unsigned key) {
            const bool below = above && key <= T;
            seen += ok ? 1 : 0;
            le += ok && below ? 1 : 0;
            // the insertion, straight-line: the key is carried up the column, every slot keeps the smaller of the two and
            // hands on the larger; what falls off the end is the largest.  The reads do not wait for one another
            if (ok && !below && !idle && (m < kMedianCap || key < top)) {
                unsigned carry = key;
#pragma unroll
                for (int j = 0; j < kMedianCap; j++) {
                    const unsigned c = col[j][lane];
                    top = min(c, carry);
                    carry = max(c, carry);
                    col[j][lane] = top;
                }
                m = min(m + 1, kMedianCap);
            }
        });
        n = seen;
        const int r_lo = n > 0 ? (n - 1) >> 1 : 0, r_hi = n >> 1;
        if (!got_lo && (r_lo < le || r_lo - le < m || n == 0)) {
            k_lo = r_lo < le || n == 0 ? T : col[r_lo - le][lane];
            got_lo = true;
        }
        if (!got_hi && (r_hi < le || r_hi - le < m || n == 0)) {
            k_hi = r_hi < le || n == 0 ? T : col[r_hi - le][lane];
            got_hi = true;
        }
        if (__ballot(!(got_lo && got_hi)) == 0ull) break;
        T = m == kMedianCap ? top : 0xFFFFFFFFu;   // a lane with a rank to find has a full column
        above = true;
    }
    const float e_lo = median_value(k_lo), e_hi = median_value(k_hi);
    const float mid = __double2float_rn(((double)e_lo + (double)e_hi) * 0.5);
    const float v = n == 0 ? 0.0f : ((n & 1) ? e_lo : mid);
    if (live) {
        const size_t o = (size_t)y * (size_t)a.Wc + (size_t)x;
        a.out[o] = mosaic_store_value(v, PIX());
        if (a.count) a.count[o] = n;
    }
}

}  // namespace oflk
