// oflk_nv12.hpp -- gfx950 device code of NV12 video (oflk_warp_affine_nv12, oflk_warp_perspective_nv12, the NV12 sequence call
// and the NV12 online stabiliser made of them): a frame is H W 3 / 2 contiguous bytes, Y[H][W] followed by UV[H/2][W/2][2]
// (U at byte 0, V at byte 1), H and W even, and every result is tied byte for byte to what the planar entry points return for
// the Y plane under the map and for the U and V planes under the map restated in chroma coordinates.
//
// The statement is tests/nv12_model.py (include/oflk.h repeats it).
//
//   k_warp_nv12<PERSP, VEC>  one launch for both planes of all F frames.  Blocks with blockIdx.x < ceil(H / 4) do luma: block
//                       (x, y) is warp_frames' (oflk_stabilize.hpp) on the Y plane, its u8 lane shape and operations, four
//                       pixels a lane, one dword stored.  The blocks above do chroma, never both: chroma block number
//                       (blockIdx.x - ceil(H / 4)) gridDim.y + blockIdx.y counts the (row group, column block) pairs of
//                       the H/2 x W/2 plane row group first, so the narrower plane leaves no empty block columns behind.
//                       A chroma lane forms mc from the frame's map (nv12_chroma_map: a few float64 operations per frame,
//                       no second map buffer), then position, test and weights once per chroma pixel (bilinear_taps on the
//                       H/2 x W/2 plane), gathers each tap as one 2-byte load that holds U and V, runs bilinear_finish
//                       twice on the one set of weights, selects 128 outside and stores its four pixels.
//                       VEC counts the planes whose lanes store at once: 0 none, 1 luma (W % 4 == 0, out and inside
//                       4-byte aligned: a dword of Y and a dword of inside), 2 both (W % 8 == 0 and out 8-byte aligned as
//                       well: a chroma lane's four pairs as one dwordx2).  They are separate kernels for k_warp_affine's
//                       reason.
//
// A tap's address: the UV plane begins H W bytes into the frame and pair i lies 2 i bytes behind that, i <= H W / 4 - 1, so
// a 2-byte load at it ends at the frame's last byte at the latest: no load leaves the frame and no last-pixel case arises.
// Byte offsets inside a frame are 32-bit (H W < 2^30, checked on the host, so H W 3 / 2 < 2^31); offsets across frames 64-bit.
#pragma once
#include "oflk_stabilize.hpp"

#pragma clang fp contract(off)

namespace oflk {

struct WarpNv12Args {
    const unsigned char *in;   // [F][H W 3 / 2]
    const double *map;         // [F][6]; PERSP: [F][9]
    unsigned char *out;        // [F][H W 3 / 2]
    unsigned char *inside;     // [F][H][W] or NULL
    int F, H, W;
    double sx, sy;             // the siting: chroma sample (i, j) sits at luma (2 i + sx, 2 j + sy)
    unsigned luma_groups;      // ceil(H / 4): the blockIdx.x below which a block does luma
    unsigned chroma_cols;      // ceil((W / 2) / (64 kWarpPx)): column blocks of the chroma plane
};

struct __attribute__((packed)) TapPair { unsigned short v; };   // U and V of one chroma sample, at any byte address

// the map of the chroma plane: the luma map conjugated by the siting, every operation rounded on its own
template <bool PERSP>
__device__ __forceinline__ void nv12_chroma_map(const double *__restrict__ m, double sx, double sy, double (&mc)[9])
{
    const double c2 = (m[0] * sx + m[1] * sy) + m[2];
    const double c5 = (m[3] * sx + m[4] * sy) + m[5];
    if constexpr (PERSP) {
        const double c8 = (m[6] * sx + m[7] * sy) + m[8];
        mc[0] = m[0] - sx * m[6]; mc[1] = m[1] - sx * m[7]; mc[2] = 0.5 * (c2 - sx * c8);
        mc[3] = m[3] - sy * m[6]; mc[4] = m[4] - sy * m[7]; mc[5] = 0.5 * (c5 - sy * c8);
        mc[6] = 2.0 * m[6]; mc[7] = 2.0 * m[7]; mc[8] = c8;
    } else {
        mc[0] = m[0]; mc[1] = m[1]; mc[2] = 0.5 * (c2 - sx);
        mc[3] = m[3]; mc[4] = m[4]; mc[5] = 0.5 * (c5 - sy);
        mc[6] = 0.0; mc[7] = 0.0; mc[8] = 1.0;
    }
}

// ---- luma: warp_frames<unsigned char, VEC, PERSP> on the Y planes, which lie H W 3 / 2 bytes apart ----
// The body repeats warp_frames' around the shared warp_row / warp_source / warp_pack instead of calling a strided warp_frames:
// through one, the compiler turned the taps' clamps from branches into v_min_f64 / v_max_f64.
template <bool PERSP, bool VEC>
__device__ __forceinline__ void nv12_luma(const WarpNv12Args &a)
{
    constexpr int NC = PERSP ? 9 : 6;
    const int x0 = ((int)blockIdx.y * 64 + (int)(threadIdx.x & 63)) * kWarpPx;
    const int y = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (x0 >= a.W || y >= a.H) return;
    const size_t plane = (size_t)a.H * (size_t)a.W, fb = plane + plane / 2;
    const unsigned row = (unsigned)y * (unsigned)a.W + (unsigned)x0;
    const double fy = (double)y, Wm1 = (double)(a.W - 1), Hm1 = (double)(a.H - 1);
    for (int f = blockIdx.z; f < a.F; f += gridDim.z) {
        const double *__restrict__ m = a.map + NC * (size_t)f;
        const WarpRow<PERSP> r = warp_row<PERSP>(m, fy);
        const unsigned char *__restrict__ img = a.in + (size_t)f * fb;
        unsigned char v[kWarpPx], in[kWarpPx];
#pragma unroll
        for (int k = 0; k < kWarpPx; k++) {   // a pixel past the row's end is computed (its taps are clamped) and not stored
            const double fx = (double)(x0 + k);
            const WarpSource p = warp_source(r, fx, Wm1, Hm1);
            const BilinearTaps t = bilinear_taps(a.H, a.W, p.ys, p.xs);
            const float s = bilinear_finish(t, ld_pix<unsigned char>(img, (unsigned)t.i00), ld_pix<unsigned char>(img, (unsigned)t.i01),
                                            ld_pix<unsigned char>(img, (unsigned)t.i10), ld_pix<unsigned char>(img, (unsigned)t.i11));
            v[k] = warp_store_value(p.ok ? s : 0.0f, (unsigned char)0);
            in[k] = p.ok ? 1 : 0;
        }
        unsigned char *__restrict__ dst = a.out + (size_t)f * fb + row;
        if constexpr (VEC) {
            *reinterpret_cast<unsigned *>(dst) = warp_pack(v);
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

// ---- chroma: the H/2 x W/2 plane of (U, V) pairs under mc, 4 rows of 64 lanes a block, kWarpPx pairs a lane ----
template <bool PERSP, bool VEC>
__device__ __forceinline__ void nv12_chroma(const WarpNv12Args &a)
{
    constexpr int NC = PERSP ? 9 : 6;
    const int CH = a.H / 2, CW = a.W / 2;
    const unsigned cb = (blockIdx.x - a.luma_groups) * gridDim.y + blockIdx.y;
    const int x0 = ((int)(cb % a.chroma_cols) * 64 + (int)(threadIdx.x & 63)) * kWarpPx;
    const int y = (int)(cb / a.chroma_cols) * 4 + (int)(threadIdx.x >> 6);
    if (x0 >= CW || y >= CH) return;
    const size_t plane = (size_t)a.H * (size_t)a.W, fb = plane + plane / 2;
    const unsigned row = (unsigned)plane + 2u * ((unsigned)y * (unsigned)CW + (unsigned)x0);   // byte offset in the frame
    const double fy = (double)y, Wm1 = (double)(CW - 1), Hm1 = (double)(CH - 1);
    for (int f = blockIdx.z; f < a.F; f += gridDim.z) {
        double mc[9];
        nv12_chroma_map<PERSP>(a.map + NC * (size_t)f, a.sx, a.sy, mc);
        const WarpRow<PERSP> r = warp_row<PERSP>(mc, fy);
        const unsigned char *__restrict__ uv = a.in + (size_t)f * fb + plane;
        unsigned v[kWarpPx];   // U in bits 0-7, V in bits 8-15
#pragma unroll
        for (int k = 0; k < kWarpPx; k++) {   // a pair past the row's end is computed (its taps are clamped) and not stored
            const double fx = (double)(x0 + k);
            const WarpSource p = warp_source(r, fx, Wm1, Hm1);
            const BilinearTaps t = bilinear_taps(CH, CW, p.ys, p.xs);
            const unsigned p00 = reinterpret_cast<const TapPair *>(uv + 2u * (unsigned)t.i00)->v;
            const unsigned p01 = reinterpret_cast<const TapPair *>(uv + 2u * (unsigned)t.i01)->v;
            const unsigned p10 = reinterpret_cast<const TapPair *>(uv + 2u * (unsigned)t.i10)->v;
            const unsigned p11 = reinterpret_cast<const TapPair *>(uv + 2u * (unsigned)t.i11)->v;
            const float su = bilinear_finish(t, (float)(p00 & 0xffu), (float)(p01 & 0xffu), (float)(p10 & 0xffu), (float)(p11 & 0xffu));
            const float sv = bilinear_finish(t, (float)(p00 >> 8), (float)(p01 >> 8), (float)(p10 >> 8), (float)(p11 >> 8));
            // outside: U = V = 128, no colour
            const unsigned bu = warp_store_value(p.ok ? su : 128.0f, (unsigned char)0), bv = warp_store_value(p.ok ? sv : 128.0f, (unsigned char)0);
            v[k] = bu | (bv << 8);
        }
        unsigned char *__restrict__ dst = a.out + (size_t)f * fb + row;
        if constexpr (VEC) {
            *reinterpret_cast<uint2 *>(dst) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
        } else {
#pragma unroll
            for (int k = 0; k < kWarpPx; k++)
                if (x0 + k < CW) {
                    dst[2 * k] = (unsigned char)v[k];
                    dst[2 * k + 1] = (unsigned char)(v[k] >> 8);
                }
        }
    }
}

// ---- grid (ceil(H / 4) + ceil(ceil(H / 8) chroma_cols / gy), gy = ceil(W / (64 kWarpPx)), min(F, 65535)), block 256 ----
template <bool PERSP, int VEC>
__global__ __launch_bounds__(256) void k_warp_nv12(const WarpNv12Args a)
{
    if (blockIdx.x < a.luma_groups)
        nv12_luma<PERSP, (VEC >= 1)>(a);
    else
        nv12_chroma<PERSP, (VEC >= 2)>(a);
}

}  // namespace oflk
