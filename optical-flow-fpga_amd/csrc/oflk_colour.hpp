// oflk_colour.hpp -- gfx950 device code of colour video (oflk_luma_u8, oflk_warp_affine_packed, oflk_warp_perspective_packed,
// the packed sequence call and the packed online stabiliser made of them): frames are interleaved bytes [F][H][W][C], C = 3
// or 4, and every result is tied byte for byte to what the planar entry points return per channel.
//
// The statement is tests/colour_model.py (include/oflk.h repeats it).
//
//   k_luma<C, VEC>      Y = (77 R + 150 G + 29 B + 128) >> 8 in integers, a streaming kernel over the F H W pixels.  VEC: a lane
//                       owns 4 consecutive pixels, reads their 4 C bytes as three dwords (C = 3) or one dwordx4 (C = 4) and
//                       stores one dword of luma; every other shape and alignment runs the element-wise instantiation
//   k_warp_packed<C, PERSP, VEC>  warp_frames' grid and lane shape, and its source position and closed-interval test through
//                       the same warp_row / warp_source (oflk_stabilize.hpp), once per pixel; the four taps are gathered
//                       as one dword each, which holds all C channels of the tap, and bilinear_finish runs C times on the one set of weights, so
//                       every channel's byte is the planar kernel's.  VEC stores a lane's 4 pixels as three dwords (C = 3) or
//                       one dwordx4 (C = 4) and the inside dword; the other instantiation stores byte by byte.  The two
//                       are two kernels for k_warp_affine's reason.
//
// The taps of C = 3: pixel i is the 3 bytes at 3 i, at any alignment.  gfx950's global loads take any byte address, so one
// global_load_dword at 3 i brings the pixel and the first byte of pixel i + 1; three global_load_ubyte would be three
// gathers a tap, twelve a pixel.  The last pixel of a frame has no pixel behind it inside the frame (and the last frame's
// none inside the allocation), so its dword is read one byte earlier, at 3 i - 1, and shifted down by 8 bits: no load touches
// a byte outside [H][W][C] of its own frame.  H, W >= 2 makes 3 i - 1 >= 8 there.
#pragma once
#include "oflk_stabilize.hpp"

#pragma clang fp contract(off)

namespace oflk {

constexpr int kLumaPx = 4;       // consecutive pixels of a lane of k_luma<C, true>
constexpr int kLumaBlock = 256;

struct LumaArgs {
    const unsigned char *in;   // [n][C]
    unsigned char *out;        // [n]
    size_t n;                  // F H W
    int bgr;                   // OFLK_ORDER_BGR: the bytes 0 and 2 change places
};

// the three low bytes of p (byte 0 at the lowest address) weighted; bgr swaps what bytes 0 and 2 weigh
__device__ __forceinline__ unsigned luma_of(unsigned p, int bgr)
{
    const unsigned b0 = p & 0xffu, b1 = (p >> 8) & 0xffu, b2 = (p >> 16) & 0xffu;
    const unsigned r = bgr ? b2 : b0, b = bgr ? b0 : b2;
    return (77u * r + 150u * b1 + 29u * b + 128u) >> 8;
}

// ---- luma: grid (min(ceil(work / 256), 65535 * 16)), block 256; work = n / 4 (VEC) or n ----
template <int C, bool VEC>
__global__ __launch_bounds__(kLumaBlock) void k_luma(const LumaArgs a)
{
    const size_t stride = (size_t)gridDim.x * kLumaBlock;
    size_t i = (size_t)blockIdx.x * kLumaBlock + threadIdx.x;
    if constexpr (VEC) {
        const size_t groups = a.n / kLumaPx;   // n % 4 == 0
        for (; i < groups; i += stride) {
            unsigned p[kLumaPx];
            if constexpr (C == 4) {
                const uint4 q = *reinterpret_cast<const uint4 *>(a.in + 16 * i);
                p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
            } else {
                const unsigned *__restrict__ src = reinterpret_cast<const unsigned *>(a.in + 12 * i);
                const unsigned d0 = src[0], d1 = src[1], d2 = src[2];
                p[0] = d0;
                p[1] = (d0 >> 24) | (d1 << 8);
                p[2] = (d1 >> 16) | (d2 << 16);
                p[3] = d2 >> 8;
            }
            *reinterpret_cast<unsigned *>(a.out + 4 * i) =
                luma_of(p[0], a.bgr) | (luma_of(p[1], a.bgr) << 8) | (luma_of(p[2], a.bgr) << 16) | (luma_of(p[3], a.bgr) << 24);
        }
    } else {
        for (; i < a.n; i += stride) {
            const unsigned char *__restrict__ q = a.in + (size_t)C * i;
            a.out[i] = (unsigned char)luma_of((unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16), a.bgr);
        }
    }
}

// ---- the packed warp: warp_frames' grid (ceil(H / 4), ceil(W / (64 kWarpPx)), min(F, 65535)), block 256 ----
struct WarpPackedArgs {
    const unsigned char *in;   // [F][H][W][C]
    const double *map;         // [F][6]; PERSP: [F][9]
    unsigned char *out;        // [F][H][W][C]
    unsigned char *inside;     // [F][H][W] or NULL
    int F, H, W;
};

struct __attribute__((packed)) TapDword { unsigned v; };   // a dword at any byte address

// the C bytes of pixel `pix` of a frame (pix <= last = H W - 1) in the low bytes of a dword; H W C < 2^31 (checked on the host)
template <int C>
__device__ __forceinline__ unsigned ld_tap(const unsigned char *__restrict__ img, unsigned pix, unsigned last)
{
    if constexpr (C == 4) {
        return reinterpret_cast<const TapDword *>(img + 4u * pix)->v;
    } else {
        const unsigned back = pix == last ? 1u : 0u;   // the frame's last pixel: the dword that ends with it
        return reinterpret_cast<const TapDword *>(img + (3u * pix - back))->v >> (8u * back);
    }
}

template <int C, bool PERSP, bool VEC>
__global__ __launch_bounds__(256) void k_warp_packed(const WarpPackedArgs a)
{
    constexpr int NC = PERSP ? 9 : 6;
    const int x0 = ((int)blockIdx.y * 64 + (int)(threadIdx.x & 63)) * kWarpPx;
    const int y = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (x0 >= a.W || y >= a.H) return;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const unsigned last = (unsigned)plane - 1u;
    const size_t row = (size_t)y * (size_t)a.W + (size_t)x0;
    const double fy = (double)y, Wm1 = (double)(a.W - 1), Hm1 = (double)(a.H - 1);
    for (int f = blockIdx.z; f < a.F; f += gridDim.z) {
        const double *__restrict__ m = a.map + NC * (size_t)f;
        const WarpRow<PERSP> r = warp_row<PERSP>(m, fy);
        const unsigned char *__restrict__ img = a.in + (size_t)f * plane * C;
        unsigned v[kWarpPx];            // a pixel's C bytes, channel c at bits 8 c
        unsigned char in[kWarpPx];
#pragma unroll
        for (int k = 0; k < kWarpPx; k++) {   // a pixel past the row's end is computed (its taps are clamped) and not stored
            const double fx = (double)(x0 + k);
            const WarpSource p = warp_source(r, fx, Wm1, Hm1);
            const BilinearTaps t = bilinear_taps(a.H, a.W, p.ys, p.xs);
            const unsigned p00 = ld_tap<C>(img, (unsigned)t.i00, last), p01 = ld_tap<C>(img, (unsigned)t.i01, last);
            const unsigned p10 = ld_tap<C>(img, (unsigned)t.i10, last), p11 = ld_tap<C>(img, (unsigned)t.i11, last);
            unsigned px = 0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float s = bilinear_finish(t, (float)((p00 >> (8 * c)) & 0xffu), (float)((p01 >> (8 * c)) & 0xffu),
                                                (float)((p10 >> (8 * c)) & 0xffu), (float)((p11 >> (8 * c)) & 0xffu));
                px |= (unsigned)warp_store_value(p.ok ? s : 0.0f, (unsigned char)0) << (8 * c);
            }
            v[k] = px;
            in[k] = p.ok ? 1 : 0;
        }
        unsigned char *__restrict__ dst = a.out + ((size_t)f * plane + row) * C;
        if constexpr (VEC) {
            if constexpr (C == 4) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
                unsigned *__restrict__ d = reinterpret_cast<unsigned *>(dst);
                d[0] = v[0] | (v[1] << 24);
                d[1] = (v[1] >> 8) | (v[2] << 16);
                d[2] = (v[2] >> 16) | (v[3] << 8);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kWarpPx; k++)
                if (x0 + k < a.W) {
#pragma unroll
                    for (int c = 0; c < C; c++) dst[C * k + c] = (unsigned char)(v[k] >> (8 * c));
                }
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

}  // namespace oflk
