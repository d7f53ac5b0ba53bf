// Median filtering of dense flow planes (oflk_flow_median, and the flow_median setting of the sequence calls): the kernel.
// Included by oflk.hip after oflk_mosaic.hpp, whose order (median_key / median_value) it uses.
#pragma once

namespace oflk {

// ---------------------------------------------------------------------------
// The statement (include/oflk.h, tests/flow_median_model.py).  A plane p is [H][W] float32 and the window SIZE x SIZE, SIZE in
// {3, 5, 7, 9}, R = SIZE / 2.  Output pixel (y, x) takes the SIZE^2 values p[clamp(y + j, 0, H-1)][clamp(x + i, 0, W-1)], i, j
// in -R .. R (the border is replicated), orders them by median_key and returns the one of rank SIZE^2 / 2.  SIZE^2 is odd, so
// the result is one of the inputs: nothing is averaged and nothing is rounded, and equal keys are equal bytes, so neither the
// selection method nor the launch geometry can show.  Every plane is filtered on its own.
//
// One block of 256 lanes is a tile of kFlowMedianTileH x kFlowMedianTileW = 8 x 32 output pixels of one plane (grid.z; the
// tiles of a plane are flattened into grid.x, so a tall or wide plane meets no grid limit).  The block stages its tile and
// the halo of R as keys, converted once per element, (8 + 2R) x (32 + 2R) dwords of LDS: 1360 / 1728 / 2128 / 2560 B for SIZE
// 3 / 5 / 7 / 9, which never limits the blocks of a CU.  The addresses are clamped before the load, so no load leaves the
// plane, and a lane beyond the plane's edge takes part in the staging and stores nothing.  A tile row is 32 consecutive
// dwords: the 32 lanes of a half wave (the conflict group of ds_read_b32) read 32 consecutive banks whatever the row stride,
// and the staging writes consecutive dwords.  An 8 x 32 tile stages 1.4 (SIZE 3) to 2.5 (SIZE 9) values per output pixel,
// nearly all of them L2 hits of the neighbouring tiles; 4 x 64, the other kernels' tile, would stage 1.5 to 3.4.
//
// The selection is forgetful selection (Perrot, Domas & Couturier 2014) for every SIZE, one template: of N = SIZE^2 keys the
// lane holds M = N / 2 + 2 (6, 14, 26, 42) in registers.  The smallest of M keys has M - 1 = N / 2 + 1 keys above or equal, so
// its rank is below N / 2, and likewise the largest lies above: neither is the median, both are forgotten, and the next key
// takes the freed place.  With every key taken in three are left, and the middle one is the median.  The extremes of k live
// keys take k/2 exchanges that order the pairs (i, k-1-i), then a chain of min over the lower half and one of max over the
// upper (an odd k's middle key belongs to both): about 3k/2 - 2 exchanges of one v_min_u32 and one v_max_u32.  The whole
// selection is 20 / 129 / 474 / 1270 exchanges a pixel for SIZE 3 / 5 / 7 / 9, twice as many VALU operations; the indices
// are compile-time constants, so the keys stay in registers and the LDS reads carry immediate offsets.  The best exchange
// networks known take 19 for 3 x 3 and 99 for 5 x 5: one method for all four sizes was preferred to a table a size.
// ---------------------------------------------------------------------------
constexpr int kFlowMedianTileW = 32;   // a block's tile: 32 lanes across ...
constexpr int kFlowMedianTileH = 8;    // ... and 8 rows (oflk_flow_median_tile)

struct FlowMedianArgs {
    const float *in;   // [P][H][W]
    float *out;        // [P][H][W], not overlapping in
    int H, W;
    int tiles_x;       // tiles across a plane
};

__device__ __forceinline__ void median_exchange(unsigned &lo, unsigned &hi)
{
    const unsigned a = lo, b = hi;
    lo = min(a, b);
    hi = max(a, b);
}

// the key of rank SIZE^2 / 2 of the window whose first key is win[0], rows STRIDE keys apart
template <int SIZE, int STRIDE>
__device__ __forceinline__ unsigned flow_median_select(const unsigned *win)
{
    constexpr int N = SIZE * SIZE, M = N / 2 + 2;
    unsigned a[M];
#pragma unroll
    for (int i = 0; i < M; i++) a[i] = win[(i / SIZE) * STRIDE + i % SIZE];
#pragma unroll
    for (int k = M; k >= 3; k--) {
#pragma unroll
        for (int i = 0; i < k / 2; i++) median_exchange(a[i], a[k - 1 - i]);
#pragma unroll
        for (int i = (k - 1) / 2; i >= 1; i--) median_exchange(a[i - 1], a[i]);   // a[0]: the smallest
#pragma unroll
        for (int i = k / 2; i < k - 1; i++) median_exchange(a[i], a[i + 1]);      // a[k-1]: the largest
        if (k > 3) {   // the next key takes the smallest one's place and the largest is dropped with k
            const int next = N - (k - 3);
            a[0] = win[(next / SIZE) * STRIDE + next % SIZE];
        }
    }
    return a[1];
}

template <int SIZE>
__global__ __launch_bounds__(256) void k_flow_median(FlowMedianArgs a)
{
    constexpr int R = SIZE / 2, LW = kFlowMedianTileW + 2 * R, LH = kFlowMedianTileH + 2 * R;
    __shared__ unsigned keys[LH * LW];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * kFlowMedianTileW;
    const int y0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * kFlowMedianTileH;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const float *__restrict__ p = a.in + (size_t)blockIdx.z * plane;
    for (int idx = tid; idx < LH * LW; idx += 256) {
        const int ly = idx / LW, lx = idx - ly * LW;
        const int gy = min(max(y0 - R + ly, 0), a.H - 1), gx = min(max(x0 - R + lx, 0), a.W - 1);
        keys[idx] = median_key(p[(size_t)gy * (size_t)a.W + (size_t)gx]);
    }
    __syncthreads();
    const int tx = tid % kFlowMedianTileW, ty = tid / kFlowMedianTileW;
    const unsigned k = flow_median_select<SIZE, LW>(keys + ty * LW + tx);
    const int x = x0 + tx, y = y0 + ty;
    if (x < a.W && y < a.H) a.out[(size_t)blockIdx.z * plane + (size_t)y * (size_t)a.W + (size_t)x] = median_value(k);
}

}  // namespace oflk
