// oflk_tracker.hpp -- gfx950 device code of the online sparse KLT tracker (oflk_tracker_*): one frame per push, the state
// on the device between pushes.
//
// The statement (include/oflk.h, tests/tracker_model.py) is the sparse-replenish one with the detection of frame t run when
// frame t is pushed.  Nothing here states arithmetic of its own: a step is sparse_step (oflk_sparse.hpp), composed exactly
// as sparse_track composes it; a detection is the seven launches of detect_launch.
//
// The tracker holds a ring of two frames and their two pyramids, [2][h_l][w_l] per level, so that the ring index of a frame
// is the frame argument sparse_step already takes: a swapped ring needs no copy of frames or pyramids, only ia and ib
// exchanged.  The two rows (xy, visible) alternate the same way.
#pragma once
#include "oflk_sparse.hpp"

#pragma clang fp contract(off)

namespace oflk {

struct PushArgs {
    const float *xy_in;             // [K][2] the previous frame's row; NULL on frame 0: every slot dead
    const unsigned char *vis_in;    // [K]
    float *xy_out;                  // [K][2] this frame's row
    unsigned char *vis_out;         // [K]
    float *residual;                // [K]
    unsigned char *born;            // [K], cleared
    int *detected;                  // [1], cleared
    int ib;                         // ring index (0 / 1) of this frame; the previous frame has the other one
};

// One push's step: grid (K), one wave per slot.  An alive slot takes the step of the pair (ring ia -> ring ib) as
// sparse_track does: forward, then backward from the rounded target, the forward-backward test (fb_finish's expressions) and
// the residual test.  residual[n]: the forward step's where the slot was alive and that step ok, NaN otherwise.  Loops are
// bounded by L * K * 2; no spin, no atomics, no communication between blocks.
template <int HW, class PIX>
__global__ __launch_bounds__(64) void k_sparse_push(SparseArgs a, PushArgs r)
{
    __shared__ SparseLds<HW> m;
    const size_t n = blockIdx.x;
    const int lane = threadIdx.x;
    const float nan = __builtin_nanf("");
    // Visibly 0 / 1, not a plain kernel argument: the compiler propagates the range of sparse_step's frame arguments over
    // all of its callers before it inlines them, and an unbounded index here costs k_sparse_track a sign extension and a
    // register at 9x9 and 11x11 -- at 11x11 its fifth wave.
    const int ib = r.ib & 1, ia = ib ^ 1;
    bool alive = r.vis_in != nullptr && r.vis_in[n] != 0;
    float x = 0.0f, y = 0.0f, res = nan;
    if (wave_uniform(alive)) {
        x = r.xy_in[2 * n];
        y = r.xy_in[2 * n + 1];
        SparseStep f{};
        float nx = 0.0f, ny = 0.0f;
        bool keep = false;
        for (int d = 0; d < 2; d++) {   // forward, then backward from the forward step's target (one copy of the step)
            const SparseStep s = sparse_step<HW, PIX>(a, m, lane, d ? ib : ia, d ? ia : ib, d ? nx : x, d ? ny : y);
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
        if (f.ok) res = f.residual;
        alive = keep;
        x = nx;
        y = ny;
    }
    if (lane == 0) {
        r.xy_out[2 * n] = alive ? x : nan;
        r.xy_out[2 * n + 1] = alive ? y : nan;
        r.vis_out[n] = alive ? 1 : 0;
        r.residual[n] = res;
        r.born[n] = 0;
        if (n == 0) *r.detected = 0;
    }
}

// The row entries of the slots that have just begun a track on frame t.  In the sequence call the next track launch starts
// them; here the row is complete when the push is.
//   free == NULL (after a detection): every slot with born[n] set takes its query (qxy[n] + 0: -0 -> +0) and is visible
//   free != NULL (oflk_tracker_add_points, after k_free_list): the i-th of n points goes to the i-th dead slot, while dead
//                slots last: position, visible, born = 1, qt = t
struct NewbornArgs {
    float2 *row;             // [K]
    unsigned char *visible;  // [K]
    unsigned char *born;     // [K]
    int *qt;                 // [K]
    const float2 *qxy;       // [K] the detection's queries, or the n points
    const int *free, *nfree;
    int n, K, t;
};

__global__ __launch_bounds__(256) void k_tracker_newborn(NewbornArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int dst = i;
    if (a.free) {
        if (i >= min(min(a.n, *a.nfree), a.K)) return;
        dst = a.free[i];
        a.born[dst] = 1;
        a.qt[dst] = a.t;
    } else if (i >= a.K || !a.born[i]) {
        return;
    }
    const float2 p = a.qxy[i];
    a.row[dst] = make_float2(p.x + 0.0f, p.y + 0.0f);
    a.visible[dst] = 1;
}

}  // namespace oflk
