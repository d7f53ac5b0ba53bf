// oflk.hip -- host side of liboflk.so: C ABI (include/oflk.h), plans, launch
// orchestration.  Device code lives in oflk_kernels.hpp.
//
// Build (see optical-flow-fpga_amd/csrc/Makefile):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared ...
//
// There is deliberately no CPU path in this library: with no usable GPU every
// compute entry point returns OFLK_ERR_NO_DEVICE.
#include "oflk_kernels.hpp"
#include "oflk_stream.hpp"
#include "oflk_sparse.hpp"
#include "oflk_tracker.hpp"
#include "oflk_motion.hpp"
#include "oflk_homography.hpp"
#include "oflk_stabilize.hpp"
#include "oflk_mosaic.hpp"
#include "oflk_flowmedian.hpp"
#include "oflk_align.hpp"
#include "oflk_colour.hpp"
#include "oflk_nv12.hpp"
#include "oflk_interp.hpp"
#include "oflk_denoise.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/oflk.h"

#define OFLK_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace oflk;

thread_local std::string t_err;
thread_local int t_resolved = 0;   // pairs the last host pyramidal call of this thread redid exactly

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    t_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(OFLK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

std::atomic<int> g_device{0};   // device of the host-pointer entry points (oflk_set_device)
std::atomic<int> g_host_arith{OFLK_ARITH_EXACT};   // arithmetic of the host-pointer entry points (oflk_set_host_arithmetic)
std::atomic<int> g_multi_workers{0};   // oflk_multi_rehearsal: queue workers of the *_multi entry points (0 = one per device)

int ensure_device(int dev)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(OFLK_ERR_NO_DEVICE,
                    "no usable HIP device (hipGetDeviceCount: %s, count %d); liboflk has no CPU path",
                    hipGetErrorString(e), n);
    }
    if (dev < 0 || dev >= n) return fail(OFLK_ERR_INVALID, "device %d out of range [0,%d)", dev, n);
    HIP_TRY(hipSetDevice(dev));
    return OFLK_OK;
}

// scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, int(4*sigma+0.5)).  For the
// reference's sigma (2.0 = 1/scale_factor, lucas_kanade_pyramidal.py:46) the
// table is SciPy's own output (NumPy's exp differs from libm's in the last ulp
// for some taps); other sigmas use libm and NumPy's pairwise normalisation order.
const double kSigma2[9] = {0x1.98862a07ae7b4p-3,  0x1.68856f9ab1982p-3,  0x1.ef9093fc46e5ap-4,
                           0x1.0941b71ceef37p-4,  0x1.ba4d4125ffd2ap-6,  0x1.1f30504e20207p-7,
                           0x1.227362b5fc92dp-9,  0x1.c98b8c5d0dda5p-12, 0x1.18aad19e4159bp-14};

double np_pairwise_f64(const double *a, size_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; i++) r += a[i];
        return r;
    } else if (n <= 128) {
        double r[8];
        size_t i;
        for (int j = 0; j < 8; j++) r[j] = a[j];
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_f64(a, n2) + np_pairwise_f64(a + n2, n - n2);
}

// The kernels form row offsets with __mul24, the SIGNED 24-bit multiply (v_mad_i32_i24: both operands sign-extended from
// bit 23): a row index or a width of 2^23 or more would read as negative.  Every entry check refuses such frames.
constexpr int kMaxDim = 1 << 23;

int make_gauss(double sigma, GaussW *g)
{
    if (!(sigma > 0.0)) return fail(OFLK_ERR_INVALID, "sigma must be positive");
    int radius = (int)(4.0 * sigma + 0.5);
    if (radius > kMaxRadius)
        return fail(OFLK_ERR_UNSUPPORTED, "gaussian radius %d > %d (scale_factor too small)", radius,
                    kMaxRadius);
    g->radius = radius;
    if (sigma == 2.0) {
        for (int k = 0; k <= 8; k++) g->w[k] = kSigma2[k];
        return OFLK_OK;
    }
    double phi[2 * kMaxRadius + 1];
    double c = -0.5 / (sigma * sigma);
    for (int i = -radius; i <= radius; i++) phi[i + radius] = std::exp(c * (double)(i * i));
    double s = 0.0 + np_pairwise_f64(phi, (size_t)(2 * radius + 1));
    for (int k = 0; k <= radius; k++) g->w[k] = phi[radius + k] / s;
    return OFLK_OK;
}

Linspace make_linspace(int S, int T)
{
    Linspace l;
    l.T = T;
    l.last = (double)(S - 1);
    l.step = T > 1 ? (double)(S - 1) / (double)(T - 1) : 0.0;
    return l;
}

int level_dims(int H, int W, int levels, double scale, int *dims)
{
    if (H < 1 || W < 1) return fail(OFLK_ERR_INVALID, "H and W must be >= 1 (got %d x %d)", H, W);
    if (levels < 1 || levels > OFLK_MAX_LEVELS)
        return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    if (!(scale > 0.0 && scale <= 1.0))
        return fail(OFLK_ERR_INVALID, "scale_factor must be in (0,1] (got %g)", scale);
    int h = H, w = W;
    for (int l = levels - 1; l >= 0; l--) {
        if (h < 1 || w < 1)
            return fail(OFLK_ERR_INVALID, "pyramid level %d of %dx%d would be empty", l, W, H);
        dims[2 * l] = h;
        dims[2 * l + 1] = w;
        h = (int)((double)h * scale);  // int(height * scale_factor), lucas_kanade_pyramidal.py:51
        w = (int)((double)w * scale);
    }
    return OFLK_OK;
}

// windows with a tiled kernel (3x3 ... 11x11); every other admissible size runs the generic one-thread-per-pixel kernel
inline bool tiled_window(int hw) { return hw >= 1 && hw <= 5; }

// The envelope of OFLK_ARITH_TOLERANT (include/oflk.h): the (levels, iterations) cells of the 5x5 window where its relaxations
// were measured to keep the worst mean EPE of the 13 verification patterns at or under a third of the 1e-4 px bar, with the
// reference's iteration counts (tests/test_tolerant_model.py sweeps L 1..4 x K 1..5).  Every other cell runs exactly.
// oracle/oflk_tolerant_model.py (tolerant_spec) states the same set.
inline bool tolerant_relaxes(int levels, int hw, int iterations)
{
    if (hw != 2) return false;
    return (levels == 1 && (iterations == 1 || iterations == 2)) || (levels == 3 && (iterations == 2 || iterations == 3));
}

int window_hw(int window_size, int *hw)
{
    if (window_size < 1) return fail(OFLK_ERR_INVALID, "window_size must be >= 1");
    int h = window_size / 2;  // even sizes round down, lucas_kanade_core.py:104
    if (window_size > OFLK_MAX_WINDOW || pairwise_depth((2 * h + 1) * (2 * h + 1)) > kGenericDepth)
        return fail(OFLK_ERR_UNSUPPORTED, "window_size %d not built (windows of up to %d x %d)", window_size, OFLK_MAX_WINDOW,
                    OFLK_MAX_WINDOW);
    *hw = h;
    return OFLK_OK;
}

// ---- kernel classes for the per-kernel event timing --------------------------
enum KClass { KC_LK_SINGLE = 0, KC_LK_ITER, KC_LK_ITER_FINEST, KC_BLUR, KC_RESAMPLE,
              KC_UPSAMPLE, KC_EXPORT, KC_INIT, KC_PYR_FUSED, KC_LK_REDO, KC_COUNT };
const char *kClassNames[KC_COUNT] = {"lk_single", "lk_iter", "lk_iter_finest", "blur",
                                     "pyr_resample", "flow_upsample", "export_fixup", "call_init",
                                     "pyr_down_fused", "lk_single_redo"};

}  // namespace

struct oflk_plan {
    int device = 0;
    int B = 0, H = 0, W = 0, L = 0, win = 0, hw = 0, K = 0;
    int dims[2 * OFLK_MAX_LEVELS] = {0};
    size_t ws_bytes = 0;
    // workspace
    float *pyr[OFLK_MAX_LEVELS] = {nullptr};      // l < L-1: [2B][h][w] (prev then curr); a sequence uses [B+1][h][w]
    // blur temporaries [tmp_imgs][H][W] of the unfused pyramid chain, allocated on first need (ensure_tmp): 2B images by
    // the first dense pyramidal pass; a sparse pass only where a level does not fit the fused kernel, and then B+1
    float *tmpA = nullptr, *tmpB = nullptr;
    size_t tmp_imgs = 0;
    // per level one block: [slot 0..1][B][h][w] of interleaved float2 {u, v} (see LkArgs); allocated by the first dense
    // pyramidal pass (ensure_dense_ws): a plan that only serves sparse calls never holds a flow field
    float *flow[OFLK_MAX_LEVELS] = {nullptr};
    // per-call state, one allocation, zeroed by k_call_init at the start of every call:
    //   acc[B][L][K][kAccShards][kAccStride] (u64) | iters_run[B][L] (i32) | uncertain[B][L] (i32) | log[B][L][K][2] (f32)
    unsigned long long *state = nullptr;
    // the backward pass's state block (same layout), allocated on the first bidirectional call; the backward pass swaps it
    // with `state` while it runs (StateSwap), so every accessor below serves both
    unsigned long long *state_b = nullptr;
    bool last_fb = false;   // the last pyramidal pass was bidirectional: the level flows are the backward pass's
    // uint8 plans only, and only when the fused pyramid kernel cannot take the frames (it always can for
    // scale 0.5 unless a level is tiny): float32 copies of the caller's frames, allocated on first need --
    // [B+1][H][W] (prev, or a sequence's B+1 frames) and [B][H][W] (curr)
    float *u8_stage[2] = {nullptr, nullptr};
    // scratch of oflk_plan_resolve_uncertain (one pair, unfused, planar), allocated on first use
    struct Exact {
        float *pyr[OFLK_MAX_LEVELS] = {nullptr};   // l < L-1: [2][h][w]
        float *u[OFLK_MAX_LEVELS] = {nullptr}, *v[OFLK_MAX_LEVELS] = {nullptr};
        float *warped = nullptr, *du = nullptr, *dv = nullptr, *f32[2] = {nullptr, nullptr}, *pieces = nullptr;
        bool ready = false;
    } exact;
    GaussW gauss;
    int arith = OFLK_ARITH_EXACT;   // oflk_plan_set_arithmetic
    int kernels = OFLK_KERNELS_AUTO;   // oflk_plan_set_kernels
    // single-scale 5x5 on integer-valued frames: the streaming kernel's list of doubtful tiles (LkArgs::redo)
    unsigned *redo = nullptr;
    // profiling
    bool prof = false;
    int prof_only = -1;  // >= 0: bracket only launches of this kernel class
    struct Ev { hipEvent_t a, b; int cls; };
    std::vector<Ev> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double acc_ms[KC_COUNT] = {0};
    long acc_n[KC_COUNT] = {0};

    size_t npix(int l) const { return (size_t)dims[2 * l] * (size_t)dims[2 * l + 1]; }
    float2 *fl(int l, int slot) const { return reinterpret_cast<float2 *>(flow[l]) + (size_t)slot * B * npix(l); }
    int Kc() const { return std::max(K, 1); }
    size_t n_acc() const { return (size_t)B * L * Kc() * kAccShards * kAccStride; }
    unsigned long long *acc() const { return state; }
    int *iters_run() const { return reinterpret_cast<int *>(state + n_acc()); }
    int *uncertain() const { return iters_run() + (size_t)B * L; }
    float *log() const { return reinterpret_cast<float *>(uncertain() + (size_t)B * L); }
    size_t n_log() const { return (size_t)B * L * Kc() * 2; }
    // 32-bit words of the whole state block (rounded up to a multiple of 4)
    size_t state_words() const { return ((2 * n_acc() + 2 * (size_t)B * L + n_log()) + 3) & ~(size_t)3; }
};

namespace {

// the backward pass's state block in place of the forward one for the lifetime of this object (on = false: no swap)
struct StateSwap {
    oflk_plan *p;
    bool on;
    StateSwap(oflk_plan *p_, bool on_) : p(p_), on(on_ && p_->state_b)
    {
        if (on) std::swap(p->state, p->state_b);
    }
    ~StateSwap()
    {
        if (on) std::swap(p->state, p->state_b);
    }
};

// fused multiply-adds in the Gaussian pyramid: OFLK_ARITH_CONTRACTED, and OFLK_ARITH_TOLERANT inside its envelope
inline bool contracted_pyramid(const oflk_plan *p)
{
    return p && (p->arith == OFLK_ARITH_CONTRACTED || (p->arith == OFLK_ARITH_TOLERANT && tolerant_relaxes(p->L, p->hw, p->K)));
}

struct Prof {
    oflk_plan *p;
    hipStream_t s;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    Prof(oflk_plan *p_, hipStream_t s_, int cls_) : p(p_), s(s_), cls(cls_)
    {
        if (!p || !p->prof) return;
        if (p->prof_only >= 0 && cls != p->prof_only) return;
        if (p->pool.empty()) {
            if (hipEventCreate(&a) != hipSuccess) { a = nullptr; return; }   // this launch goes untimed
            if (hipEventCreate(&b) != hipSuccess) {
                (void)hipEventDestroy(a);
                a = b = nullptr;
                return;
            }
        } else {
            a = p->pool.back().first;
            b = p->pool.back().second;
            p->pool.pop_back();
        }
        if (hipEventRecord(a, s) != hipSuccess) drop();
    }
    void drop()
    {
        (void)hipGetLastError();
        p->pool.push_back({a, b});
        a = b = nullptr;
    }
    ~Prof()
    {
        if (!a) return;
        if (hipEventRecord(b, s) != hipSuccess) {
            drop();
            return;
        }
        p->pending.push_back({a, b, cls});
    }
};

// smallest |d| total (fixed point) whose mean reads >= float32(0.01) for a level of `count`
// pixels: lk_mean_of is non-decreasing in the total, so "mean < 0.01" <=> total < threshold
unsigned long long conv_threshold(double count)
{
    unsigned long long lo = 0, hi = 1ull << 62;   // mean(lo) < 0.01 <= mean(hi)
    while (hi - lo > 1) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (lk_mean_of(mid, count) < 0.01f) lo = mid;
        else hi = mid;
    }
    return hi;
}

// ---- dispatch: a runtime fact lifted to a compile-time one and handed to a generic lambda.  Every templated kernel is
// launched through these; a launch site nests them and names the kernel once, e.g.
//   with_bool(vec, [&](auto VEC) { hipLaunchKernelGGL((k<decltype(VEC)::value>), grid, block, 0, s, a); });
// A site instantiates exactly the combinations its lambdas are called with: where a product of the runtime facts would
// hold a kernel that is not built, the site narrows it with `if constexpr`.
template <class T> struct Pix { using type = T; };   // the frames' element type, as a tag
template <int V> constexpr std::integral_constant<int, V> int_c{};

template <class F>
void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

template <class F>
void with_pix(bool u8, F &&f)
{
    if (u8) f(Pix<unsigned char>{});
    else f(Pix<float>{});
}

// f(int_c<v>) for the one of Vs that v equals; false, and no call, when it is none of them
template <int... Vs, class F>
bool with_int(int v, F &&f)
{
    return ((v == Vs ? (f(int_c<Vs>), true) : false) || ...);
}

// the half windows with tiled kernels (tiled_window)
template <class F>
bool with_half_window(int hw, F &&f) { return with_int<1, 2, 3, 4, 5>(hw, f); }

// is q a multiple of m bytes (m a power of two)?  The vector instantiations of the kernels want their planes aligned.
inline bool aligned(const void *q, unsigned m) { return (reinterpret_cast<uintptr_t>(q) & (m - 1)) == 0; }

// Segments of a launch that gives one wave a strip of columns times a segment of rows (k_lks, k_lk16d): `seg_rows` rows each
// when the launch has rounds of the chip's `slots` wave slots to spare (a segment pays extra rows of loads), sized so that
// the launch is a whole number of rounds; shorter ones, of at least 40 rows, when it would otherwise leave slots of its one
// round empty.  thin_rows > 0: a launch that cannot fill half the slots even so trades rows per segment, down to
// thin_rows, for parallel waves.  Never under 8 rows.
struct Segments { int segs, rows; };
Segments wave_segments(int H, long strips, long slots, int seg_rows, int thin_rows)
{
    long segs = ((long)H + seg_rows - 1) / seg_rows;
    const double rounds = (double)(strips * segs) / (double)slots;
    if (rounds > 0.75) segs = std::max<long>(1, (long)std::ceil(rounds - 0.25) * slots / strips);
    else segs = std::max(segs, std::min(slots / std::max<long>(strips, 1), std::max<long>(1, H / 40)));   // fill the one round, >= 40 rows each
    if (thin_rows > 0 && strips * segs < slots / 2)
        segs = std::max(segs, std::min(slots / 2 / std::max<long>(strips, 1), std::max<long>(1, H / thin_rows)));
    segs = std::min<long>(segs, std::max<long>(1, H / 8));
    const int rows = (int)(((long)H + segs - 1) / segs);
    return {(H + rows - 1) / rows, rows};
}

// resident blocks of the redo pass after the streaming single-scale kernel: one per CU -- an empty list (the common case)
// then costs 7 us instead of the 22 us of a full round of 1024 blocks, a long one is walked four times slower
constexpr long kRedoBlocks = 256;

// u8: a.prev / a.curr point at uint8 frames (finest level of a uint8 plan); never with MODE_GRADS
template <int MODE>
int launch_lk(oflk_plan *plan, hipStream_t s, int cls, int hw, const LkArgs &a_in, int B, bool u8 = false)
{
    LkArgs a = a_in;
    a.B = B;
    Prof pr(plan, s, cls);
    // 1-D grid.  Large launches chain vertically adjacent tiles in one block (they share 2R
    // staging rows, the expensive part of stage 1): tile rows are cut into segments of `cap`
    // rows, then ever shorter ones (each at most half of what is left), and every XCD runs its segments longest first so that the
    // drain of the grid is made of single tiles.  Small launches keep one tile per block.
    const int tiles_x = (a.W + k5TX - 1) / k5TX, tiles_y = (a.H + k5TY - 1) / k5TY;
    if (a.W <= 2 * hw || a.H <= 2 * hw) {
        // nothing has a full window: all-zero d (and k_lkw may assume H, W > 2*hw)
        const unsigned nb = (unsigned)(((size_t)a.H * (size_t)a.W + 255) / 256);
        hipLaunchKernelGGL((k_lk_degenerate<MODE>), dim3(nb, (unsigned)B), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        return OFLK_OK;
    }
    if (!tiled_window(hw)) {
        // 1x1, 13x13 and larger windows: one thread per output pixel, np.sum's pairwise order for any length
        if constexpr (MODE == MODE_ITER) {
            return fail(OFLK_ERR_UNSUPPORTED, "the fused iteration has no kernel for half window %d", hw);   // (plans of such windows run unfused)
        } else {
            const dim3 grid((a.W + 63) / 64, (a.H + 3) / 4, (unsigned)B);
            const auto generic = [&](auto PIX) {
                hipLaunchKernelGGL((k_lk_generic<MODE, typename decltype(PIX)::type>), grid, dim3(256), 0, s, a, hw);
            };
            if constexpr (MODE == MODE_SINGLE) with_pix(u8, generic);
            else generic(Pix<float>{});
            HIP_TRY(hipGetLastError());
            return OFLK_OK;
        }
    }
    constexpr int cap_env = 8;   // tiles per chained block at most (12 / 16 were measured: no change)
    const long resident = 1024;  // 256 CUs x 4 blocks
    const long per_slot = (long)B * tiles_x * tiles_y / resident;
    int cap = MODE == MODE_GRADS ? 1 : (int)std::min<long>(std::max(1, cap_env), per_slot / 5);
    cap = std::max(cap, (tiles_y + kMaxSegs / 2 - 1) / (kMaxSegs / 2));  // keep the table short
    // seg_row holds tile rows as unsigned short
    if (MODE == MODE_GRADS || hw > 2 || cap_env <= 1 || per_slot < 10 || tiles_y > 65535) cap = 1;   // kLkChain
    unsigned nblocks;
    if (MODE == MODE_SINGLE && a.redo_pass) {
        // redo pass of the streaming kernel: resident blocks that walk the device-side list of flagged tiles
        a.nseg = 0;
        nblocks = (unsigned)std::min<long>((long)B * tiles_x * tiles_y, kRedoBlocks);
    } else if (cap <= 1) {
        a.nseg = 0;
        nblocks = (unsigned)(tiles_x * tiles_y * B);
    } else {
        int row = 0, n = 0;
        while (row < tiles_y) {
            const int rest = tiles_y - row;
            int len = std::min(cap, std::max(1, rest / 2));   // halving tail: 8,8,8,8,6,3,2,1,1 for 45 rows
            if (n == kMaxSegs - 1) len = rest;  // the halving tail of a very tall frame can get here: last segment takes the rest
            a.seg_row[n++] = (unsigned short)row;
            row += len;
        }
        a.seg_row[n] = (unsigned short)tiles_y;
        a.nseg = n;
        const int strips = B * tiles_x;
        nblocks = 8u * (unsigned)((strips + 7) / 8) * (unsigned)n;
    }
    dim3 grid(nblocks);
    // the VEC instantiation moves 16 / 8 bytes per lane: every plane must start 16-byte aligned
    // (each row then does, W % 4 == 0); anything else takes the element-wise instantiation
    const bool frames_ok = u8 ? (aligned(a.prev, 4) && aligned(a.curr, 4)) : (aligned(a.prev, 16) && aligned(a.curr, 16));   // uint8: 4 pixels per dword
    const bool vec = (a.W & 3) == 0 && frames_ok && aligned(a.aux, 16) && aligned(a.fl[0], 16) && aligned(a.fl[1], 16) &&
                     aligned(a.ou, 16) && aligned(a.ov, 16);
    // REDOL: the instantiation that walks the redo list
    const auto tile = [&](auto HW, auto REDOL) {
        const auto typed = [&](auto PIX) {
            with_bool(vec, [&](auto VEC) {
                hipLaunchKernelGGL((k_lkw<decltype(HW)::value, MODE, decltype(VEC)::value, typename decltype(PIX)::type, decltype(REDOL)::value>),
                                   grid, dim3(256), 0, s, a);
            });
        };
        if constexpr (MODE == MODE_GRADS) typed(Pix<float>{});   // gradients are float planes
        else with_pix(u8, typed);
    };
    if constexpr (MODE == MODE_SINGLE) {
        if (a.redo_pass && hw == 3) {   // only the 7x7 kernel has the list-walking instantiation
            tile(int_c<3>, std::true_type{});
            HIP_TRY(hipGetLastError());
            return OFLK_OK;
        }
    }
    if (!with_half_window(hw, [&](auto HW) { tile(HW, std::false_type{}); })) return fail(OFLK_ERR_UNSUPPORTED, "half window %d not built", hw);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// k_lks (oflk_stream.hpp): the streaming form of the 5x5 kernel (single-scale: 7x7 too), for passes whose window sums need
// not be in NumPy's order (the tolerant mode's fine levels; single-scale on integer-valued frames, where any order is
// exact).  One wave per (strip of 120 output columns, segment of Hs rows); wave_segments sizes the segments, ~128 rows each
// when there are rounds to spare (a segment pays 2 (hw + 1) extra rows).
constexpr int kLksSegRows = 128;
template <int MODE>
int launch_lks(oflk_plan *plan, hipStream_t s, int cls, const LkArgs &a_in, int B, bool u8, int warp, int hw = 2)
{
    LkArgs a = a_in;
    a.B = B;
    Prof pr(plan, s, cls);
    const long strips = ((long)a.W + kLksOutW - 1) / kLksOutW * B;
    const long slots = 256 * 4 * (MODE == MODE_SINGLE ? 4 : kLksWaves);   // wave slots of the chip at the kernel's occupancy (SINGLE: ~100 VGPRs)
    // a segment pays 6 extra rows; a launch that cannot fill the slots (a single pair in the tolerant mode) goes down to 12 rows
    const Segments sg = wave_segments(a.H, strips, slots, kLksSegRows, 12);
    a.Hs = sg.rows;
    a.segs = sg.segs;
    const long nwave = strips * a.segs;
    dim3 grid((unsigned)((nwave + 3) / 4)), block(256);
    const bool frames_ok = u8 ? (aligned(a.prev, 2) && aligned(a.curr, 2)) : (aligned(a.prev, 8) && aligned(a.curr, 8));
    const bool vec = (a.W & 1) == 0 && a.W >= 2 && frames_ok && aligned(a.ou, 8) && aligned(a.ov, 8) &&
                     (MODE != MODE_ITER || (aligned(a.fl[0], 16) && aligned(a.fl[1], 16)));
    // WV: the warp's arithmetic; UPS: the flow upsampling fused in; HW: the half window
    const auto stream = [&](auto WV, auto UPS, auto HW) {
        with_pix(u8, [&](auto PIX) {
            with_bool(vec, [&](auto VEC) {
                hipLaunchKernelGGL((k_lks<MODE, decltype(VEC)::value, decltype(WV)::value, typename decltype(PIX)::type, decltype(UPS)::value,
                                          decltype(HW)::value>), grid, block, 0, s, a);
            });
        });
    };
    if constexpr (MODE == MODE_ITER) {
        // a level's first iteration with the flow upsampling fused in (tolerant mode) exists for the fused-lerp warp only
        if (a.up_src != nullptr) stream(int_c<WARP_LERP64>, std::true_type{}, int_c<2>);
        else if (warp == WARP_LERP64) stream(int_c<WARP_LERP64>, std::false_type{}, int_c<2>);
        else stream(int_c<WARP_SCIPY>, std::false_type{}, int_c<2>);
    } else if (hw == 3) {   // single-scale only
        stream(int_c<WARP_SCIPY>, std::false_type{}, int_c<3>);
    } else {
        stream(int_c<WARP_SCIPY>, std::false_type{}, int_c<2>);
    }
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

inline dim3 grid2d(int W, int H, int n) { return dim3((W + 63) / 64, (H + 3) / 4, n); }
// k_resample: 4 outputs per thread along x
inline dim3 grid_resample(int W, int H, int n) { return dim3((W + 255) / 256, (H + 3) / 4, n); }

// Does the source span of every run of `tile` resampled indices (T of them, spread over S source ones) fit `cap` staged
// source elements?  Exactly the index arithmetic of k_pyr_down and k_upsample, evaluated for each tile row / column.
bool span_ok(int S, int T, int tile, int cap)
{
    Linspace l = make_linspace(S, T);
    auto at = [&](int i) { return T <= 1 ? 0.0 : (i == T - 1 ? l.last : (double)i * l.step); };
    for (int t0 = 0; t0 < T; t0 += tile) {
        int last = std::min(t0 + tile, T) - 1;
        int lo = (int)std::floor(at(t0));
        if (t0 + tile >= T) lo = std::min(lo, std::max(S - 2, 0));
        int hi = std::min((int)std::floor(at(last)) + 1, S - 1);
        if (hi - lo + 1 > cap) return false;
    }
    return true;
}

// Which path a pyramid step takes.  Tight: every 32 x 16 coarse tile samples at most 32 x 64 blurred values (the half-scale
// ratio).  General: at most 34 x 66.  Otherwise the unfused chain.
enum { PYR_UNFUSED = 0, PYR_GENERAL = 1, PYR_TIGHT = 2 };
int pyr_form(int h, int w, int ho, int wo, const GaussW &g)
{
    if (g.radius != 8) return PYR_UNFUSED;
    if (span_ok(h, ho, kPTH, kPBHT) && span_ok(w, wo, kPTW, kPBWT)) return PYR_TIGHT;
    return span_ok(h, ho, kPTH, kPBH) && span_ok(w, wo, kPTW, kPBW) ? PYR_GENERAL : PYR_UNFUSED;
}

// Is a tight step at the exact half-scale ratio, i.e. does np.linspace(0, S - 1, T) put every point but its last in
// [2 i, 2 i + 1) on both axes?  Evaluated on the values the kernel receives.  The tight form alone does not say so: its spans
// also fit at other ratios of the radius-8 band (scale factor 0.52, say), where floor(i * step) leaves 2 i.
bool half_axis(int S, int T)
{
    if (T < 2) return false;
    const Linspace l = make_linspace(S, T);
    for (int i = 0; i < T - 1; i++)
        if (std::floor((double)i * l.step) != (double)(2 * i)) return false;
    return true;
}
bool pyr_half(int h, int w, int ho, int wo, const GaussW &g)
{
    return pyr_form(h, w, ho, wo, g) == PYR_TIGHT && half_axis(h, ho) && half_axis(w, wo);
}

// does every 32 x 16 coarse tile's source span fit one of the fused kernel's LDS tiles?
bool pyr_fused_fits(int h, int w, int ho, int wo, const GaussW &g) { return pyr_form(h, w, ho, wo, g) != PYR_UNFUSED; }

// does every 256 x 4 output block of k_upsample find its coarse source span inside the staged LDS tile?
bool upsample_fits(int hc, int wc, int ht, int wt) { return span_ok(hc, ht, kUTH, kUSH) && span_ok(wc, wt, kUTW, kUSW); }

// The geometry of upsample_flow from a coarse hc x wc field to h x w (lucas_kanade_pyramidal.py:122-136): both planes,
// values scaled by the size ratios.  The caller adds its planes.
ResampleArgs upsample_args(int hc, int wc, int h, int w)
{
    ResampleArgs r{};
    r.scale[0] = (float)((double)w / (double)wc);  // scale_x (:123, :135)
    r.scale[1] = (float)((double)h / (double)hc);  // scale_y (:122, :136)
    r.H = hc; r.W = wc; r.Ho = h; r.Wo = w;
    r.ly = make_linspace(hc, h);
    r.lx = make_linspace(wc, w);
    r.nplanes = 2;
    r.apply_scale = 1;
    return r;
}

// upsample_flow of `nimg` flow fields (both planes); r is fully populated by the caller
int launch_upsample(oflk_plan *plan, hipStream_t s, const ResampleArgs &r_in, int nimg)
{
    ResampleArgs r = r_in;
    // 16-byte stores want Wo % 4 == 0 and 16-byte aligned output planes (hipMalloc / torch give that)
    r.vec_store = (r.Wo & 3) == 0 && aligned(r.out[0], 16) && (r.interleaved || aligned(r.out[1], 16));
    Prof pr(plan, s, KC_UPSAMPLE);
    if (upsample_fits(r.H, r.W, r.Ho, r.Wo)) {
        dim3 grid((r.Wo + kUTW - 1) / kUTW, (r.Ho + kUTH - 1) / kUTH, nimg);
        // a one-row or one-column coarse field keeps run-time tap strides; every other one has them at compile time
        if (r.H == 1 || r.W == 1) hipLaunchKernelGGL(k_upsample<true>, grid, dim3(256), 0, s, r);
        else hipLaunchKernelGGL(k_upsample<false>, grid, dim3(256), 0, s, r);
    } else {
        hipLaunchKernelGGL(k_resample<2>, grid_resample(r.Wo, r.Ho, nimg), dim3(256), 0, s, r);
    }
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// what the first pyramid launch of a pyramidal call carries besides its own work
struct PyrExtra {
    const float *in2 = nullptr;   // images nsplit .. nimg-1 (the second caller buffer)
    int nsplit = 0;
    unsigned *zero_words = nullptr;   // per-call state to clear
    size_t n_zero_words = 0;
    float *zero_u = nullptr, *zero_v = nullptr;   // coarsest-level flow planes to clear
    size_t n_zero_flow = 0;
    bool u8 = false;                  // the input images are uint8 (the caller's frames of a uint8 plan)
};

// the clear that every pass of a pyramidal call starts from: the per-call state (acc, iters_run, uncertain, log) = 0 and
// flow = zeros at the coarsest level (lucas_kanade_pyramidal.py:182-184; slot 0: u then v, B * n floats each)
PyrExtra call_clear(const oflk_plan *p)
{
    PyrExtra x;
    x.zero_words = reinterpret_cast<unsigned *>(p->state);
    x.n_zero_words = p->state_words();
    x.n_zero_flow = (size_t)p->B * p->npix(0);
    x.zero_u = reinterpret_cast<float *>(p->fl(0, 0));
    x.zero_v = x.zero_u + x.n_zero_flow;
    return x;
}

int launch_call_init(oflk_plan *plan, hipStream_t s, const PyrExtra &x)
{
    Prof pr(plan, s, KC_INIT);
    hipLaunchKernelGGL(k_call_init, dim3(256), dim3(256), 0, s, x.zero_words, x.n_zero_words, x.zero_u, x.zero_v,
                       x.n_zero_flow);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// gaussian blur + linspace resample of `nimg` images: in [nimg][h][w] -> out [nimg][ho][wo]
int launch_pyr_down(oflk_plan *plan, const GaussW &gauss, hipStream_t s, const float *in, float *out,
                    float *tmpA, float *tmpB, int nimg, int h, int w, int ho, int wo,
                    const PyrExtra *extra = nullptr)
{
    if (const int form = pyr_form(h, w, ho, wo, gauss); form != PYR_UNFUSED) {
        PyrArgs a{};
        a.in = in;
        a.in2 = in;
        a.nsplit = nimg;
        if (extra) {
            if (extra->in2) {
                a.in2 = extra->in2;
                a.nsplit = extra->nsplit;
            }
            a.zero_words = extra->zero_words;
            a.n_zero_words = extra->n_zero_words;
            a.zero_u = extra->zero_u;
            a.zero_v = extra->zero_v;
            a.n_zero_flow = extra->n_zero_flow;
        }
        a.out = out;
        a.H = h; a.W = w; a.Ho = ho; a.Wo = wo;
        a.ly = make_linspace(h, ho);
        a.lx = make_linspace(w, wo);
        for (int k = 0; k <= 8; k++) a.w[k] = gauss.w[k];
        dim3 grid((wo + kPTW - 1) / kPTW, (ho + kPTH - 1) / kPTH, nimg);
        Prof pr(plan, s, KC_PYR_FUSED);
        // contracted / tolerant plans: the opt-in fused sums as they are.  The exact arithmetic (every other plan, and no
        // plan at all) runs them behind the rounding certificate, which leaves SciPy's results
        constexpr int kExactForm = PYR_CERTIFIED;
        const int arith = contracted_pyramid(plan) ? PYR_CONTRACTED : kExactForm;
        // the tile: a tight step at the exact half-scale ratio takes the instantiation with compile-time tap and staging offsets
        const int tile = form != PYR_TIGHT ? PYR_TILE_GENERAL : (pyr_half(h, w, ho, wo, gauss) ? PYR_TILE_HALF : PYR_TILE_TIGHT);
        with_pix(extra && extra->u8, [&](auto PIX) {
            with_int<PYR_CONTRACTED, kExactForm>(arith, [&](auto ARITH) {
                with_int<PYR_TILE_GENERAL, PYR_TILE_TIGHT, PYR_TILE_HALF>(tile, [&](auto TILE) {
                    hipLaunchKernelGGL((k_pyr_down<typename decltype(PIX)::type, decltype(ARITH)::value, decltype(TILE)::value>), grid,
                                       dim3(256), 0, s, a);
                });
            });
        });
        HIP_TRY(hipGetLastError());
        return OFLK_OK;
    }
    if (extra) {
        // unfused path: the extras become launches of their own
        if (extra->zero_words) {
            int rc = launch_call_init(plan, s, *extra);
            if (rc) return rc;
        }
        if (extra->in2) {
            int rc = launch_pyr_down(plan, gauss, s, in, out, tmpA, tmpB, extra->nsplit, h, w, ho, wo);
            if (rc) return rc;
            return launch_pyr_down(plan, gauss, s, extra->in2, out + (size_t)extra->nsplit * ho * wo, tmpA, tmpB,
                                   nimg - extra->nsplit, h, w, ho, wo);
        }
    }
    {
        Prof pr(plan, s, KC_BLUR);
        const bool fma = contracted_pyramid(plan);   // the unfused chain keeps the plan's arithmetic
        with_bool(fma, [&](auto FMA) {
            hipLaunchKernelGGL((k_blur<0, decltype(FMA)::value>), grid2d(w, h, nimg), dim3(256), 0, s, in, tmpA, h, w, gauss);
        });
        HIP_TRY(hipGetLastError());
        with_bool(fma, [&](auto FMA) {
            hipLaunchKernelGGL((k_blur<1, decltype(FMA)::value>), grid2d(w, h, nimg), dim3(256), 0, s, (const float *)tmpA, tmpB, h, w, gauss);
        });
        HIP_TRY(hipGetLastError());
    }
    ResampleArgs r{};
    r.in[0] = tmpB;
    r.out[0] = out;
    r.acc = nullptr;
    r.in_sel_stride = 0;
    r.H = h; r.W = w; r.Ho = ho; r.Wo = wo;
    r.ly = make_linspace(h, ho);
    r.lx = make_linspace(w, wo);
    r.nplanes = 1;
    r.apply_scale = 0;
    r.vec_store = (wo & 3) == 0 && aligned(out, 16);
    {
        Prof pr(plan, s, KC_RESAMPLE);
        with_bool(contracted_pyramid(plan), [&](auto FMA) {
            hipLaunchKernelGGL((k_resample<1, decltype(FMA)::value>), grid_resample(wo, ho, nimg), dim3(256), 0, s, r);
        });
    }
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the first step of a pyramid, from the finest down, that the fused kernel cannot take (its coarser level); -1: none
int pyr_first_unfused(const int *dims, int levels, const GaussW &gauss)
{
    for (int l = levels - 2; l >= 0; l--)
        if (!pyr_fused_fits(dims[2 * (l + 1)], dims[2 * (l + 1) + 1], dims[2 * l], dims[2 * l + 1], gauss)) return l;
    return -1;
}

// the refusal of a caller that has no temporaries for the unfused chain
int pyr_chain_fits(const int *dims, int levels, const GaussW &gauss)
{
    const int l = pyr_first_unfused(dims, levels, gauss), *fine = dims + 2 * (levels - 1);
    return l < 0 ? OFLK_OK : fail(OFLK_ERR_UNSUPPORTED, "pyramid level %d of %dx%d does not fit the fused pyramid kernel", l, fine[1], fine[0]);
}

// The level walk of one set of n images: from `fine` (level levels-1) into image img0 onward of out[levels-2] .. out[0]; `first`
// rides on the first launch.  plan, tmpA, tmpB: a plan's (Prof timing, arithmetic, the unfused chain), or NULL behind pyr_chain_fits
int pyr_chain(oflk_plan *plan, const GaussW &gauss, hipStream_t s, const float *fine, float *const *out, size_t img0, float *tmpA,
              float *tmpB, int n, const int *dims, int levels, const PyrExtra &first)
{
    const float *in = fine;
    for (int l = levels - 2; l >= 0; l--) {
        const int ho = dims[2 * l], wo = dims[2 * l + 1];
        float *const o = out[l] + img0 * (size_t)ho * (size_t)wo;
        if (int rc = launch_pyr_down(plan, gauss, s, in, o, tmpA, tmpB, n, dims[2 * (l + 1)], dims[2 * (l + 1) + 1], ho, wo,
                                     l == levels - 2 ? &first : nullptr))
            return rc;
        in = o;
    }
    return OFLK_OK;
}

template <typename T>
int dmalloc(T **p, size_t n, size_t *total)
{
    size_t bytes = std::max<size_t>(n * sizeof(T), 256);
    hipError_t e = hipMalloc((void **)p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        return fail(OFLK_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    *total += bytes;
    return OFLK_OK;
}

// blur temporaries for `nimg` images of the plan's frame size (the unfused pyramid chain)
int ensure_tmp(oflk_plan *p, size_t nimg)
{
    if (p->tmp_imgs >= nimg) return OFLK_OK;
    const size_t N = (size_t)p->H * p->W;
    for (float **q : {&p->tmpA, &p->tmpB}) {
        if (*q) {
            (void)hipFree(*q);
            p->ws_bytes -= std::max<size_t>(p->tmp_imgs * N * sizeof(float), 256);
        }
        *q = nullptr;
    }
    p->tmp_imgs = 0;
    int rc = dmalloc(&p->tmpA, nimg * N, &p->ws_bytes);
    if (!rc) rc = dmalloc(&p->tmpB, nimg * N, &p->ws_bytes);
    if (!rc) p->tmp_imgs = nimg;
    return rc;
}

// what only the dense pyramidal passes use: every level's two flow slots and blur temporaries for 2B images
int ensure_dense_ws(oflk_plan *p)
{
    int rc;
    for (int l = 0; l < p->L; l++)
        if (!p->flow[l] && (rc = dmalloc(&p->flow[l], (size_t)2 * 2 * p->B * p->npix(l), &p->ws_bytes))) return rc;   // two interleaved slots
    return p->L > 1 ? ensure_tmp(p, 2 * (size_t)p->B) : OFLK_OK;
}

void plan_free(oflk_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    for (int l = 0; l < OFLK_MAX_LEVELS; l++) {
        if (p->pyr[l]) (void)hipFree(p->pyr[l]);
        if (p->flow[l]) (void)hipFree(p->flow[l]);
    }
    if (p->tmpA) (void)hipFree(p->tmpA);
    if (p->tmpB) (void)hipFree(p->tmpB);
    if (p->state) (void)hipFree(p->state);
    if (p->state_b) (void)hipFree(p->state_b);
    if (p->redo) (void)hipFree(p->redo);
    for (auto &q : p->u8_stage)
        if (q) (void)hipFree(q);
    for (int l = 0; l < OFLK_MAX_LEVELS; l++)
        for (float *q : {p->exact.pyr[l], p->exact.u[l], p->exact.v[l]})
            if (q) (void)hipFree(q);
    for (float *q : {p->exact.warped, p->exact.du, p->exact.dv, p->exact.f32[0], p->exact.f32[1], p->exact.pieces})
        if (q) (void)hipFree(q);
    for (auto &e : p->pending) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    for (auto &e : p->pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    delete p;
}

}  // namespace

// =============================================================================
// library
// =============================================================================
OFLK_API const char *oflk_version(void) { return "oflk 0.4.0 (gfx950)"; }

OFLK_API int oflk_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

OFLK_API const char *oflk_last_error(void) { return t_err.c_str(); }

OFLK_API int oflk_set_device(int device)
{
    int rc = ensure_device(device);
    if (rc == OFLK_OK) g_device = device;
    return rc;
}

OFLK_API int oflk_pyramid_level_dims(int H, int W, int levels, double scale_factor, int *dims_out)
{
    if (!dims_out) return fail(OFLK_ERR_INVALID, "dims_out is NULL");
    return level_dims(H, W, levels, scale_factor, dims_out);
}

// =============================================================================
// plan API
// =============================================================================
// the largest frames a plan or a tracker takes
static int check_frame_bounds(int H, int W)
{
    if ((size_t)H * (size_t)W >= ((size_t)1 << 29))
        return fail(OFLK_ERR_UNSUPPORTED, "frames of 2^29 pixels or more are not supported");  // 32-bit byte offsets into float2 planes
    if (H >= kMaxDim || W >= kMaxDim)
        return fail(OFLK_ERR_UNSUPPORTED, "frames of 2^23 rows or columns or more are not supported (got %d x %d)", H, W);
    return OFLK_OK;
}

OFLK_API int oflk_plan_create(oflk_plan **out, int device, int B, int H, int W, int levels,
                              int window_size, int iters)
{
    if (!out) return fail(OFLK_ERR_INVALID, "plan pointer is NULL");
    *out = nullptr;
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1");
    if (iters < 0) return fail(OFLK_ERR_INVALID, "iters must be >= 0");
    int hw = 0;
    int rc = check_frame_bounds(H, W);
    if (rc || (rc = window_hw(window_size, &hw))) return rc;
    int dims[2 * OFLK_MAX_LEVELS];
    rc = level_dims(H, W, levels, 0.5, dims);
    if (rc) return rc;
    rc = ensure_device(device);
    if (rc) return rc;

    oflk_plan *p = new oflk_plan();
    p->device = device;
    p->B = B; p->H = H; p->W = W; p->L = levels; p->win = window_size; p->hw = hw; p->K = iters;
    std::memcpy(p->dims, dims, sizeof(int) * 2 * levels);
    rc = make_gauss(2.0, &p->gauss);  // sigma = 1/scale_factor, scale_factor = 0.5 (:24, :46)
    // the pyramid, the per-call state and the redo list; the dense passes' flow slots and blur temporaries come with the
    // first pass that needs them (ensure_dense_ws), which is why a plan's first pass of a kind is eager
    for (int l = 0; l < levels - 1 && !rc; l++) rc = dmalloc(&p->pyr[l], 2 * (size_t)B * p->npix(l), &p->ws_bytes);
    if (!rc) rc = dmalloc(&p->state, p->state_words() / 2, &p->ws_bytes);
    if (!rc && (p->hw == 2 || p->hw == 3)) {
        // redo list of the single-scale streaming kernel (LkArgs::redo): all zero between calls
        const size_t n = 2 + 2 * (size_t)B * ((W + k5TX - 1) / k5TX) * ((H + k5TY - 1) / k5TY);
        rc = dmalloc(&p->redo, n, &p->ws_bytes);
        if (!rc && hipMemset(p->redo, 0, std::max<size_t>(n * sizeof(unsigned), 256)) != hipSuccess) rc = fail(OFLK_ERR_HIP, "hipMemset of the redo list failed");
    }
    if (rc) {
        std::string keep = t_err;
        plan_free(p);
        t_err = keep;
        return rc;
    }
    *out = p;
    return OFLK_OK;
}

OFLK_API int oflk_plan_destroy(oflk_plan *plan)
{
    plan_free(plan);
    return OFLK_OK;
}

OFLK_API size_t oflk_plan_workspace_bytes(const oflk_plan *plan) { return plan ? plan->ws_bytes : 0; }

namespace {
int plan_single_scale(oflk_plan *p, const void *d_prev, const void *d_curr, bool u8, float *d_u, float *d_v,
                      hipStream_t s)
{
    if (!p || !d_prev || !d_curr || !d_u || !d_v) return fail(OFLK_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    LkArgs a{};
    a.prev = static_cast<const float *>(d_prev);   // element type is the kernel's PIX (launch_lk, u8)
    a.curr = static_cast<const float *>(d_curr);
    a.ou = d_u; a.ov = d_v;
    a.H = p->H; a.W = p->W;
    // The streaming kernel walks rows one after the other inside a wave: a launch too small to fill the chip's wave slots with
    // segments of ~40 rows is latency-bound there (one 640x480 pair: 37 us against the tile kernel's 6), so small launches
    // keep the tile kernel -- both are exact, the choice is speed only.
    const long stream_waves = ((long)p->W + kLksOutW - 1) / kLksOutW * p->B * std::max(1, p->H / 40);
    if ((p->hw == 2 || p->hw == 3) && p->H > 2 * p->hw && p->W > 2 * p->hw &&
        ((p->kernels == OFLK_KERNELS_AUTO && stream_waves >= 2048) || p->kernels == OFLK_KERNELS_STREAM)) {
        // 5x5 window: the streaming kernel, whose order-free sums are NumPy's wherever the frames are integers in [0, 255]
        // and a window's Sxx, Syy stay below 2^16 (proof at kLksExactBound); it flags the tiles where that is in doubt and
        // the tile kernel redoes exactly those in NumPy's order.  Results are the reference's either way.
        a.redo = p->redo;   // allocated and zeroed with the plan
        int rc = launch_lks<MODE_SINGLE>(p, s, KC_LK_SINGLE, a, p->B, u8, WARP_SCIPY, p->hw);
        if (rc) return rc;
        a.redo_pass = 1;
        return launch_lk<MODE_SINGLE>(p, s, KC_LK_REDO, p->hw, a, p->B, u8);
    }
    return launch_lk<MODE_SINGLE>(p, s, KC_LK_SINGLE, p->hw, a, p->B, u8);
}
// seq: d_curr == d_prev + one plane, both inside one buffer of B+1 frames (oflk_plan_pyramidal_sequence); d_ub, d_vb
// (a sequence only): the backward flows too, on the same pyramid (oflk_plan_pyramidal_sequence_fb)
int plan_pyramidal(oflk_plan *p, const void *d_prev, const void *d_curr, bool u8, float *d_u, float *d_v, hipStream_t s,
                   bool seq = false, float *d_ub = nullptr, float *d_vb = nullptr);
// level_out = false: the coarser levels' flows are not written where oflk_plan_read_level_flow looks
int resolve_pair(oflk_plan *p, int b, const void *d_prev_in, const void *d_curr_in, bool u8, float *d_u, float *d_v, hipStream_t s,
                 bool level_out = true);
}  // namespace

OFLK_API int oflk_plan_single_scale(oflk_plan *p, const float *d_prev, const float *d_curr,
                                    float *d_u, float *d_v, void *stream)
{
    return plan_single_scale(p, d_prev, d_curr, false, d_u, d_v, (hipStream_t)stream);
}

// BASELINE config 5: fp16 gradients / accumulators (k_lk16d).  pixel_max bounds the frame values.
OFLK_API int oflk_plan_single_scale_fp16(oflk_plan *p, const float *d_prev, const float *d_curr, float *d_u, float *d_v,
                                         float pixel_max, void *stream)
{
    if (!p || !d_prev || !d_curr || !d_u || !d_v) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (!(pixel_max > 0.0f) || !std::isfinite(pixel_max)) return fail(OFLK_ERR_INVALID, "pixel_max must be positive and finite");
    HIP_TRY(hipSetDevice(p->device));
    const int hw = p->hw, taps = (2 * hw + 1) * (2 * hw + 1);
    // s_g = 2^-k, the largest power of two (<= 1) with taps * (pixel_max / 2 * s_g)^2 <= 60000
    int k = 0;
    while ((double)taps * std::pow(0.5 * (double)pixel_max * std::ldexp(1.0, -k), 2.0) > 60000.0) k++;
    // one wave per (strip of 128 - 4 ceil(R/2) output columns, segment of Hs rows): two columns per lane (k_lk16d;
    // 7x7: 77 VGPRs = 6 waves per SIMD, halo 6 %).  wave_segments sizes the segments, ~64 rows each (a segment pays 2R
    // extra rows of loads).
    Lk16sArgs g{};
    g.prev = d_prev; g.curr = d_curr; g.u = d_u; g.v = d_v;
    g.H = p->H; g.W = p->W; g.B = p->B;
    g.s_g = (float)std::ldexp(1.0, -k);
    g.s_t = 0.5f * g.s_g;
    g.det_thr = (float)(1e-4 * std::ldexp(1.0, -4 * k));
    hipStream_t s = (hipStream_t)stream;
    Prof pr(p, s, KC_LK_SINGLE);
    const int outw = 2 * (64 - 2 * ((hw + 2) / 2));
    const long strips = ((long)g.W + outw - 1) / outw * g.B;
    const long slots = hw <= 2 ? 8192 : hw == 3 ? 6144 : hw == 4 ? 5120 : 4096;   // wave slots of the chip at 8 / 8 / 6 / 5 / 4 waves per SIMD
    const Segments sg = wave_segments(g.H, strips, slots, 64, 0);
    g.Hs = sg.rows;
    g.segs = sg.segs;
    const long nwave = strips * g.segs;
    dim3 sgrid((unsigned)((nwave + 3) / 4)), sblock(256);
    const bool vec8 = (g.W & 1) == 0 && g.W >= 2 && aligned(d_prev, 8) && aligned(d_curr, 8) && aligned(d_u, 8) && aligned(d_v, 8);   // 8-byte column pairs
    const bool built = with_half_window(hw, [&](auto HW) {
        with_bool(vec8, [&](auto VEC) {
            hipLaunchKernelGGL((k_lk16d<decltype(HW)::value, decltype(VEC)::value>), sgrid, sblock, 0, s, g);
        });
    });
    if (!built) return fail(OFLK_ERR_UNSUPPORTED, "half window %d not built", hw);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

OFLK_API int oflk_plan_single_scale_u8(oflk_plan *p, const unsigned char *d_prev, const unsigned char *d_curr,
                                       float *d_u, float *d_v, void *stream)
{
    return plan_single_scale(p, d_prev, d_curr, true, d_u, d_v, (hipStream_t)stream);
}

OFLK_API int oflk_plan_pyramidal(oflk_plan *p, const float *d_prev, const float *d_curr, float *d_u,
                                 float *d_v, void *stream)
{
    return plan_pyramidal(p, d_prev, d_curr, false, d_u, d_v, (hipStream_t)stream);
}

OFLK_API int oflk_plan_pyramidal_u8(oflk_plan *p, const unsigned char *d_prev, const unsigned char *d_curr,
                                    float *d_u, float *d_v, void *stream)
{
    return plan_pyramidal(p, d_prev, d_curr, true, d_u, d_v, (hipStream_t)stream);
}

// A sequence is the pair batch whose pair b reads frames b and b+1 of one buffer: curr = frames + one plane (for uint8 one
// plane of BYTES).  Every kernel addresses pair b as prev + b * plane and curr + b * plane, so only the pyramid changes.
OFLK_API int oflk_plan_pyramidal_sequence(oflk_plan *p, const float *d_frames, float *d_u, float *d_v, void *stream)
{
    if (!p || !d_frames) return fail(OFLK_ERR_INVALID, "NULL argument");
    return plan_pyramidal(p, d_frames, d_frames + (size_t)p->H * p->W, false, d_u, d_v, (hipStream_t)stream, true);
}

OFLK_API int oflk_plan_pyramidal_sequence_u8(oflk_plan *p, const unsigned char *d_frames, float *d_u, float *d_v, void *stream)
{
    if (!p || !d_frames) return fail(OFLK_ERR_INVALID, "NULL argument");
    return plan_pyramidal(p, d_frames, d_frames + (size_t)p->H * p->W, true, d_u, d_v, (hipStream_t)stream, true);
}

// Both directions on one pyramid: the backward pass is the forward one with prev and curr exchanged (plan_pyramidal)
OFLK_API int oflk_plan_pyramidal_sequence_fb(oflk_plan *p, const float *d_frames, float *d_uf, float *d_vf, float *d_ub,
                                             float *d_vb, void *stream)
{
    if (!p || !d_frames || !d_ub || !d_vb) return fail(OFLK_ERR_INVALID, "NULL argument");
    return plan_pyramidal(p, d_frames, d_frames + (size_t)p->H * p->W, false, d_uf, d_vf, (hipStream_t)stream, true, d_ub, d_vb);
}

OFLK_API int oflk_plan_pyramidal_sequence_fb_u8(oflk_plan *p, const unsigned char *d_frames, float *d_uf, float *d_vf,
                                                float *d_ub, float *d_vb, void *stream)
{
    if (!p || !d_frames || !d_ub || !d_vb) return fail(OFLK_ERR_INVALID, "NULL argument");
    return plan_pyramidal(p, d_frames, d_frames + (size_t)p->H * p->W, true, d_uf, d_vf, (hipStream_t)stream, true, d_ub, d_vb);
}

namespace {
int iterate_levels(oflk_plan *p, hipStream_t s, const float *d_prev, const float *d_curr, size_t img_prev, size_t img_curr,
                   bool u8, float *d_u, float *d_v);

// Can the fused pyramid kernel take the caller's uint8 frames?  (Always for scale 0.5 unless a level is tiny.)  Where it
// cannot, the unfused kernels read float32: stage_u8 converts the frames once into the plan's u8_stage buffers.
bool u8_needs_stage(const oflk_plan *p)
{
    const int L = p->L;
    return L > 1 &&
           !pyr_fused_fits(p->dims[2 * (L - 1)], p->dims[2 * (L - 1) + 1], p->dims[2 * (L - 2)], p->dims[2 * (L - 2) + 1], p->gauss);
}

// seq: the B+1 frames at d_prev all go to the first stage; otherwise prev and curr to one each
int stage_u8(oflk_plan *p, hipStream_t s, const void *d_prev_in, const void *d_curr_in, bool seq)
{
    const size_t N = (size_t)p->H * p->W, n = (size_t)p->B * N;
    size_t tot = 0;
    int rc;
    for (int i = 0; i < (seq ? 1 : 2); i++)
        if (!p->u8_stage[i] && (rc = dmalloc(&p->u8_stage[i], i == 0 ? n + N : n, &tot))) return rc;
    p->ws_bytes += tot;
    const size_t n0 = seq ? n + N : n;
    hipLaunchKernelGGL(k_u8_to_f32, dim3((unsigned)((n0 + 4095) / 4096)), dim3(256), 0, s, static_cast<const unsigned char *>(d_prev_in),
                       p->u8_stage[0], n0);
    HIP_TRY(hipGetLastError());
    if (seq) return OFLK_OK;
    hipLaunchKernelGGL(k_u8_to_f32, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, s, static_cast<const unsigned char *>(d_curr_in),
                       p->u8_stage[1], n);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// The pyramids of a pass (lucas_kanade_pyramidal.py:173-174), fine -> coarse, into p->pyr: of prev and curr of every pair
// (images 0..B-1 from d_prev, B..2B-1 from d_curr, one launch per level), or of a sequence's B+1 frames, each once (one
// buffer at d_prev).  The finest level is the caller's frames (image.copy() at :40 is a no-op here).  `first` rides on the
// first launch: the call's clear, and whether the frames are uint8.
int build_pyramids(oflk_plan *p, hipStream_t s, const float *d_prev, const float *d_curr, bool seq, PyrExtra first)
{
    first.in2 = seq ? nullptr : d_curr;
    first.nsplit = seq ? 0 : p->B;
    return pyr_chain(p, p->gauss, s, d_prev, p->pyr, 0, p->tmpA, p->tmpB, seq ? p->B + 1 : 2 * p->B, p->dims, p->L, first);
}

int plan_pyramidal(oflk_plan *p, const void *d_prev_in, const void *d_curr_in, bool u8, float *d_u, float *d_v,
                   hipStream_t s, bool seq, float *d_ub, float *d_vb)
{
    if (!p || !d_prev_in || !d_curr_in || !d_u || !d_v) return fail(OFLK_ERR_INVALID, "NULL argument");
    const bool fb = d_ub || d_vb;
    if (fb && (!seq || !d_ub || !d_vb)) return fail(OFLK_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    const int B = p->B, L = p->L;
    int rc;
    if (fb && !p->state_b) {
        // the backward pass's state block, once per plan (this allocation is why the first bidirectional call is eager)
        if ((rc = dmalloc(&p->state_b, p->state_words() / 2, &p->ws_bytes))) return rc;
    }
    p->last_fb = fb;
    if (u8 && u8_needs_stage(p)) {
        // the unfused pyramid kernels read float32: convert once and run the float path
        if ((rc = stage_u8(p, s, d_prev_in, d_curr_in, seq))) return rc;
        if (seq) return plan_pyramidal(p, p->u8_stage[0], p->u8_stage[0] + (size_t)p->H * p->W, false, d_u, d_v, s, true, d_ub, d_vb);
        return plan_pyramidal(p, p->u8_stage[0], p->u8_stage[1], false, d_u, d_v, s);
    }
    // typed float for the common case; with u8 the kernels of the finest level read them as uint8
    const float *d_prev = static_cast<const float *>(d_prev_in), *d_curr = static_cast<const float *>(d_curr_in);

    // every level's flow lives in two interleaved {u, v} ping-pong slots of the plan; only the finest
    // level's last launch writes the caller's planar planes (k_export_fixup de-interleaves the rest).  They and the blur
    // temporaries are allocated by a plan's first dense pass (this allocation is why that pass is eager)
    if ((rc = ensure_dense_ws(p))) return rc;

    if (!tiled_window(p->hw)) {
        // 1x1 / 13x13 and larger windows have no fused iteration kernel: every pair runs the reference's own sequence of
        // steps with the standalone kernels (resolve_pair: pyramid, warp, generic single-scale LK, flow += d, upsample,
        // np.mean in NumPy's order, the exit test on the host) -- exact, and as slow as that sounds
        for (int b = 0; b < B; b++)
            if ((rc = resolve_pair(p, b, d_prev_in, d_curr_in, u8, d_u, d_v, s))) return rc;
        if (fb) {   // the backward pairs: frames exchanged, into the second state block
            StateSwap sw(p, true);
            for (int b = 0; b < B; b++)
                if ((rc = resolve_pair(p, b, d_curr_in, d_prev_in, u8, d_ub, d_vb, s))) return rc;
        }
        return OFLK_OK;
    }

    // the call's clear: carried by the first pyramid launch, or a launch of its own when there is no pyramid
    PyrExtra first = call_clear(p);
    if (L == 1) {
        rc = launch_call_init(p, s, first);
        if (rc) return rc;
    }

    first.u8 = u8;
    if ((rc = build_pyramids(p, s, d_prev, d_curr, seq, first))) return rc;

    // pair b reads pyramid images b and B + b, or a sequence's frames b and b + 1
    if ((rc = iterate_levels(p, s, d_prev, d_curr, 0, seq ? 1 : B, u8, d_u, d_v)) || !fb) return rc;
    // the backward pass on the same pyramid: pair b reads frames b + 1 and b, with its own state block and the coarsest
    // level's flow cleared again (stream order puts this after the forward pass's last reads of both)
    StateSwap sw(p, true);
    if ((rc = launch_call_init(p, s, call_clear(p)))) return rc;
    return iterate_levels(p, s, d_curr, d_prev, 1, 0, u8, d_ub, d_vb);
}

// Does level l run the streaming kernel?  Tolerant mode inside its envelope: the two finest levels (order-free window sums,
// fused-lerp warp).  The launches of the level and the guards of its exit decisions (k_export_fixup) both follow this.
bool level_streams(const oflk_plan *p, int l)
{
    return p->arith == OFLK_ARITH_TOLERANT && tolerant_relaxes(p->L, p->hw, p->K) && l >= p->L - 2 && p->dims[2 * l] > 4 &&
           p->dims[2 * l + 1] > 4;
}

// The level loop (lucas_kanade_pyramidal.py:186-223) and the export of one direction: pair b reads prev image img_prev + b
// and curr image img_curr + b of every coarser pyramid level, and d_prev / d_curr + b * plane at the finest level.  The
// plan's per-call state (acc, iters_run, uncertain, log) and the coarsest level's flow are already cleared.
int iterate_levels(oflk_plan *p, hipStream_t s, const float *d_prev, const float *d_curr, size_t img_prev, size_t img_curr,
                   bool u8, float *d_u, float *d_v)
{
    const int B = p->B, L = p->L, K = p->K;
    int rc;
    for (int l = 0; l < L; l++) {
        const int h = p->dims[2 * l], w = p->dims[2 * l + 1];
        const size_t n = (size_t)h * w;
        // the flow upsampling into a level of the streaming kernel is fused into its first iteration
        const bool stream = level_streams(p, l);
        const bool fuse_up = stream && l > 0 && K >= 1 && p->dims[2 * (l - 1)] >= 2 && p->dims[2 * (l - 1) + 1] >= 2;
        if (l > 0 && !fuse_up) {
            // upsample_flow (:195-197) from whichever slot holds level l-1's result
            ResampleArgs r = upsample_args(p->dims[2 * (l - 1)], p->dims[2 * (l - 1) + 1], h, w);
            // interleaved planes: slot s of level l-1 sits s * (B*n_c) float2 elements after slot 0
            r.interleaved = 1;
            r.in[0] = reinterpret_cast<const float *>(p->fl(l - 1, 0));
            r.acc = p->acc();
            r.acc_level = l - 1; r.L = L; r.K = p->Kc(); r.iters = K;
            r.acc_thr = conv_threshold((double)p->npix(l - 1));
            r.in_sel_stride = (size_t)B * p->npix(l - 1);
            r.out[0] = reinterpret_cast<float *>(p->fl(l, 0));
            rc = launch_upsample(p, s, r, B);
            if (rc) return rc;
        }
        const float *lp = (l == L - 1) ? d_prev : p->pyr[l] + img_prev * n;
        const float *lc = (l == L - 1) ? d_curr : p->pyr[l] + img_curr * n;
        for (int k = 0; k < K; k++) {
            LkArgs a{};
            a.prev = lp; a.curr = lc;
            a.fl[0] = p->fl(l, 0); a.fl[1] = p->fl(l, 1);
            a.ou = d_u; a.ov = d_v;
            a.planar_out = (l == L - 1 && k == K - 1) ? 1 : 0;
            a.acc = p->acc();
            a.conv_thr = conv_threshold((double)n);
            a.level = l; a.iter = k; a.L = L; a.K = p->Kc();
            a.H = h; a.W = w;
            if (fuse_up && k == 0) {
                const ResampleArgs r = upsample_args(p->dims[2 * (l - 1)], p->dims[2 * (l - 1) + 1], h, w);
                a.up_src = p->fl(l - 1, 0);
                a.up_slot_stride = (size_t)B * p->npix(l - 1);
                a.up_level = l - 1;
                a.up_iters = K;
                a.up_thr = conv_threshold((double)p->npix(l - 1));
                a.Hc = r.H; a.Wc = r.W;
                a.up_ly = r.ly; a.up_lx = r.lx;
                a.up_sx = r.scale[0]; a.up_sy = r.scale[1];
            }
            if (stream) rc = launch_lks<MODE_ITER>(p, s, l == L - 1 ? KC_LK_ITER_FINEST : KC_LK_ITER, a, B, u8 && l == L - 1, WARP_LERP64);
            else rc = launch_lk<MODE_ITER>(p, s, l == L - 1 ? KC_LK_ITER_FINEST : KC_LK_ITER, p->hw, a, B, u8 && l == L - 1);
            if (rc) return rc;
        }
    }
    // pairs whose finest level exited early hold their result in the internal slot
    {
        ExportArgs e{};
        e.src[0] = p->fl(L - 1, 0);
        e.src[1] = p->fl(L - 1, 1);
        e.dst_u = d_u;
        e.dst_v = d_v;
        e.acc = p->acc();
        e.want = 0;
        e.L = L; e.K = p->Kc(); e.iters = K;
        for (int l = 0; l < L; l++) {
            e.counts[l] = (double)p->npix(l);
            e.thr[l] = conv_threshold(e.counts[l]);
        }
        e.log = p->log();
        e.iters_run = p->iters_run();
        e.uncertain = p->uncertain();
        for (int l = 0; l < L; l++) {
            const double t = (double)e.thr[l];
            const double g = decision_guard(level_streams(p, l) ? SUM_STREAM : SUM_TILES, p->dims[2 * l], p->dims[2 * l + 1]);
            e.guard_lo[l] = (unsigned long long)std::floor(t * (1.0 - g));
            e.guard_hi[l] = (unsigned long long)std::ceil(t * (1.0 + g));
        }
        e.plane = (size_t)p->H * p->W;
        // few blocks per pair: the copy is the rare case, the common one is "nothing to do"
        dim3 grid((unsigned)std::min<size_t>((e.plane + 255) / 256, 128), B);
        Prof pr(p, s, KC_EXPORT);
        hipLaunchKernelGGL(k_export_fixup, grid, dim3(256), 0, s, e);
        HIP_TRY(hipGetLastError());
    }
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_plan_read_log(oflk_plan *p, float *residual_log, int *iters_run, void *stream)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    if (residual_log)
        HIP_TRY(hipMemcpyAsync(residual_log, p->log(),
                               (size_t)p->B * p->L * std::max(p->K, 1) * 2 * sizeof(float),
                               hipMemcpyDeviceToHost, s));
    if (iters_run)
        HIP_TRY(hipMemcpyAsync(iters_run, p->iters_run(), (size_t)p->B * p->L * sizeof(int),
                               hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return OFLK_OK;
}

namespace {

// np.mean(np.abs(d)) of a device plane in NumPy's own summation order (k_np_abs_piece_sums + the serial
// addition of the pieces, here on the host in fp32; this translation unit is built with -ffp-contract=off)
int np_mean_abs(oflk_plan *p, const float *d, size_t n, hipStream_t s, float *mean)
{
    const size_t pieces = (n + kNpPiece - 1) / kNpPiece;
    hipLaunchKernelGGL(k_np_abs_piece_sums, dim3((unsigned)((pieces + 63) / 64)), dim3(64), 0, s, d, n, p->exact.pieces);
    HIP_TRY(hipGetLastError());
    std::vector<float> h(pieces);
    HIP_TRY(hipMemcpyAsync(h.data(), p->exact.pieces, pieces * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    volatile float acc = 0.0f;   // every add rounded to fp32, in order
    for (size_t i = 0; i < pieces; i++) acc = acc + h[i];
    *mean = (float)((double)acc / (double)n);
    return OFLK_OK;
}

// One pair, the reference's own sequence of steps (lucas_kanade_pyramidal.py:173-223) with the standalone
// kernels -- pyramid, warp, single-scale LK, flow += d, upsample, all value-identical to the fused path --
// and the exit decision taken on the HOST from NumPy-order means.  Results and log replace pair b's.
int resolve_pair(oflk_plan *p, int b, const void *d_prev_in, const void *d_curr_in, bool u8, float *d_u, float *d_v, hipStream_t s,
                 bool level_out)
{
    const int L = p->L, K = p->K, H = p->H, W = p->W;
    const size_t N = (size_t)H * W;
    oflk_plan::Exact &x = p->exact;
    int rc;
    if ((rc = ensure_dense_ws(p))) return rc;   // the blur temporaries and the level flows' slots
    if (!x.ready) {
        size_t tot = 0;
        for (int l = 0; l < L; l++) {
            const size_t n = p->npix(l);
            if (l < L - 1 && (rc = dmalloc(&x.pyr[l], 2 * n, &tot))) return rc;
            if ((rc = dmalloc(&x.u[l], n, &tot)) || (rc = dmalloc(&x.v[l], n, &tot))) return rc;
        }
        if ((rc = dmalloc(&x.warped, N, &tot)) || (rc = dmalloc(&x.du, N, &tot)) || (rc = dmalloc(&x.dv, N, &tot)) ||
            (rc = dmalloc(&x.f32[0], N, &tot)) || (rc = dmalloc(&x.f32[1], N, &tot)) ||
            (rc = dmalloc(&x.pieces, (N + kNpPiece - 1) / kNpPiece, &tot)))
            return rc;
        p->ws_bytes += tot;
        x.ready = true;
    }
    // the pair's frames as float32 planes
    const float *fp, *fc;
    if (u8) {
        dim3 grid((unsigned)((N + 4095) / 4096));
        hipLaunchKernelGGL(k_u8_to_f32, grid, dim3(256), 0, s, static_cast<const unsigned char *>(d_prev_in) + (size_t)b * N, x.f32[0], N);
        hipLaunchKernelGGL(k_u8_to_f32, grid, dim3(256), 0, s, static_cast<const unsigned char *>(d_curr_in) + (size_t)b * N, x.f32[1], N);
        HIP_TRY(hipGetLastError());
        fp = x.f32[0];
        fc = x.f32[1];
    } else {
        fp = static_cast<const float *>(d_prev_in) + (size_t)b * N;
        fc = static_cast<const float *>(d_curr_in) + (size_t)b * N;
    }
    for (int l = L - 2; l >= 0; l--) {
        const int h = p->dims[2 * (l + 1)], w = p->dims[2 * (l + 1) + 1], ho = p->dims[2 * l], wo = p->dims[2 * l + 1];
        if (l == L - 2) {
            PyrExtra two;
            two.in2 = fc;
            two.nsplit = 1;
            rc = launch_pyr_down(nullptr, p->gauss, s, fp, x.pyr[l], p->tmpA, p->tmpB, 2, h, w, ho, wo, &two);
        } else {
            rc = launch_pyr_down(nullptr, p->gauss, s, x.pyr[l + 1], x.pyr[l], p->tmpA, p->tmpB, 2, h, w, ho, wo);
        }
        if (rc) return rc;
    }
    std::vector<float> log((size_t)L * p->Kc() * 2, 0.0f);
    std::vector<int> runs((size_t)L, 0);
    HIP_TRY(hipMemsetAsync(x.u[0], 0, p->npix(0) * sizeof(float), s));   // flow = zeros at the coarsest level (:182-184)
    HIP_TRY(hipMemsetAsync(x.v[0], 0, p->npix(0) * sizeof(float), s));
    for (int l = 0; l < L; l++) {
        const int h = p->dims[2 * l], w = p->dims[2 * l + 1];
        const size_t n = (size_t)h * w;
        if (l > 0) {
            ResampleArgs r = upsample_args(p->dims[2 * (l - 1)], p->dims[2 * (l - 1) + 1], h, w);
            r.in[0] = x.u[l - 1]; r.in[1] = x.v[l - 1];
            r.out[0] = x.u[l]; r.out[1] = x.v[l];
            if ((rc = launch_upsample(nullptr, s, r, 1))) return rc;
        }
        const float *lp = (l == L - 1) ? fp : x.pyr[l];
        const float *lc = (l == L - 1) ? fc : x.pyr[l] + n;
        for (int k = 0; k < K; k++) {
            hipLaunchKernelGGL(k_warp, grid2d(w, h, 1), dim3(256), 0, s, lc, (const float *)x.u[l], (const float *)x.v[l], x.warped, h, w);
            HIP_TRY(hipGetLastError());
            LkArgs a{};
            a.prev = lp; a.curr = x.warped;
            a.ou = x.du; a.ov = x.dv;
            a.H = h; a.W = w;
            if ((rc = launch_lk<MODE_SINGLE>(nullptr, s, KC_LK_SINGLE, p->hw, a, 1))) return rc;
            hipLaunchKernelGGL(k_flow_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x.u[l], x.v[l], (const float *)x.du,
                               (const float *)x.dv, n);
            HIP_TRY(hipGetLastError());
            float mu, mv;
            if ((rc = np_mean_abs(p, x.du, n, s, &mu)) || (rc = np_mean_abs(p, x.dv, n, s, &mv))) return rc;
            log[((size_t)l * p->Kc() + k) * 2] = mu;
            log[((size_t)l * p->Kc() + k) * 2 + 1] = mv;
            runs[(size_t)l] = k + 1;
            if (mu < 0.01f && mv < 0.01f) break;   // :221-223
        }
    }
    HIP_TRY(hipMemcpyAsync(d_u + (size_t)b * N, x.u[L - 1], N * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_v + (size_t)b * N, x.v[L - 1], N * sizeof(float), hipMemcpyDeviceToDevice, s));
    // the coarser levels' final flows where oflk_plan_read_level_flow looks for them: the interleaved slot the
    // (new) iteration count of the level selects (strided copies: u into the .x, v into the .y of every float2)
    for (int l = 0; level_out && l < L - 1; l++) {
        const size_t n = p->npix(l);
        float *dst = reinterpret_cast<float *>(p->fl(l, runs[(size_t)l] & 1) + (size_t)b * n);
        HIP_TRY(hipMemcpy2DAsync(dst, sizeof(float2), x.u[l], sizeof(float), sizeof(float), n, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpy2DAsync(dst + 1, sizeof(float2), x.v[l], sizeof(float), sizeof(float), n, hipMemcpyDeviceToDevice, s));
    }
    // the pair's log, iteration counts and (cleared) flags in the plan's state, where read_log looks
    HIP_TRY(hipMemcpyAsync(p->log() + (size_t)b * L * p->Kc() * 2, log.data(), log.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->iters_run() + (size_t)b * L, runs.data(), runs.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(p->uncertain() + (size_t)b * L, 0, (size_t)L * sizeof(int), s));
    HIP_TRY(hipStreamSynchronize(s));   // log / runs are host vectors
    return OFLK_OK;
}

int resolve_uncertain(oflk_plan *p, const void *d_prev, const void *d_curr, bool u8, float *d_u, float *d_v, hipStream_t s,
                      int *resolved, bool level_out = true)
{
    if (!p || !d_prev || !d_curr || !d_u || !d_v) return fail(OFLK_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    std::vector<int> flags((size_t)p->B * p->L);
    HIP_TRY(hipMemcpyAsync(flags.data(), p->uncertain(), flags.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int n = 0;
    for (int b = 0; b < p->B; b++) {
        bool any = false;
        for (int l = 0; l < p->L; l++) any = any || flags[(size_t)b * p->L + l] != 0;
        if (!any) continue;
        int rc = resolve_pair(p, b, d_prev, d_curr, u8, d_u, d_v, s, level_out);
        if (rc) return rc;
        n++;
    }
    if (resolved) *resolved = n;
    return OFLK_OK;
}

// both directions of a bidirectional sequence pass; the level flows stay the backward pass's
int resolve_uncertain_fb(oflk_plan *p, const void *d_frames, bool u8, float *d_uf, float *d_vf, float *d_ub, float *d_vb,
                         hipStream_t s, int *resolved)
{
    if (!p || !d_frames || !d_uf || !d_vf || !d_ub || !d_vb) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (!p->state_b) return fail(OFLK_ERR_INVALID, "the plan has run no bidirectional pass");
    const void *d_next = static_cast<const char *>(d_frames) + (size_t)p->H * p->W * (u8 ? 1 : sizeof(float));
    int nf = 0, nb = 0, rc;
    if ((rc = resolve_uncertain(p, d_frames, d_next, u8, d_uf, d_vf, s, &nf, !p->last_fb))) return rc;
    {
        StateSwap sw(p, true);
        if ((rc = resolve_uncertain(p, d_next, d_frames, u8, d_ub, d_vb, s, &nb))) return rc;
    }
    if (resolved) *resolved = nf + nb;
    return OFLK_OK;
}

}  // namespace

OFLK_API int oflk_plan_resolve_uncertain(oflk_plan *p, const float *d_prev, const float *d_curr, float *d_u, float *d_v,
                                         void *stream, int *resolved)
{
    return resolve_uncertain(p, d_prev, d_curr, false, d_u, d_v, (hipStream_t)stream, resolved);
}

OFLK_API int oflk_plan_resolve_uncertain_u8(oflk_plan *p, const unsigned char *d_prev, const unsigned char *d_curr, float *d_u,
                                            float *d_v, void *stream, int *resolved)
{
    return resolve_uncertain(p, d_prev, d_curr, true, d_u, d_v, (hipStream_t)stream, resolved);
}

OFLK_API int oflk_plan_resolve_uncertain_sequence_fb(oflk_plan *p, const float *d_frames, float *d_uf, float *d_vf, float *d_ub,
                                                     float *d_vb, void *stream, int *resolved)
{
    return resolve_uncertain_fb(p, d_frames, false, d_uf, d_vf, d_ub, d_vb, (hipStream_t)stream, resolved);
}

OFLK_API int oflk_plan_resolve_uncertain_sequence_fb_u8(oflk_plan *p, const unsigned char *d_frames, float *d_uf, float *d_vf,
                                                        float *d_ub, float *d_vb, void *stream, int *resolved)
{
    return resolve_uncertain_fb(p, d_frames, true, d_uf, d_vf, d_ub, d_vb, (hipStream_t)stream, resolved);
}

OFLK_API int oflk_last_resolved(void) { return t_resolved; }

OFLK_API int oflk_plan_read_uncertain(oflk_plan *p, int *uncertain, void *stream)
{
    if (!p || !uncertain) return fail(OFLK_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(uncertain, p->uncertain(), (size_t)p->B * p->L * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return OFLK_OK;
}

OFLK_API int oflk_plan_read_log_backward(oflk_plan *p, float *residual_log, int *iters_run, void *stream)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    if (!p->state_b) return fail(OFLK_ERR_INVALID, "the plan has run no bidirectional pass");
    StateSwap sw(p, true);
    return oflk_plan_read_log(p, residual_log, iters_run, stream);
}

OFLK_API int oflk_plan_read_uncertain_backward(oflk_plan *p, int *uncertain, void *stream)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    if (!p->state_b) return fail(OFLK_ERR_INVALID, "the plan has run no bidirectional pass");
    StateSwap sw(p, true);
    return oflk_plan_read_uncertain(p, uncertain, stream);
}

OFLK_API int oflk_plan_read_level_flow(oflk_plan *p, int level, int pair, float *u, float *v, void *stream)
{
    if (!p || !u || !v) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (level < 0 || level >= p->L - 1)
        return fail(OFLK_ERR_INVALID, "level must be in [0,%d): the finest level's flow is the call's result", p->L - 1);
    if (pair < 0 || pair >= p->B) return fail(OFLK_ERR_INVALID, "pair %d out of range [0,%d)", pair, p->B);
    HIP_TRY(hipSetDevice(p->device));
    if (!p->flow[level]) return fail(OFLK_ERR_INVALID, "no pyramidal pass has run on this plan yet");
    hipStream_t s = (hipStream_t)stream;
    StateSwap sw(p, p->last_fb);   // after a bidirectional pass the slots hold the backward flows
    int executed = 0;
    HIP_TRY(hipMemcpyAsync(&executed, p->iters_run() + (size_t)pair * p->L + level, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int slot = executed & 1;   // the ping-pong slot the level's last executed iteration wrote
    const size_t n = p->npix(level);
    std::vector<float2> both(n);
    HIP_TRY(hipMemcpyAsync(both.data(), p->fl(level, slot) + (size_t)pair * n, n * sizeof(float2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) {   // de-interleave on the host (a debugging / plotting path)
        u[i] = both[i].x;
        v[i] = both[i].y;
    }
    return OFLK_OK;
}

namespace {
int check_arith(int mode)
{
    if (mode != OFLK_ARITH_EXACT && mode != OFLK_ARITH_CONTRACTED && mode != OFLK_ARITH_TOLERANT)
        return fail(OFLK_ERR_INVALID, "arithmetic mode must be OFLK_ARITH_EXACT (0), OFLK_ARITH_CONTRACTED (1) or OFLK_ARITH_TOLERANT (2), got %d", mode);
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_plan_set_arithmetic(oflk_plan *p, int mode)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    if (int rc = check_arith(mode)) return rc;
    p->arith = mode;
    return OFLK_OK;
}

OFLK_API int oflk_set_host_arithmetic(int mode)
{
    if (int rc = check_arith(mode)) return rc;
    g_host_arith.store(mode);
    return OFLK_OK;
}

OFLK_API int oflk_tolerant_relaxes(int levels, int window_size, int iterations)
{
    return window_size >= 1 && tolerant_relaxes(levels, window_size / 2, iterations) ? 1 : 0;
}

OFLK_API int oflk_upsample_staged(int Hc, int Wc, int Ht, int Wt)
{
    return Hc >= 1 && Wc >= 1 && Ht >= 1 && Wt >= 1 && upsample_fits(Hc, Wc, Ht, Wt) ? 1 : 0;
}

OFLK_API int oflk_pyramid_step_fused(int h, int w, int ho, int wo, int radius)
{
    if (h < 1 || w < 1 || ho < 1 || wo < 1) return 0;
    GaussW g{};
    g.radius = radius;   // the only field of the weights that the decision reads
    return pyr_fused_fits(h, w, ho, wo, g) ? 1 : 0;
}

OFLK_API int oflk_pyramid_step_form(int h, int w, int ho, int wo, int radius)
{
    if (h < 1 || w < 1 || ho < 1 || wo < 1) return 0;
    GaussW g{};
    g.radius = radius;
    return pyr_form(h, w, ho, wo, g);
}

OFLK_API int oflk_pyramid_step_half(int h, int w, int ho, int wo, int radius)
{
    if (h < 1 || w < 1 || ho < 1 || wo < 1) return 0;
    GaussW g{};
    g.radius = radius;
    return pyr_half(h, w, ho, wo, g) ? 1 : 0;
}

OFLK_API double oflk_device_mean_error(int path, int level_h, int level_w, double mean)
{
    return device_mean_error(path, level_h, level_w, mean);
}

OFLK_API double oflk_decision_guard(int path, int level_h, int level_w)
{
    return decision_guard(path, level_h, level_w);
}

OFLK_API int oflk_multi_rehearsal(int workers)
{
    if (workers < 0 || workers > 64) return fail(OFLK_ERR_INVALID, "workers must be 0 ... 64, got %d", workers);
    g_multi_workers.store(workers);
    return OFLK_OK;
}

OFLK_API int oflk_plan_set_kernels(oflk_plan *p, int choice)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    if (choice != OFLK_KERNELS_AUTO && choice != OFLK_KERNELS_TILE && choice != OFLK_KERNELS_STREAM)
        return fail(OFLK_ERR_INVALID, "kernel choice must be OFLK_KERNELS_AUTO (0), OFLK_KERNELS_TILE (1) or OFLK_KERNELS_STREAM (2), got %d", choice);
    p->kernels = choice;
    return OFLK_OK;
}

OFLK_API int oflk_plan_set_profiling(oflk_plan *p, int enabled)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    p->prof = enabled != 0;
    p->prof_only = enabled == 2 ? KC_LK_ITER_FINEST : -1;  // 2: only the dominant kernel
    for (auto &e : p->pending) p->pool.push_back({e.a, e.b});
    p->pending.clear();
    for (int i = 0; i < KC_COUNT; i++) {
        p->acc_ms[i] = 0;
        p->acc_n[i] = 0;
    }
    return OFLK_OK;
}

OFLK_API int oflk_plan_kernel_times(oflk_plan *p, const char **names, double *total_ms,
                                    long *launches, int max_entries)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    for (auto &e : p->pending) {
        HIP_TRY(hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        p->acc_ms[e.cls] += ms;
        p->acc_n[e.cls] += 1;
        p->pool.push_back({e.a, e.b});
    }
    p->pending.clear();
    int n = std::min<int>(KC_COUNT, max_entries);
    for (int i = 0; i < n; i++) {
        if (names) names[i] = kClassNames[i];
        if (total_ms) total_ms[i] = p->acc_ms[i];
        if (launches) launches[i] = p->acc_n[i];
    }
    return n;
}

// =============================================================================
// host-pointer entry points
// =============================================================================
namespace {

struct Arena {
    std::vector<void *> blocks;
    ~Arena() { release(); }
    void release()
    {
        for (void *b : blocks) (void)hipFree(b);
        blocks.clear();
    }
    template <typename T>
    int get(T **p, size_t n)
    {
        size_t tot = 0;
        int rc = dmalloc(p, n, &tot);
        if (!rc) blocks.push_back(*p);
        return rc;
    }
};

// Per-device state of the host entry points: a small cache of plans keyed by shape (the verifier
// alternates single-scale and pyramidal calls of one size; a caller may mix a few sizes) and the
// device buffers the frames and flows are staged in.  Everything in a context lives on ITS device,
// so switching devices (oflk_set_device, the multi-GPU entry points) never mixes allocations.
constexpr int kMaxDevices = 64;
constexpr size_t kPlanCache = 6;

struct HostCtx {
    std::mutex mu;   // one host call at a time per device; different devices run concurrently
    std::vector<oflk_plan *> plans;                          // most recently used first
    float *io[4] = {nullptr, nullptr, nullptr, nullptr};    // device prev, curr, u, v
    size_t io_elems = 0;
    unsigned char *u8[2] = {nullptr, nullptr};              // device uint8 frames
    size_t u8_elems = 0;
    // chunked host calls (run_batch_chunked): two slots of chunk-sized frames in / flow out, three streams
    unsigned char *ring_in[4] = {nullptr, nullptr, nullptr, nullptr};   // [2 * slot + (prev, curr)], PIXELS
    float *ring_out[4] = {nullptr, nullptr, nullptr, nullptr};          // [2 * slot + (u, v)]
    size_t ring_in_bytes = 0, ring_out_elems = 0;
    hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
};
HostCtx g_ctx[kMaxDevices];

// One host-pointer call: the lock on the context of its device, the device made current for the calling thread, and the
// call's own device buffers, freed before the lock is released.  Everything is staged on the null stream; sync() is the
// last step of a call, so that the caller's arrays are complete when it returns.
class HostCall {
  public:
    HostCtx *c = nullptr;
    int dev = -1;

    int begin(int device = g_device.load())
    {
        if (device < 0 || device >= kMaxDevices) return fail(OFLK_ERR_INVALID, "device %d out of range", device);
        lk = std::unique_lock<std::mutex>(g_ctx[device].mu);
        int rc = ensure_device(device);
        if (rc) return rc;
        c = &g_ctx[device];
        dev = device;
        return OFLK_OK;
    }
    // a buffer of n elements for this call; none (NULL) when `want` is false, for an output the caller did not ask for
    template <typename T>
    int alloc(T **d, size_t n, bool want = true)
    {
        *d = nullptr;
        return want ? ar.get(d, n) : OFLK_OK;
    }
    template <typename T>
    int upload(T **d, const T *host, size_t n)
    {
        int rc = ar.get(d, n);
        return rc ? rc : to_device(*d, host, n);
    }
    template <typename T>
    int to_device(T *d, const T *host, size_t n)
    {
        HIP_TRY(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, nullptr));
        return OFLK_OK;
    }
    template <typename T>
    int to_host(T *host, const T *d, size_t n)
    {
        HIP_TRY(hipMemcpyAsync(host, d, n * sizeof(T), hipMemcpyDeviceToHost, nullptr));
        return OFLK_OK;
    }
    int sync()
    {
        HIP_TRY(hipStreamSynchronize(nullptr));
        return OFLK_OK;
    }

  private:
    std::unique_lock<std::mutex> lk;   // declared before ar: destroyed after it
    Arena ar;
};

bool has_shape(const oflk_plan *q, int B, int H, int W, int L, int win, int K)
{
    return q->B == B && q->H == H && q->W == W && q->L == L && q->win == win && q->K == K;
}

int host_plan(HostCtx &c, int dev, int B, int H, int W, int L, int win, int K, oflk_plan **out)
{
    for (size_t i = 0; i < c.plans.size(); i++) {
        oflk_plan *q = c.plans[i];
        if (has_shape(q, B, H, W, L, win, K)) {
            c.plans.erase(c.plans.begin() + (long)i);
            c.plans.insert(c.plans.begin(), q);
            q->arith = g_host_arith.load();
            *out = q;
            return OFLK_OK;
        }
    }
    oflk_plan *q = nullptr;
    int rc = oflk_plan_create(&q, dev, B, H, W, L, win, K);
    if (rc == OFLK_ERR_NOMEM && !c.plans.empty()) {
        // make room: drop every cached plan and try once more
        for (oflk_plan *old : c.plans) plan_free(old);
        c.plans.clear();
        rc = oflk_plan_create(&q, dev, B, H, W, L, win, K);
    }
    if (rc) return rc;
    q->arith = g_host_arith.load();
    c.plans.insert(c.plans.begin(), q);
    while (c.plans.size() > kPlanCache) {
        plan_free(c.plans.back());
        c.plans.pop_back();
    }
    *out = q;
    return OFLK_OK;
}

// the cached plan of an earlier host call of this shape on the current device (not created here)
int cached_plan(HostCtx &c, int B, int H, int W, int L, int win, int K, oflk_plan **out)
{
    for (oflk_plan *q : c.plans)
        if (has_shape(q, B, H, W, L, win, K)) {
            *out = q;
            return OFLK_OK;
        }
    return fail(OFLK_ERR_INVALID, "no pyramidal call of this shape (B=%d, %dx%d, %d levels, window %d, %d iterations) "
                                  "has run on this device yet", B, W, H, L, win, K);
}

// A set of cached device buffers of `have` elements each, grown to `need`: all freed, then all allocated again
template <typename T, size_t N>
int grow(T *(&set)[N], size_t &have, size_t need)
{
    if (need <= have) return OFLK_OK;
    for (T *&q : set) {
        if (q) (void)hipFree(q);
        q = nullptr;
    }
    have = 0;
    size_t tot = 0;
    for (T *&q : set) {
        int rc = dmalloc(&q, need, &tot);
        if (rc) return rc;
    }
    have = need;
    return OFLK_OK;
}

int host_ring(HostCtx &c, size_t in_bytes, size_t out_elems)
{
    // each stream on its own: a call that failed half-way here must not leave a later one on the null (blocking) stream
    for (hipStream_t *st : {&c.s_in, &c.s_comp, &c.s_out}) {
        if (*st) continue;
        hipError_t e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
        if (e != hipSuccess) {
            *st = nullptr;
            return fail(OFLK_ERR_HIP, "hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
        }
    }
    int rc = grow(c.ring_in, c.ring_in_bytes, in_bytes);
    return rc ? rc : grow(c.ring_out, c.ring_out_elems, out_elems);
}

// Pairs per chunk of a chunked host call: ~32 MB of flow per plane (four 1080p pairs, one 4K pair), worth it from four chunks
// on.  Below B exactly when the call is chunked (B: the whole batch in one piece).
int chunk_pairs(int B, int H, int W)
{
    const size_t pair_out = (size_t)H * W * sizeof(float);
    const int C = (int)std::max<size_t>(1, ((size_t)32 << 20) / std::max<size_t>(pair_out, 1));
    return B >= 4 * C && (size_t)B * pair_out >= ((size_t)64 << 20) ? C : B;
}

int check_hw(const void *a, const void *b, int H, int W)
{
    if (!a || !b) return fail(OFLK_ERR_INVALID, "NULL array argument");
    if (H < 1 || W < 1) return fail(OFLK_ERR_INVALID, "H and W must be >= 1 (got %d x %d)", H, W);
    if ((size_t)H * (size_t)W >= ((size_t)1 << 30))
        return fail(OFLK_ERR_UNSUPPORTED, "frames of 2^30 pixels or more are not supported");  // 32-bit byte offsets
    if (H >= kMaxDim || W >= kMaxDim)
        return fail(OFLK_ERR_UNSUPPORTED, "frames of 2^23 rows or columns or more are not supported (got %d x %d)", H, W);
    return OFLK_OK;
}

// A large host batch in chunks, so that the PCIe link works in both directions while the GPU computes:
//   main thread    H2D(k+1) on s_in   |  kernels(k) on s_comp  |  (exit decisions, log of chunk k)
//   second thread                         D2H(k-1) on s_out
// Two slots of chunk-sized device buffers; a chunk's inputs wait for the kernels two chunks back, its kernels for
// the D2H two chunks back.  The callers' arrays are ordinary pageable memory: a copy from / to them holds its host
// thread until it is done, which is why the two directions have a thread each.  Frame pairs are independent, so
// the results do not depend on the cut (tests/test_gpu_round3.py).  A synchronous float32 call moves 33 MB per
// 1080p pair over the link, half of it each way: overlapped, the floor is one direction's time.
// seq: a frame sequence (curr == prev + one plane); a chunk of C pairs takes its C+1 frames into one slot buffer, so the
// frame on the boundary of two chunks is uploaded by both.
template <class PIXELS>
int run_batch_chunked(HostCtx *c, int dev, const PIXELS *prev, const PIXELS *curr, int B, int C, int H, int W, int levels,
                      int window_size, int iters, float *u, float *v, float *residual_log, int *iters_run, bool seq = false)
{
    constexpr bool U8 = sizeof(PIXELS) == 1;
    const bool single = levels == 0;
    const int Lp = single ? 1 : levels, Kp = single ? 0 : iters;
    const int Lc = std::max(levels, 1), Kc = std::max(iters, 1);
    const size_t plane = (size_t)H * W;
    const int nchunk = (B + C - 1) / C;
    int rc;
    if ((rc = host_ring(*c, (size_t)(seq ? C + 1 : C) * plane * sizeof(PIXELS), (size_t)C * plane))) return rc;
    oflk_plan *pc = nullptr, *pt = nullptr;
    if ((rc = host_plan(*c, dev, C, H, W, Lp, window_size, Kp, &pc))) return rc;
    const int tail = B - (nchunk - 1) * C;
    if (tail != C) {
        // Both plans must be alive at once.  A lookup that runs out of device memory frees EVERY cached plan (host_plan), the
        // other one of this pair included, so after the second lookup the first is looked up again and both are checked
        // against the cache; if the two do not fit the device together the batch cannot run chunked.
        if ((rc = host_plan(*c, dev, tail, H, W, Lp, window_size, Kp, &pt))) return rc;
        if ((rc = host_plan(*c, dev, C, H, W, Lp, window_size, Kp, &pc))) return rc;
        auto cached = [&](const oflk_plan *q) { return std::find(c->plans.begin(), c->plans.end(), q) != c->plans.end(); };
        if (!cached(pc) || !cached(pt))
            return fail(OFLK_ERR_NOMEM, "the chunk plan (%d pairs) and the tail plan (%d pairs) of %dx%d do not fit the device together", C, tail, W, H);
    }

    hipEvent_t ev_in[2] = {nullptr, nullptr};   // a slot's frames have arrived
    for (int i = 0; i < 2; i++) {
        if (hipEventCreateWithFlags(&ev_in[i], hipEventDisableTiming) != hipSuccess) {
            if (ev_in[0]) (void)hipEventDestroy(ev_in[0]);
            return fail(OFLK_ERR_HIP, "hipEventCreate");
        }
    }
    // hand-over to the D2H thread: chunks [0, computed) are ready to leave, chunks [0, copied) have left
    std::mutex mu;
    std::condition_variable cv;
    int computed = 0, copied = 0, out_rc = OFLK_OK;
    bool stop = false;
    std::string out_msg;
    std::thread out_thread;
    auto out_body = [&]() {
        if (ensure_device(dev)) { std::lock_guard<std::mutex> g(mu); out_rc = OFLK_ERR_HIP; out_msg = t_err; cv.notify_all(); return; }
        for (int k = 0; k < nchunk; k++) {
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return computed > k || stop; });
                if (computed <= k) return;
            }
            const int slot = k & 1, nb = k == nchunk - 1 ? tail : C;
            const size_t off = (size_t)k * C * plane, bytes = (size_t)nb * plane * sizeof(float);
            hipError_t e = hipMemcpyAsync(u + off, c->ring_out[2 * slot], bytes, hipMemcpyDeviceToHost, c->s_out);
            if (e == hipSuccess) e = hipMemcpyAsync(v + off, c->ring_out[2 * slot + 1], bytes, hipMemcpyDeviceToHost, c->s_out);
            if (e == hipSuccess) e = hipStreamSynchronize(c->s_out);
            std::lock_guard<std::mutex> g(mu);
            if (e != hipSuccess) {
                out_rc = OFLK_ERR_HIP;
                out_msg = std::string("D2H of a chunk: ") + hipGetErrorString(e);
                cv.notify_all();
                return;
            }
            copied = k + 1;
            cv.notify_all();
        }
    };
    try {
        out_thread = std::thread(out_body);
    } catch (...) {   // no exception leaves the C ABI
        for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev_in[i]);
        return fail(OFLK_ERR_HIP, "could not start the D2H thread of a chunked batch");
    }
    auto finish = [&](int code) {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
        }
        cv.notify_all();
        out_thread.join();
        if (code != OFLK_OK || out_rc != OFLK_OK) {
            // an abandoned batch may still have copies and kernels in flight on the ring buffers: the next call reuses them
            (void)hipStreamSynchronize(c->s_in);
            (void)hipStreamSynchronize(c->s_comp);
            (void)hipStreamSynchronize(c->s_out);
        }
        for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev_in[i]);
        if (code == OFLK_OK && out_rc != OFLK_OK) return fail(out_rc, "%s", out_msg.c_str());
        return code;
    };
    auto h2d = [&](int k) -> int {
        const int slot = k & 1, nb = k == nchunk - 1 ? tail : C;
        const size_t off = (size_t)k * C * plane, bytes = (size_t)nb * plane * sizeof(PIXELS);
        if (seq) {
            HIP_TRY(hipMemcpyAsync(c->ring_in[2 * slot], prev + off, bytes + plane * sizeof(PIXELS), hipMemcpyHostToDevice, c->s_in));
        } else {
            HIP_TRY(hipMemcpyAsync(c->ring_in[2 * slot], prev + off, bytes, hipMemcpyHostToDevice, c->s_in));
            HIP_TRY(hipMemcpyAsync(c->ring_in[2 * slot + 1], curr + off, bytes, hipMemcpyHostToDevice, c->s_in));
        }
        HIP_TRY(hipEventRecord(ev_in[slot], c->s_in));
        return OFLK_OK;
    };
    int resolved_total = 0;
    if ((rc = h2d(0))) return finish(rc);
    for (int k = 0; k < nchunk; k++) {
        const int slot = k & 1, nb = k == nchunk - 1 ? tail : C;
        oflk_plan *p = nb == C ? pc : pt;
        if (k >= 2) {   // the slot's flow buffers are free once chunk k-2 has left
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return copied >= k - 1 || out_rc != OFLK_OK; });
            if (out_rc != OFLK_OK) { g.unlock(); return finish(OFLK_OK); }
        }
        if ((rc = hipStreamWaitEvent(c->s_comp, ev_in[slot], 0)) != hipSuccess) return finish(fail(OFLK_ERR_HIP, "hipStreamWaitEvent"));
        const void *dp = c->ring_in[2 * slot];
        const void *dc = seq ? static_cast<const void *>(static_cast<const PIXELS *>(dp) + plane) : c->ring_in[2 * slot + 1];
        float *du = c->ring_out[2 * slot], *dv = c->ring_out[2 * slot + 1];
        rc = single ? plan_single_scale(p, dp, dc, U8, du, dv, c->s_comp) : plan_pyramidal(p, dp, dc, U8, du, dv, c->s_comp, seq);
        if (rc) return finish(rc);
        // the next chunk's frames travel while this one is computed (the kernels that read its slot, chunk k-1's, are done:
        // the previous turn of this loop ended by waiting for them)
        if (k + 1 < nchunk && (rc = h2d(k + 1))) return finish(rc);
        if (!single && iters > 0) {
            int n = 0;
            if ((rc = resolve_uncertain(p, dp, dc, U8, du, dv, c->s_comp, &n))) return finish(rc);
            resolved_total += n;
        }
        if (single) {
            if (hipStreamSynchronize(c->s_comp) != hipSuccess) return finish(fail(OFLK_ERR_HIP, "hipStreamSynchronize"));
        } else {
            rc = oflk_plan_read_log(p, residual_log ? residual_log + (size_t)k * C * Lc * Kc * 2 : nullptr,
                                    iters_run ? iters_run + (size_t)k * C * Lc : nullptr, c->s_comp);
            if (rc) return finish(rc);
        }
        {
            std::lock_guard<std::mutex> g(mu);
            computed = k + 1;
        }
        cv.notify_all();
    }
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return copied >= nchunk || out_rc != OFLK_OK; });
    }
    t_resolved += resolved_total;
    return finish(OFLK_OK);
}

// One batch on one device, host pointers in and out.  PIXELS: float or unsigned char frames (the
// uint8 kernels read the frames as they are: no float32 copy of them exists on the device).
// levels == 0 selects single-scale.  seq: prev holds a sequence of B+1 frames and curr == prev + one plane (each frame is
// uploaded once, and a pyramidal pass builds each frame's pyramid once).
template <class PIXELS>
int run_batch_on(int dev, const PIXELS *prev, const PIXELS *curr, int B, int H, int W, int levels, int window_size,
                 int iters, float *u, float *v, float *residual_log, int *iters_run, bool seq = false)
{
    constexpr bool U8 = sizeof(PIXELS) == 1;
    t_resolved = 0;   // of THIS call (oflk_last_resolved)
    int rc = check_hw(prev, curr, H, W);
    if (rc) return rc;
    if (!u || !v) return fail(OFLK_ERR_INVALID, "NULL output");
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1");
    HostCall call;
    if ((rc = call.begin(dev))) return rc;
    HostCtx *c = call.c;
    const bool single = levels == 0;
    const int C = chunk_pairs(B, H, W);
    if (C < B)
        return run_batch_chunked<PIXELS>(c, dev, prev, curr, B, C, H, W, levels, window_size, iters, u, v, residual_log, iters_run,
                                         seq);
    oflk_plan *p = nullptr;
    if ((rc = host_plan(*c, dev, B, H, W, single ? 1 : levels, window_size, single ? 0 : iters, &p))) return rc;
    const size_t plane = (size_t)H * W, n = (size_t)B * plane;
    const size_t nin = seq ? n + plane : n;   // frames in the first device buffer (a sequence: all B+1)
    if ((rc = grow(c->io, c->io_elems, nin))) return rc;
    PIXELS **in = nullptr;   // the context's frame buffers of this pixel type
    if constexpr (U8) {
        if ((rc = grow(c->u8, c->u8_elems, nin))) return rc;
        in = c->u8;
    } else {
        in = c->io;
    }
    if ((rc = call.to_device(in[0], prev, nin)) || (!seq && (rc = call.to_device(in[1], curr, n)))) return rc;
    const void *dp = in[0], *dc = seq ? in[0] + plane : in[1];
    rc = single ? plan_single_scale(p, dp, dc, U8, c->io[2], c->io[3], nullptr)
                : plan_pyramidal(p, dp, dc, U8, c->io[2], c->io[3], nullptr, seq);
    if (rc) return rc;
    // exit decisions the device could not take with certainty are redone in NumPy's own summation order
    if (!single && iters > 0) {
        int n_res = 0;
        if ((rc = resolve_uncertain(p, dp, dc, U8, c->io[2], c->io[3], nullptr, &n_res))) return rc;
        t_resolved += n_res;
    }
    if ((rc = call.to_host(u, c->io[2], n)) || (rc = call.to_host(v, c->io[3], n))) return rc;
    return single ? call.sync() : oflk_plan_read_log(p, residual_log, iters_run, nullptr);   // the log's read syncs too
}

// contiguous share of `total` units for shard `i` of `n`; sizes differ by at most one
// (the rule of optical-flow-fpga_amd/python/oflk_dist.py shard_range)
void shard_range(int total, int i, int n, int *begin, int *end)
{
    const int base = total / n, extra = total % n;
    *begin = i * base + std::min(i, extra);
    *end = *begin + base + (i < extra ? 1 : 0);
}

// Frame pairs are independent units (lucas_kanade_pyramidal.py:141-228 touches only its two inputs), and how long one
// takes depends on its data (the early exit of :221-223 ends a level after one iteration or after all of them), so the
// devices do not get fixed shards: the batch is cut into chunks of consecutive pairs and every device's host thread pulls
// the next chunk from a shared counter until none is left -- a device whose pairs converge early simply takes more chunks.
// No data crosses between devices, and a pair's result does not depend on which device computed it or in which chunk.
// seq: a sequence (curr == prev + one plane); the chunk of pairs [b0, b1) reads frames [b0, b1].
template <class PIXELS>
int run_batch_multi(const PIXELS *prev, const PIXELS *curr, int B, int H, int W, int levels, int window_size, int iters,
                    int n_gpus, float *u, float *v, float *residual_log, int *iters_run, bool seq = false)
{
    int rc = check_hw(prev, curr, H, W);
    if (rc) return rc;
    if (!u || !v) return fail(OFLK_ERR_INVALID, "NULL output");
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1");
    const int ndev = oflk_device_count();
    if (ndev < 1) return fail(OFLK_ERR_NO_DEVICE, "no usable HIP device; liboflk has no CPU path");
    if (n_gpus <= 0) n_gpus = ndev;
    if (n_gpus > ndev) return fail(OFLK_ERR_INVALID, "n_gpus = %d but %d device(s) visible", n_gpus, ndev);
    const int rehearsal = g_multi_workers.load();
    int workers_n = rehearsal > 0 ? rehearsal : n_gpus;
    workers_n = std::min(workers_n, B);   // never more workers than pairs
    if (workers_n == 1)
        return run_batch_on<PIXELS>(g_device.load(), prev, curr, B, H, W, levels, window_size, iters, u, v, residual_log,
                                    iters_run, seq);
    const size_t plane = (size_t)H * W;
    const int Lc = std::max(levels, 1), Kc = std::max(iters, 1);
    // chunks: about four per worker, so that the last ones even out what the data made uneven; at least one pair
    const int chunk = std::max(1, (B + 4 * workers_n - 1) / (4 * workers_n));
    std::atomic<int> next{0};
    std::vector<int> codes((size_t)workers_n, OFLK_OK), redone((size_t)workers_n, 0);
    std::vector<std::string> msgs((size_t)workers_n);
    std::atomic<bool> failed{false};
    std::vector<std::thread> workers;
    for (int g = 0; g < workers_n; g++) {
        workers.emplace_back([&, g]() {
            const int dev = g % n_gpus;
            while (!failed.load()) {
                const int b0 = next.fetch_add(chunk);
                if (b0 >= B) break;
                const int b1 = std::min(b0 + chunk, B);
                const size_t off = (size_t)b0 * plane;
                const int c = run_batch_on<PIXELS>(dev, prev + off, curr + off, b1 - b0, H, W, levels, window_size, iters,
                                                   u + off, v + off,
                                                   residual_log ? residual_log + (size_t)b0 * Lc * Kc * 2 : nullptr,
                                                   iters_run ? iters_run + (size_t)b0 * Lc : nullptr, seq);
                redone[(size_t)g] += t_resolved;                  // the worker's count of pairs redone
                if (c) {
                    codes[(size_t)g] = c;
                    msgs[(size_t)g] = t_err;                      // the worker's thread-local message
                    failed.store(true);                           // the others stop after their current chunk
                    break;
                }
            }
        });
    }
    for (auto &w : workers) w.join();
    t_resolved = 0;
    for (int g = 0; g < workers_n; g++) t_resolved += redone[(size_t)g];
    for (int g = 0; g < workers_n; g++)
        if (codes[(size_t)g]) return fail(codes[(size_t)g], "device %d: %s", g % n_gpus, msgs[(size_t)g].c_str());
    return OFLK_OK;
}

}  // namespace

OFLK_API int oflk_single_scale_batch(const float *prev, const float *curr, int B, int H, int W,
                                     int window_size, float *u, float *v)
{
    return run_batch_on<float>(g_device.load(), prev, curr, B, H, W, 0, window_size, 0, u, v, nullptr, nullptr);
}

OFLK_API int oflk_single_scale(const float *prev, const float *curr, int H, int W, int window_size,
                               float *u, float *v)
{
    return oflk_single_scale_batch(prev, curr, 1, H, W, window_size, u, v);
}

OFLK_API int oflk_pyramidal_batch(const float *prev, const float *curr, int B, int H, int W,
                                  int levels, int window_size, int iters, float *u, float *v,
                                  float *residual_log, int *iters_run)
{
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_batch_on<float>(g_device.load(), prev, curr, B, H, W, levels, window_size, iters, u, v, residual_log,
                               iters_run);
}

OFLK_API int oflk_pyramidal(const float *prev, const float *curr, int H, int W, int levels,
                            int window_size, int iters, float *u, float *v, float *residual_log,
                            int *iters_run)
{
    return oflk_pyramidal_batch(prev, curr, 1, H, W, levels, window_size, iters, u, v, residual_log,
                                iters_run);
}

// ---- uint8 ingestion: raw 8-bit frames as the reference stores them (frame_0x.bin,
// generate_test_suite.py:259-261).  The kernels read the bytes directly (4 pixels per dword in the
// single-scale staging, byte gathers in the warp): the uint8 -> float32 conversion the verifier
// performs on the host (optical_flow_verifier.py:61-65) happens in registers ------------------
OFLK_API int oflk_single_scale_u8(const unsigned char *prev, const unsigned char *curr, int B, int H, int W,
                                  int window_size, float *u, float *v)
{
    return run_batch_on<unsigned char>(g_device.load(), prev, curr, B, H, W, 0, window_size, 0, u, v, nullptr, nullptr);
}

OFLK_API int oflk_pyramidal_u8(const unsigned char *prev, const unsigned char *curr, int B, int H, int W,
                               int levels, int window_size, int iters, float *u, float *v,
                               float *residual_log, int *iters_run)
{
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_batch_on<unsigned char>(g_device.load(), prev, curr, B, H, W, levels, window_size, iters, u, v,
                                       residual_log, iters_run);
}

OFLK_API int oflk_single_scale_fp16(const float *prev, const float *curr, int B, int H, int W, int window_size,
                                    float pixel_max, float *u, float *v)
{
    int rc = check_hw(prev, curr, H, W);
    if (rc) return rc;
    if (!u || !v) return fail(OFLK_ERR_INVALID, "NULL output");
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1");
    HostCall call;
    if ((rc = call.begin())) return rc;
    HostCtx *c = call.c;
    oflk_plan *p = nullptr;
    if ((rc = host_plan(*c, call.dev, B, H, W, 1, window_size, 0, &p))) return rc;
    const size_t n = (size_t)B * H * W;
    if ((rc = grow(c->io, c->io_elems, n))) return rc;
    if ((rc = call.to_device(c->io[0], prev, n)) || (rc = call.to_device(c->io[1], curr, n))) return rc;
    if ((rc = oflk_plan_single_scale_fp16(p, c->io[0], c->io[1], c->io[2], c->io[3], pixel_max, nullptr))) return rc;
    if ((rc = call.to_host(u, c->io[2], n)) || (rc = call.to_host(v, c->io[3], n))) return rc;
    return call.sync();
}

// ---- RTL-bit-accurate integer mode ---------------------------------
namespace {
int check_rtl(const void *prev, const void *curr, int B, int H, int W, const void *u, const void *v)
{
    if (!prev || !curr || !u || !v) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1");
    if (H < 5 || W < 5) return fail(OFLK_ERR_INVALID, "the RTL's line buffers need H, W >= 5 (got %d x %d)", H, W);
    if (W > kRtlMaxW || H > kRtlMaxH)
        return fail(OFLK_ERR_UNSUPPORTED, "the RTL's coordinate ports are 10 / 9 bits wide: W <= %d, H <= %d (got %d x %d)", kRtlMaxW,
                    kRtlMaxH, W, H);
    return OFLK_OK;
}
}  // namespace

OFLK_API long oflk_rtl_stream_length(int H, int W)
{
    return H < 5 || W < 5 ? 0 : (long)(H - 4) * (long)(W - 4);
}

OFLK_API int oflk_rtl_flow_u8_device(const unsigned char *d_prev, const unsigned char *d_curr, int B, int H, int W, short *d_u,
                                     short *d_v, void *stream)
{
    int rc = check_rtl(d_prev, d_curr, B, H, W, d_u, d_v);
    if (rc) return rc;
    RtlArgs a{};
    a.prev = d_prev; a.curr = d_curr; a.u = d_u; a.v = d_v;
    a.H = H; a.W = W; a.B = B;
    const long M = oflk_rtl_stream_length(H, W);
    dim3 grid((unsigned)((M + kRtlChunk - 1) / kRtlChunk), (unsigned)B);
    const size_t lds = (size_t)(4 * W + kRtlChunk) * sizeof(short4);   // <= 48 KB at W = 1024
    hipLaunchKernelGGL(k_rtl_flow, grid, dim3(256), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

OFLK_API int oflk_rtl_flow_u8(const unsigned char *prev, const unsigned char *curr, int B, int H, int W, short *u, short *v)
{
    int rc = check_rtl(prev, curr, B, H, W, u, v);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    HostCtx *c = call.c;
    const size_t n = (size_t)B * H * W, m = (size_t)B * (size_t)oflk_rtl_stream_length(H, W);
    if ((rc = grow(c->u8, c->u8_elems, n))) return rc;
    if ((rc = grow(c->io, c->io_elems, (m + 1) / 2))) return rc;   // two int16 planes in the float32 scratch planes 2 and 3
    short *d_u = reinterpret_cast<short *>(c->io[2]), *d_v = reinterpret_cast<short *>(c->io[3]);
    if ((rc = call.to_device(c->u8[0], prev, n)) || (rc = call.to_device(c->u8[1], curr, n))) return rc;
    if ((rc = oflk_rtl_flow_u8_device(c->u8[0], c->u8[1], B, H, W, d_u, d_v, nullptr))) return rc;
    if ((rc = call.to_host(u, d_u, m)) || (rc = call.to_host(v, d_v, m))) return rc;
    return call.sync();
}

// ---- one process, several GPUs: the batch sharded over devices 0 .. n_gpus-1 ---------------
OFLK_API int oflk_single_scale_batch_multi(const float *prev, const float *curr, int B, int H, int W,
                                           int window_size, int n_gpus, float *u, float *v)
{
    return run_batch_multi<float>(prev, curr, B, H, W, 0, window_size, 0, n_gpus, u, v, nullptr, nullptr);
}

OFLK_API int oflk_pyramidal_batch_multi(const float *prev, const float *curr, int B, int H, int W, int levels,
                                        int window_size, int iters, int n_gpus, float *u, float *v,
                                        float *residual_log, int *iters_run)
{
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_batch_multi<float>(prev, curr, B, H, W, levels, window_size, iters, n_gpus, u, v, residual_log, iters_run);
}

OFLK_API int oflk_pyramidal_u8_multi(const unsigned char *prev, const unsigned char *curr, int B, int H, int W,
                                     int levels, int window_size, int iters, int n_gpus, float *u, float *v,
                                     float *residual_log, int *iters_run)
{
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_batch_multi<unsigned char>(prev, curr, B, H, W, levels, window_size, iters, n_gpus, u, v, residual_log,
                                          iters_run);
}

// ---- frame sequences: T frames in, the T-1 flows (t -> t+1) out, each frame uploaded once and its pyramid built once -------
namespace {
// n_gpus == 0: the single-device path (oflk_set_device's device); levels == 0: single-scale
template <class PIXELS>
int run_sequence(const PIXELS *frames, int T, int H, int W, int levels, int window_size, int iters, int n_gpus, bool multi,
                 float *u, float *v, float *residual_log, int *iters_run)
{
    int rc = check_hw(frames, frames, H, W);
    if (rc) return rc;
    if (T < 2) return fail(OFLK_ERR_INVALID, "a sequence needs T >= 2 frames (got %d)", T);
    const PIXELS *next = frames + (size_t)H * W;   // pair b is (frames[b], next[b])
    if (multi) return run_batch_multi<PIXELS>(frames, next, T - 1, H, W, levels, window_size, iters, n_gpus, u, v, residual_log,
                                              iters_run, true);
    return run_batch_on<PIXELS>(g_device.load(), frames, next, T - 1, H, W, levels, window_size, iters, u, v, residual_log,
                                iters_run, true);
}
}  // namespace

OFLK_API int oflk_pyramidal_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float *u,
                                     float *v, float *residual_log, int *iters_run)
{
    t_resolved = 0;
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_sequence<float>(frames, T, H, W, levels, window_size, iters, 0, false, u, v, residual_log, iters_run);
}

OFLK_API int oflk_pyramidal_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                        float *u, float *v, float *residual_log, int *iters_run)
{
    t_resolved = 0;
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_sequence<unsigned char>(frames, T, H, W, levels, window_size, iters, 0, false, u, v, residual_log, iters_run);
}

OFLK_API int oflk_pyramidal_sequence_multi(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                           int n_gpus, float *u, float *v, float *residual_log, int *iters_run)
{
    t_resolved = 0;
    if (levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    return run_sequence<float>(frames, T, H, W, levels, window_size, iters, n_gpus, true, u, v, residual_log, iters_run);
}

OFLK_API int oflk_single_scale_sequence(const float *frames, int T, int H, int W, int window_size, float *u, float *v)
{
    t_resolved = 0;
    return run_sequence<float>(frames, T, H, W, 0, window_size, 0, 0, false, u, v, nullptr, nullptr);
}

// ---- forward-backward consistency ------------------------------------------------------------------------------------
namespace {
int check_alpha_beta(float alpha, float beta)
{
    if (!(std::isfinite(alpha) && alpha >= 0.0f) || !(std::isfinite(beta) && beta >= 0.0f))
        return fail(OFLK_ERR_INVALID, "alpha and beta must be finite and >= 0 (got %g, %g)", (double)alpha, (double)beta);
    return OFLK_OK;
}

int check_fb(const void *uf, const void *vf, const void *ub, const void *vb, int B, int H, int W, float alpha, float beta,
             const void *ef, const void *eb, const void *qf, const void *qb)
{
    if (!uf || !vf || !ub || !vb) return fail(OFLK_ERR_INVALID, "NULL flow argument");
    if (!ef && !eb && !qf && !qb) return fail(OFLK_ERR_INVALID, "every output is NULL");
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1 (got %d)", B);
    if (int rc = check_alpha_beta(alpha, beta)) return rc;
    return check_hw(uf, vf, H, W);   // lean_taps' 32-bit byte offsets and signed 24-bit row products
}

int fb_launch(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W, float alpha, float beta,
              float *ef, float *eb, unsigned char *qf, unsigned char *qb, hipStream_t s)
{
    FbArgs a{};
    a.uf = uf; a.vf = vf; a.ub = ub; a.vb = vb;
    a.err_f = ef; a.err_b = eb; a.valid_f = qf; a.valid_b = qb;
    a.H = H; a.W = W;
    a.alpha = alpha; a.beta = beta;
    const int dirs = ((ef || qf) ? 1 : 0) | ((eb || qb) ? 2 : 0);   // >= 1 (check_fb)
    const dim3 grid = grid2d(W, H, B);
    const bool some = with_int<1, 2, 3>(dirs, [&](auto DIRS) {
        with_bool(W == 1, [&](auto NARROW) {
            hipLaunchKernelGGL((k_fb_check<decltype(NARROW)::value, decltype(DIRS)::value>), grid, dim3(256), 0, s, a);
        });
    });
    if (!some) return fail(OFLK_ERR_INVALID, "every output is NULL");
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// The settings of the tracking, fit and stabilising calls: one aggregate a group, filled once where an OFLK_API function takes
// the flat list and passed whole from there on; each has one check (check_sparse_config, check_sparse_test, check_select,
// check_motion / check_ransac, check_stab_window).  FitConfig::model is OFLK_MOTION_*, or an internal code where the caller says so
struct PyrWindow { int levels, window_size, iters; };
struct TrackTest { float alpha, beta, max_residual; };
struct Selection { float q, md; int K, every; };
struct FitConfig { int model, hypotheses; float threshold; unsigned seed; };
struct TrajWindow { const double *weights; int radius; };               // weights [radius + 1]
struct KltConfig { PyrWindow pyr; TrackTest test; Selection select; };   // what replenished sparse KLT takes besides its frames

bool is_flow_median_size(int size) { return size == 3 || size == 5 || size == 7 || size == 9; }

int check_flow_median_size(int size)
{
    if (!is_flow_median_size(size)) return fail(OFLK_ERR_INVALID, "size must be 3, 5, 7 or 9 (got %d)", size);
    return OFLK_OK;
}

// P planes through k_flow_median<size>, cut at the grid's z limit; the arguments are checked
int flow_median_launch(const float *d_in, float *d_out, size_t P, int H, int W, int size, hipStream_t s)
{
    constexpr size_t kMaxZ = 65535;
    FlowMedianArgs a{};
    a.H = H; a.W = W;
    a.tiles_x = (W + kFlowMedianTileW - 1) / kFlowMedianTileW;
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((H + kFlowMedianTileH - 1) / kFlowMedianTileH);   // < 2^24 (check_hw)
    const size_t plane = (size_t)H * W;
    for (size_t z0 = 0; z0 < P; z0 += kMaxZ) {
        a.in = d_in + z0 * plane;
        a.out = d_out + z0 * plane;
        const dim3 grid(tiles, 1, (unsigned)std::min(kMaxZ, P - z0));
        const bool built = with_int<3, 5, 7, 9>(size, [&](auto SIZE) {
            hipLaunchKernelGGL((k_flow_median<decltype(SIZE)::value>), grid, dim3(256), 0, s, a);
        });
        if (!built) return fail(OFLK_ERR_INVALID, "size must be 3, 5, 7 or 9 (got %d)", size);
        HIP_TRY(hipGetLastError());
    }
    return OFLK_OK;
}

// The frames and the flow configuration of a host sequence call
struct Seq : PyrWindow {
    const void *frames;   // [T][H][W], uint8 or float32
    bool u8;
    int T, H, W;
    int flow_median = 0;  // 0, or the window of the median that every flow plane of a chunk goes through (3, 5, 7, 9)
    size_t frame_bytes() const { return (size_t)H * W * (u8 ? 1 : sizeof(float)); }
};

int check_seq(const Seq &seq)
{
    if (int rc = check_hw(seq.frames, seq.frames, seq.H, seq.W)) return rc;
    if (seq.T < 2) return fail(OFLK_ERR_INVALID, "a sequence needs T >= 2 frames (got %d)", seq.T);
    return OFLK_OK;
}

// One chunk of both directions of a sequence on the null stream: the device buffers of C+1 frames and of the four flows
// of C pairs (chunk_pairs), and what fills them.  With seq.flow_median one more [C][H][W] buffer: each flow array is filtered
// into it and the two pointers are exchanged, so d[0..3] are the filtered flows for whatever follows
struct BidirChunk {
    char *frames = nullptr;   // [C+1][H][W] of the call's pixels
    float *d[4] = {};         // uf, vf, ub, vb: [C][H][W] each
    float *spare = nullptr;   // [C][H][W] with seq.flow_median, else none

    static int check(const Seq &seq)   // what both directions refuse before any device call; t_resolved starts at 0
    {
        t_resolved = 0;
        if (int rc = check_seq(seq)) return rc;
        if (seq.levels < 1) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, seq.levels);
        if (seq.flow_median != 0 && !is_flow_median_size(seq.flow_median))
            return fail(OFLK_ERR_INVALID, "flow_median must be 0, 3, 5, 7 or 9 (got %d)", seq.flow_median);
        return OFLK_OK;
    }
    int alloc(HostCall &call, const Seq &seq, int C)
    {
        int rc = call.alloc(&frames, (size_t)(C + 1) * seq.frame_bytes());
        for (auto &q : d)
            if (!rc) rc = call.alloc(&q, (size_t)C * seq.H * seq.W);
        if (!rc) rc = call.alloc(&spare, (size_t)C * seq.H * seq.W, seq.flow_median != 0);
        return rc;
    }
    // pairs b0 .. b0+nb-1: their nb+1 frames go up, one bidirectional plan pass writes d, and the flagged pairs of both
    // directions are resolved (counted into t_resolved)
    int run(HostCall &call, const Seq &seq, int b0, int nb)
    {
        const size_t fb = seq.frame_bytes();
        return compute(call, seq, nb, [&] {
            return call.to_device(frames, static_cast<const char *>(seq.frames) + (size_t)b0 * fb, (size_t)(nb + 1) * fb);
        });
    }
    // the same for nb pairs whose nb+1 frames fill() puts into `frames` on the null stream, from wherever it has them (a
    // colour or NV12 call forms them on the device from the chunk it has sent up): seq.frames is not read
    template <class FILL>
    int compute(HostCall &call, const Seq &seq, int nb, FILL &&fill)
    {
        const size_t fb = seq.frame_bytes();
        oflk_plan *p = nullptr;
        int rc = host_plan(*call.c, call.dev, nb, seq.H, seq.W, seq.levels, seq.window_size, seq.iters, &p);
        if (rc || (rc = fill()) || (rc = plan_pyramidal(p, frames, frames + fb, seq.u8, d[0], d[1], nullptr, true, d[2], d[3])))
            return rc;
        int n_res = 0;
        if (seq.iters > 0 && (rc = resolve_uncertain_fb(p, frames, seq.u8, d[0], d[1], d[2], d[3], nullptr, &n_res))) return rc;
        t_resolved += n_res;
        if (!seq.flow_median) return OFLK_OK;
        for (auto &q : d) {   // the resolved flows are the ones filtered
            if ((rc = flow_median_launch(q, spare, (size_t)nb, seq.H, seq.W, seq.flow_median, nullptr))) return rc;
            std::swap(q, spare);
        }
        return OFLK_OK;
    }
};

// Both directions of a sequence and their consistency, host pointers.  Chunks of C pairs run one after the other on the
// null stream: BidirChunk fills d[0..3], one check launch follows, everything comes down, and the stream is synchronized,
// as the next chunk reuses the buffers.
template <class PIXELS>
int run_sequence_fb(const PIXELS *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha, float beta,
                    float *uf, float *vf, float *ub, float *vb, float *ef, float *eb, unsigned char *qf, unsigned char *qb,
                    int flow_median = 0)
{
    const Seq seq{{levels, window_size, iters}, frames, sizeof(PIXELS) == 1, T, H, W, flow_median};
    const bool check = ef || eb || qf || qb;
    int rc = BidirChunk::check(seq);
    if (rc || (check && (rc = check_fb(uf, vf, ub, vb, T - 1, H, W, alpha, beta, ef, eb, qf, qb)))) return rc;
    if (!uf || !vf || !ub || !vb) return fail(OFLK_ERR_INVALID, "NULL flow argument");
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int B = T - 1, C = chunk_pairs(B, H, W);
    const size_t plane = (size_t)H * W;
    BidirChunk k{};
    float *d_e[2];
    float *const outs[4] = {uf, vf, ub, vb};
    unsigned char *d_q[2];
    if ((rc = k.alloc(call, seq, C)) || (rc = call.alloc(&d_e[0], C * plane, ef)) || (rc = call.alloc(&d_e[1], C * plane, eb)) ||
        (rc = call.alloc(&d_q[0], C * plane, qf)) || (rc = call.alloc(&d_q[1], C * plane, qb)))
        return rc;
    for (int b0 = 0; b0 < B; b0 += C) {
        const int nb = std::min(C, B - b0);
        const size_t off = (size_t)b0 * plane, n = (size_t)nb * plane;
        if ((rc = k.run(call, seq, b0, nb))) return rc;
        if (check && (rc = fb_launch(k.d[0], k.d[1], k.d[2], k.d[3], nb, H, W, alpha, beta, d_e[0], d_e[1], d_q[0], d_q[1], nullptr)))
            return rc;
        for (int i = 0; i < 4; i++)
            if ((rc = call.to_host(outs[i] + off, k.d[i], n))) return rc;
        if ((ef && (rc = call.to_host(ef + off, d_e[0], n))) || (eb && (rc = call.to_host(eb + off, d_e[1], n))) ||
            (qf && (rc = call.to_host(qf + off, d_q[0], n))) || (qb && (rc = call.to_host(qb + off, d_q[1], n))) ||
            (rc = call.sync()))
            return rc;
    }
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_fb_consistency(const float *d_uf, const float *d_vf, const float *d_ub, const float *d_vb, int B, int H, int W,
                                 float alpha, float beta, float *d_err_f, float *d_err_b, unsigned char *d_valid_f,
                                 unsigned char *d_valid_b, void *stream)
{
    int rc = check_fb(d_uf, d_vf, d_ub, d_vb, B, H, W, alpha, beta, d_err_f, d_err_b, d_valid_f, d_valid_b);
    if (rc) return rc;
    return fb_launch(d_uf, d_vf, d_ub, d_vb, B, H, W, alpha, beta, d_err_f, d_err_b, d_valid_f, d_valid_b, (hipStream_t)stream);
}

OFLK_API int oflk_fb_consistency_host(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W,
                                      float alpha, float beta, float *err_f, float *err_b, unsigned char *valid_f,
                                      unsigned char *valid_b)
{
    int rc = check_fb(uf, vf, ub, vb, B, H, W, alpha, beta, err_f, err_b, valid_f, valid_b);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)B * H * W;
    const float *in[4] = {uf, vf, ub, vb};
    float *d[4], *d_e[2];
    unsigned char *d_q[2];
    for (int i = 0; i < 4; i++)
        if ((rc = call.upload(&d[i], in[i], n))) return rc;
    if ((rc = call.alloc(&d_e[0], n, err_f)) || (rc = call.alloc(&d_e[1], n, err_b)) || (rc = call.alloc(&d_q[0], n, valid_f)) ||
        (rc = call.alloc(&d_q[1], n, valid_b)))
        return rc;
    if ((rc = fb_launch(d[0], d[1], d[2], d[3], B, H, W, alpha, beta, d_e[0], d_e[1], d_q[0], d_q[1], nullptr))) return rc;
    if ((err_f && (rc = call.to_host(err_f, d_e[0], n))) || (err_b && (rc = call.to_host(err_b, d_e[1], n))) ||
        (valid_f && (rc = call.to_host(valid_f, d_q[0], n))) || (valid_b && (rc = call.to_host(valid_b, d_q[1], n))))
        return rc;
    return call.sync();
}

OFLK_API int oflk_pyramidal_sequence_fb(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                        float alpha, float beta, float *uf, float *vf, float *ub, float *vb, float *err_f,
                                        float *err_b, unsigned char *valid_f, unsigned char *valid_b)
{
    return run_sequence_fb<float>(frames, T, H, W, levels, window_size, iters, alpha, beta, uf, vf, ub, vb, err_f, err_b, valid_f,
                                  valid_b);
}

OFLK_API int oflk_pyramidal_sequence_fb_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                           int iters, float alpha, float beta, float *uf, float *vf, float *ub, float *vb,
                                           float *err_f, float *err_b, unsigned char *valid_f, unsigned char *valid_b)
{
    return run_sequence_fb<unsigned char>(frames, T, H, W, levels, window_size, iters, alpha, beta, uf, vf, ub, vb, err_f, err_b,
                                          valid_f, valid_b);
}

OFLK_API int oflk_pyramidal_sequence_fb_median(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                               float alpha, float beta, int flow_median, float *uf, float *vf, float *ub,
                                               float *vb, float *err_f, float *err_b, unsigned char *valid_f,
                                               unsigned char *valid_b)
{
    return run_sequence_fb<float>(frames, T, H, W, levels, window_size, iters, alpha, beta, uf, vf, ub, vb, err_f, err_b, valid_f,
                                  valid_b, flow_median);
}

OFLK_API int oflk_pyramidal_sequence_fb_median_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                                  int iters, float alpha, float beta, int flow_median, float *uf, float *vf,
                                                  float *ub, float *vb, float *err_f, float *err_b, unsigned char *valid_f,
                                                  unsigned char *valid_b)
{
    return run_sequence_fb<unsigned char>(frames, T, H, W, levels, window_size, iters, alpha, beta, uf, vf, ub, vb, err_f, err_b,
                                          valid_f, valid_b, flow_median);
}

// ---- Shi-Tomasi corners ----------------------------------------------------------------------------------------------
namespace {
int check_corner_window(int window_size)
{
    if (window_size < 3 || window_size > 11 || window_size % 2 == 0)
        return fail(OFLK_ERR_UNSUPPORTED, "corner windows are odd sizes in [3,11] (got %d)", window_size);
    return OFLK_OK;
}

// the selection's parameters (every value OFLK_ERR_INVALID)
int check_select(float q, float md, int K)
{
    if (!(std::isfinite(q) && q >= 0.0f && q <= 1.0f))
        return fail(OFLK_ERR_INVALID, "quality_level must be in [0,1] (got %g)", (double)q);
    if (!(std::isfinite(md) && md >= 0.0f)) return fail(OFLK_ERR_INVALID, "min_distance must be finite and >= 0 (got %g)", (double)md);
    if (K < 1) return fail(OFLK_ERR_INVALID, "max_corners must be >= 1 (got %d)", K);
    return OFLK_OK;
}
int check_select(const Selection &k) { return check_select(k.q, k.md, k.K); }   // `every` is the caller's: >= 1 or >= 0

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// a grid of cells of side ceil(md) over the frame (one cell once that covers the frame); none unless `on`
struct CellGrid { int cell, gw, gh; };

CellGrid cell_grid(bool on, float md, int H, int W)
{
    if (!on) return {};
    const int cell = (int)std::min<double>(std::ceil((double)md), (double)std::max(H, W));
    return {cell, (W + cell - 1) / cell, (H + cell - 1) / cell};
}

// The workspace of oflk_good_features, 256-byte aligned pieces: fmax [F] and ncand [F] (zeroed by k_corner_init), S
// [F][H][W], keys [F][H*W] (the worst case: every pixel a candidate) and, for md > 1, the grid [F][gh][gw][4].
// That of oflk_replenish_features (slots = K) is the one of one frame, then the seed grid's heads [gh][gw] (md = 0:
// none), its nodes [K], the free list [K] and its length [1].
struct FeatWs {
    CellGrid occ, seed;   // the selection's occupancy grid and the seeds' grid
    unsigned *fmax, *ncand;
    float *S;
    unsigned long long *keys;
    int *grid, *head, *free, *nfree;   // grid, head: NULL without their cells
    int2 *node;
    size_t bytes;
};

// the pieces of a workspace at `base` (NULL: only `bytes` is of use)
FeatWs feat_ws(void *base, int F, int H, int W, float md, int slots)
{
    FeatWs v{};
    v.occ = cell_grid(md > 1.0f, md, H, W);
    if (slots) v.seed = cell_grid(md > 0.0f, md, H, W);
    auto take = [&](auto *&p, size_t n) {   // the next piece: n elements
        p = n ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(base) + v.bytes) : nullptr;
        v.bytes += align256(n * sizeof(*p));
    };
    const size_t nF = (size_t)F, plane = (size_t)H * (size_t)W;
    take(v.fmax, nF); take(v.ncand, nF);
    take(v.S, nF * plane); take(v.keys, nF * plane);
    take(v.grid, nF * (size_t)v.occ.gw * v.occ.gh * 4);
    if (slots) {
        take(v.head, (size_t)v.seed.gw * v.seed.gh);
        take(v.node, (size_t)slots); take(v.free, (size_t)slots); take(v.nfree, 1);
    }
    return v;
}

int corner_score_launch(const void *frames, bool u8, int F, int H, int W, int window_size, float *score, unsigned *fmax,
                        hipStream_t s)
{
    CornerArgs a{};
    a.frames = frames;
    a.score = score;
    a.fmax = fmax;
    a.F = F; a.H = H; a.W = W;
    const dim3 grid((unsigned)((W + kCsTW - 1) / kCsTW), (unsigned)std::min((H + kCsTH - 1) / kCsTH, 65535),
                    (unsigned)std::min(F, 65535));
    const bool built = with_half_window(window_size / 2, [&](auto HW) {
        with_pix(u8, [&](auto PIX) {
            hipLaunchKernelGGL((k_corner_score<typename decltype(PIX)::type, decltype(HW)::value>), grid, dim3(256), 0, s, a);
        });
    });
    if (!built) return fail(OFLK_ERR_UNSUPPORTED, "corner window %d not built", window_size);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// The slot side of a detection (the replenish statement, F = 1): the slots' state (xy, visible) of frame t in; the new
// points go into the free slots of qt and of the selection's xy (the queries), born [K] and detected [1] out
struct SlotSide {
    const float *xy; const unsigned char *visible;
    int *qt; unsigned char *born; int *detected; int t;
};

// Score, candidates and selection of F frames on stream s, no host round trip; the arguments are checked.  Without
// slots the selection writes count, xy and score; with them it fills free slots and uses neither count nor score.
int detect_launch(const void *frames, bool u8, int F, int H, int W, int window_size, float q, float md, int K, const FeatWs &ws,
                  int *count, float *xy, float *score, const SlotSide *slots, hipStream_t s)
{
    const unsigned fz = (unsigned)std::min(F, 65535);
    CandArgs c{};
    c.score = ws.S; c.fmax = ws.fmax; c.keys = ws.keys; c.ncand = ws.ncand;
    c.F = F; c.H = H; c.W = W;
    c.q = (double)q;
    SelectArgs a{};
    a.keys = ws.keys; a.ncand = ws.ncand; a.grid = ws.grid;
    a.count = slots ? slots->detected : count; a.xy = xy; a.score = slots ? nullptr : score;
    a.F = F; a.H = H; a.W = W; a.K = K;
    a.cell = std::max(ws.occ.cell, 1); a.gw = ws.occ.gw; a.gh = ws.occ.gh;
    a.md2 = (double)md * (double)md;
    a.use_grid = ws.occ.cell != 0;
    hipLaunchKernelGGL(k_corner_init, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, ws.fmax, ws.ncand, F);
    HIP_TRY(hipGetLastError());
    int rc = corner_score_launch(frames, u8, F, H, W, window_size, ws.S, ws.fmax, s);
    if (rc) return rc;
    if (slots) {   // the seeds' lists and the free list, and what the two kernels take of them
        if (ws.head) {
            const int cells = ws.seed.gw * ws.seed.gh;
            hipLaunchKernelGGL(k_seed_clear, dim3((unsigned)std::min((cells + 255) / 256, 1024)), dim3(256), 0, s, ws.head, cells);
            HIP_TRY(hipGetLastError());
        }
        SeedArgs sa{};
        sa.xy = slots->xy; sa.visible = slots->visible; sa.born = slots->born; sa.head = ws.head; sa.node = ws.node;
        sa.K = K; sa.H = H; sa.W = W; sa.cell = std::max(ws.seed.cell, 1); sa.gw = ws.seed.gw;
        hipLaunchKernelGGL(k_seed_link, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, sa);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_free_list, dim3(1), dim3(256), 0, s, slots->visible, K, ws.free, ws.nfree);
        HIP_TRY(hipGetLastError());
        c.head = ws.head; c.node = ws.node; c.cell = sa.cell; c.gw = ws.seed.gw; c.gh = ws.seed.gh;
        c.md2 = a.md2;
        a.free = ws.free; a.nfree = ws.nfree; a.qt = slots->qt; a.born = slots->born; a.t = slots->t;
    }
    const dim3 cgrid((unsigned)((W + 63) / 64), (unsigned)std::min((H + 3) / 4, 65535), fz);
    with_bool(ws.head != nullptr, [&](auto SEEDS) { hipLaunchKernelGGL(k_corner_cand<decltype(SEEDS)::value>, cgrid, dim3(256), 0, s, c); });
    HIP_TRY(hipGetLastError());
    with_bool(slots != nullptr, [&](auto SLOTS) {
        hipLaunchKernelGGL(k_corner_select<decltype(SLOTS)::value>, dim3(fz), dim3(256), 0, s, a);
    });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

int check_corner_frames(const void *frames, int F, int H, int W)
{
    if (!frames) return fail(OFLK_ERR_INVALID, "NULL frames");
    if (F < 1) return fail(OFLK_ERR_INVALID, "F must be >= 1 (got %d)", F);
    return check_hw(frames, frames, H, W);
}

template <class PIXELS>
int corner_score_host(const PIXELS *frames, int F, int H, int W, int window_size, float *score)
{
    int rc = check_corner_frames(frames, F, H, W);
    if (rc) return rc;
    if (!score) return fail(OFLK_ERR_INVALID, "NULL score");
    if ((rc = check_corner_window(window_size))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)F * H * W;
    PIXELS *d_f;
    float *d_s;
    if ((rc = call.upload(&d_f, frames, n)) || (rc = call.alloc(&d_s, n))) return rc;
    if ((rc = corner_score_launch(d_f, sizeof(PIXELS) == 1, F, H, W, window_size, d_s, nullptr, nullptr))) return rc;
    if ((rc = call.to_host(score, d_s, n))) return rc;
    return call.sync();
}

template <class PIXELS>
int good_features_host(const PIXELS *frames, int F, int H, int W, int window_size, float q, float md, int K, int *count,
                       float *xy, float *score)
{
    int rc = check_corner_frames(frames, F, H, W);
    if (rc) return rc;
    if (!count || !xy || !score) return fail(OFLK_ERR_INVALID, "NULL output argument");
    if ((rc = check_select(q, md, K)) || (rc = check_corner_window(window_size))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)F * H * W, nk = (size_t)F * K;
    PIXELS *d_f;
    char *d_ws;
    int *d_cnt;
    float *d_xy, *d_sc;
    if ((rc = call.upload(&d_f, frames, n)) || (rc = call.alloc(&d_ws, feat_ws(nullptr, F, H, W, md, 0).bytes)) ||
        (rc = call.alloc(&d_cnt, (size_t)F)) || (rc = call.alloc(&d_xy, 2 * nk)) || (rc = call.alloc(&d_sc, nk)))
        return rc;
    if ((rc = detect_launch(d_f, sizeof(PIXELS) == 1, F, H, W, window_size, q, md, K, feat_ws(d_ws, F, H, W, md, 0), d_cnt, d_xy,
                            d_sc, nullptr, nullptr)))
        return rc;
    if ((rc = call.to_host(count, d_cnt, (size_t)F)) || (rc = call.to_host(xy, d_xy, 2 * nk)) ||
        (rc = call.to_host(score, d_sc, nk)))
        return rc;
    return call.sync();
}

// the arguments of one detection, host or device pointers
int check_replenish(const void *frame, int H, int W, int window_size, float q, float md, int K, int t, const void *xy,
                    const void *visible, const void *qt, const void *qxy, const void *born, const void *detected)
{
    int rc = check_corner_frames(frame, 1, H, W);
    if (rc) return rc;
    if (!xy || !visible || !qt || !qxy || !born || !detected) return fail(OFLK_ERR_INVALID, "NULL slot state or output argument");
    if (t < 0) return fail(OFLK_ERR_INVALID, "t must be >= 0 (got %d)", t);
    if ((rc = check_select(q, md, K))) return rc;
    return check_corner_window(window_size);
}

template <class PIXELS>
int replenish_host(const PIXELS *frame, int H, int W, int window_size, float q, float md, int K, int t, const float *xy,
                   const unsigned char *visible, int *qt, float *qxy, unsigned char *born, int *detected)
{
    int rc = check_replenish(frame, H, W, window_size, q, md, K, t, xy, visible, qt, qxy, born, detected);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t row = (size_t)K;
    PIXELS *d_f;
    char *d_ws;
    float *d_xy, *d_qxy;
    unsigned char *d_vis, *d_born;
    int *d_qt, *d_det;
    if ((rc = call.upload(&d_f, frame, (size_t)H * W)) || (rc = call.alloc(&d_ws, feat_ws(nullptr, 1, H, W, md, K).bytes)) ||
        (rc = call.upload(&d_xy, xy, 2 * row)) || (rc = call.upload(&d_vis, visible, row)) ||
        (rc = call.upload(&d_qt, const_cast<const int *>(qt), row)) ||
        (rc = call.upload(&d_qxy, const_cast<const float *>(qxy), 2 * row)) || (rc = call.alloc(&d_born, row)) ||
        (rc = call.alloc(&d_det, 1)))
        return rc;
    const SlotSide slots{d_xy, d_vis, d_qt, d_born, d_det, t};
    if ((rc = detect_launch(d_f, sizeof(PIXELS) == 1, 1, H, W, window_size, q, md, K, feat_ws(d_ws, 1, H, W, md, K), nullptr, d_qxy,
                            nullptr, &slots, nullptr)))
        return rc;
    if ((rc = call.to_host(qt, d_qt, row)) || (rc = call.to_host(qxy, d_qxy, 2 * row)) || (rc = call.to_host(born, d_born, row)) ||
        (rc = call.to_host(detected, d_det, 1)))
        return rc;
    return call.sync();
}
}  // namespace

OFLK_API int oflk_corner_score(const void *d_frames, int u8, int F, int H, int W, int window_size, float *d_score, void *stream)
{
    int rc = check_corner_frames(d_frames, F, H, W);
    if (rc) return rc;
    if (!d_score) return fail(OFLK_ERR_INVALID, "NULL d_score");
    if ((rc = check_corner_window(window_size))) return rc;
    return corner_score_launch(d_frames, u8 != 0, F, H, W, window_size, d_score, nullptr, (hipStream_t)stream);
}

OFLK_API int oflk_corner_score_host(const float *frames, int F, int H, int W, int window_size, float *score)
{
    return corner_score_host<float>(frames, F, H, W, window_size, score);
}

OFLK_API int oflk_corner_score_host_u8(const unsigned char *frames, int F, int H, int W, int window_size, float *score)
{
    return corner_score_host<unsigned char>(frames, F, H, W, window_size, score);
}

OFLK_API int oflk_good_features_workspace(int F, int H, int W, int window_size, float min_distance, int max_corners,
                                          size_t *bytes)
{
    if (!bytes) return fail(OFLK_ERR_INVALID, "NULL bytes");
    if (F < 1) return fail(OFLK_ERR_INVALID, "F must be >= 1 (got %d)", F);
    int rc = check_hw(bytes, bytes, H, W);
    if (rc || (rc = check_select(0.0f, min_distance, max_corners)) || (rc = check_corner_window(window_size))) return rc;
    *bytes = feat_ws(nullptr, F, H, W, min_distance, 0).bytes;
    return OFLK_OK;
}

OFLK_API int oflk_good_features(const void *d_frames, int u8, int F, int H, int W, int window_size, float quality_level,
                                float min_distance, int max_corners, void *d_workspace, size_t workspace_bytes, int *d_count,
                                float *d_xy, float *d_score, void *stream)
{
    int rc = check_corner_frames(d_frames, F, H, W);
    if (rc) return rc;
    if (!d_workspace || !d_count || !d_xy || !d_score) return fail(OFLK_ERR_INVALID, "NULL workspace or output argument");
    if ((rc = check_select(quality_level, min_distance, max_corners)) || (rc = check_corner_window(window_size))) return rc;
    const size_t need = feat_ws(nullptr, F, H, W, min_distance, 0).bytes;
    if (workspace_bytes < need)
        return fail(OFLK_ERR_INVALID, "workspace of %zu bytes, %zu needed (oflk_good_features_workspace)", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(d_workspace) % 256 != 0 || reinterpret_cast<uintptr_t>(d_xy) % 8 != 0)
        return fail(OFLK_ERR_INVALID, "d_workspace must be 256-byte aligned and d_xy 8-byte aligned");
    return detect_launch(d_frames, u8 != 0, F, H, W, window_size, quality_level, min_distance, max_corners,
                         feat_ws(d_workspace, F, H, W, min_distance, 0), d_count, d_xy, d_score, nullptr, (hipStream_t)stream);
}

OFLK_API int oflk_good_features_host(const float *frames, int F, int H, int W, int window_size, float quality_level,
                                     float min_distance, int max_corners, int *count, float *xy, float *score)
{
    return good_features_host<float>(frames, F, H, W, window_size, quality_level, min_distance, max_corners, count, xy, score);
}

OFLK_API int oflk_good_features_host_u8(const unsigned char *frames, int F, int H, int W, int window_size, float quality_level,
                                        float min_distance, int max_corners, int *count, float *xy, float *score)
{
    return good_features_host<unsigned char>(frames, F, H, W, window_size, quality_level, min_distance, max_corners, count, xy,
                                             score);
}

OFLK_API int oflk_replenish_features_workspace(int H, int W, int window_size, float min_distance, int max_corners, size_t *bytes)
{
    if (!bytes) return fail(OFLK_ERR_INVALID, "NULL bytes");
    int rc = check_hw(bytes, bytes, H, W);
    if (rc || (rc = check_select(0.0f, min_distance, max_corners)) || (rc = check_corner_window(window_size))) return rc;
    *bytes = feat_ws(nullptr, 1, H, W, min_distance, max_corners).bytes;
    return OFLK_OK;
}

OFLK_API int oflk_replenish_features(const void *d_frame, int u8, int H, int W, int window_size, float quality_level,
                                     float min_distance, int max_corners, int t, const float *d_xy,
                                     const unsigned char *d_visible, void *d_workspace, size_t workspace_bytes, int *d_qt,
                                     float *d_qxy, unsigned char *d_born, int *d_detected, void *stream)
{
    int rc = check_replenish(d_frame, H, W, window_size, quality_level, min_distance, max_corners, t, d_xy, d_visible, d_qt, d_qxy,
                             d_born, d_detected);
    if (rc) return rc;
    if (!d_workspace) return fail(OFLK_ERR_INVALID, "NULL workspace");
    const size_t need = feat_ws(nullptr, 1, H, W, min_distance, max_corners).bytes;
    if (workspace_bytes < need)
        return fail(OFLK_ERR_INVALID, "workspace of %zu bytes, %zu needed (oflk_replenish_features_workspace)", workspace_bytes,
                    need);
    if (reinterpret_cast<uintptr_t>(d_workspace) % 256 != 0 || reinterpret_cast<uintptr_t>(d_qxy) % 8 != 0)
        return fail(OFLK_ERR_INVALID, "d_workspace must be 256-byte aligned and d_qxy 8-byte aligned");
    const SlotSide slots{d_xy, d_visible, d_qt, d_born, d_detected, t};
    return detect_launch(d_frame, u8 != 0, 1, H, W, window_size, quality_level, min_distance, max_corners,
                         feat_ws(d_workspace, 1, H, W, min_distance, max_corners), nullptr, d_qxy, nullptr, &slots,
                         (hipStream_t)stream);
}

OFLK_API int oflk_replenish_features_host(const float *frame, int H, int W, int window_size, float quality_level,
                                          float min_distance, int max_corners, int t, const float *xy,
                                          const unsigned char *visible, int *qt, float *qxy, unsigned char *born, int *detected)
{
    return replenish_host<float>(frame, H, W, window_size, quality_level, min_distance, max_corners, t, xy, visible, qt, qxy, born,
                                 detected);
}

OFLK_API int oflk_replenish_features_host_u8(const unsigned char *frame, int H, int W, int window_size, float quality_level,
                                             float min_distance, int max_corners, int t, const float *xy,
                                             const unsigned char *visible, int *qt, float *qxy, unsigned char *born,
                                             int *detected)
{
    return replenish_host<unsigned char>(frame, H, W, window_size, quality_level, min_distance, max_corners, t, xy, visible, qt,
                                         qxy, born, detected);
}

// ---- point tracks ----------------------------------------------------------------------------------------------------
namespace {
// the query arguments of every track entry point; qt (host forms only, may be NULL) must lie in [0, T-1]
int check_queries(const int *qt, int T, const void *qxy, int N, const void *tracks, const void *visible)
{
    if (!qxy || !tracks || !visible) return fail(OFLK_ERR_INVALID, "NULL query or output argument");
    if (N < 1) return fail(OFLK_ERR_INVALID, "N must be >= 1 (got %d)", N);
    for (int n = 0; qt && n < N; n++)
        if (qt[n] < 0 || qt[n] >= T) return fail(OFLK_ERR_INVALID, "query %d: frame %d outside [0,%d]", n, qt[n], T - 1);
    return OFLK_OK;
}

// the flows' and the test's arguments as oflk_fb_consistency takes them, then the queries'
int check_track(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W, float alpha, float beta,
                const int *qt, const float *qxy, int N, const float *tracks, const unsigned char *visible)
{
    int rc = check_fb(uf, vf, ub, vb, B, H, W, alpha, beta, tracks, nullptr, nullptr, nullptr);
    return rc ? rc : check_queries(qt, B + 1, qxy, N, tracks, visible);
}

int track_launch(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W, float alpha, float beta,
                 int t0, const int *qt, const float *qxy, int N, float *tracks, unsigned char *visible, hipStream_t s)
{
    TrackArgs a{};
    a.uf = uf; a.vf = vf; a.ub = ub; a.vb = vb;
    a.qt = qt; a.qxy = qxy;
    a.tracks = tracks; a.visible = visible;
    a.B = B; a.H = H; a.W = W; a.N = N; a.t0 = t0;
    a.alpha = alpha; a.beta = beta;
    const dim3 grid((unsigned)((N + 63) / 64));
    with_bool(W == 1, [&](auto NARROW) { hipLaunchKernelGGL(k_track<decltype(NARROW)::value>, grid, dim3(64), 0, s, a); });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

struct TrackRows {   // the device side of every sequence track call: the queries and one chunk's rows
    int *qt = nullptr;                     // [N]; NULL: every query starts on frame 0
    float *qxy = nullptr, *tr = nullptr;   // [N][2] and [C+1][N][2]
    unsigned char *vis = nullptr;          // [C+1][N]
    float *res = nullptr;                  // [C+1][N] step residuals, which only the sparse engine writes; NULL: none
};

// The pairs t0 .. t0+B-1 in segments [s0, e) cut at the multiples of `every`, the detection frames (0: none, one segment):
// detect(s0, r) ahead of a segment that begins on one, then step(s0, e, r) for every segment; r = s0 - t0 is the segment's
// first row.  The last row is never a detection row.  64-bit: t0 + B may reach INT_MAX.
template <class Detect, class Step>
int walk_segments(int t0, int B, int every, Detect detect, Step step)
{
    const long long end = (long long)t0 + B;
    for (long long s0 = t0; s0 < end;) {
        const long long e = every ? std::min(end, (s0 / every + 1) * every) : end;
        const int r = (int)(s0 - t0);
        int rc;
        if (every && s0 % every == 0 && (rc = detect((int)s0, r))) return rc;
        if ((rc = step((int)s0, (int)e, r))) return rc;
        s0 = e;
    }
    return OFLK_OK;
}

// Tracks of a whole sequence, host pointers: the one driver of the six sequence track calls.  Chunks of C pairs run one after
// the other on the null stream.  The chunk's frames go up (the dense engine's flows follow them at once); row 0 of a later
// chunk is the previous chunk's last row; a source that detects once does so now, on the first chunk's frame 0; the engine
// readies the chunk (the sparse engine's pyramids); its pairs are walked in segments (walk_segments): before the segment
// that begins at a detection frame s, the source puts new queries (qt, qxy) into R from row r of the chunk, and the segment's
// launch (t0 = s) starts them on its row 0 and continues the others; the rows come down and the stream is synchronized, as
// the next chunk reuses the buffers.
//   Engine: how tracks are made.  check(seq) its refusals, pairs(B, H, W) a chunk's size, alloc(call, seq, C),
//           upload(call, seq, b0, nb) the chunk's frames up, ready(seq) what else a chunk needs before its segments,
//           frame(seq, r) the chunk's device frame r, step(seq, R, N, s0, e, r) one segment's launch.  DenseTracks, SparseTracks.
//   Source: where queries come from.  check(seq, tracks, visible), detect_every(T), setup(call, seq, R, C) its buffers,
//           first(call, seq, R, frame, b0) on an uploaded chunk's frame 0, begin(R, b0, nb) ahead of a chunk's segments,
//           detect(call, seq, R, frame, s, r) and down(call, seq, R, b0, nb, r0): what comes down beside rows r0 .. nb.
//           GivenQueries, DetectOnce and Replenished.
template <class Engine, class Source>
int run_sequence_tracks(const Seq &seq, Engine eng, Source src, int N, float *tracks, unsigned char *visible)
{
    int rc = eng.check(seq);
    if (rc || (rc = src.check(seq, tracks, visible))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int B = seq.T - 1, C = eng.pairs(B, seq.H, seq.W), every = src.detect_every(seq.T);
    const size_t row = (size_t)N;
    TrackRows R;
    if ((rc = eng.alloc(call, seq, C)) || (rc = call.alloc(&R.tr, (size_t)(C + 1) * 2 * row)) ||
        (rc = call.alloc(&R.vis, (size_t)(C + 1) * row)) || (rc = src.setup(call, seq, R, C)))
        return rc;
    for (int b0 = 0; b0 < B; b0 += C) {
        const int nb = std::min(C, B - b0);
        if ((rc = eng.upload(call, seq, b0, nb))) return rc;
        if (b0 > 0) {   // row 0 of this chunk is the previous (full, C-pair) chunk's last row
            HIP_TRY(hipMemcpyAsync(R.tr, R.tr + (size_t)C * 2 * row, 2 * row * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(R.vis, R.vis + (size_t)C * row, row, hipMemcpyDeviceToDevice, nullptr));
        }
        if ((rc = src.first(call, seq, R, eng.frame(seq, 0), b0)) || (rc = eng.ready(seq)) || (rc = src.begin(R, b0, nb))) return rc;
        rc = walk_segments(b0, nb, every, [&](int s, int r) { return src.detect(call, seq, R, eng.frame(seq, r), s, r); },
                           [&](int s0, int e, int r) { return eng.step(seq, R, N, s0, e, r); });
        if (rc) return rc;
        // row 0 of a later chunk is already on the host, unless the chunk begins at a detection frame: that segment's
        // launch is what makes the row final, so it goes again
        const int r0 = b0 > 0 && !(every && b0 % every == 0) ? 1 : 0;
        const size_t nr = (size_t)(nb + 1 - r0);
        if ((rc = call.to_host(tracks + (size_t)(b0 + r0) * 2 * row, R.tr + (size_t)r0 * 2 * row, nr * 2 * row)) ||
            (rc = call.to_host(visible + (size_t)(b0 + r0) * row, R.vis + (size_t)r0 * row, nr * row)) ||
            (rc = src.down(call, seq, R, b0, nb, r0)) || (rc = call.sync()))
            return rc;
    }
    return OFLK_OK;
}

// The dense engine: a chunk is BidirChunk's (run_sequence_fb's), a segment one k_track launch on its flows
struct DenseTracks {
    float alpha, beta;
    BidirChunk k{};

    int check(const Seq &seq) const
    {
        const int rc = BidirChunk::check(seq);
        return rc ? rc : check_alpha_beta(alpha, beta);
    }
    static int pairs(int B, int H, int W) { return chunk_pairs(B, H, W); }
    int alloc(HostCall &call, const Seq &seq, int C) { return k.alloc(call, seq, C); }
    int upload(HostCall &call, const Seq &seq, int b0, int nb) { return k.run(call, seq, b0, nb); }   // and both flows
    static int ready(const Seq &) { return OFLK_OK; }
    const void *frame(const Seq &seq, int r) const { return k.frames + (size_t)r * seq.frame_bytes(); }
    int step(const Seq &seq, const TrackRows &R, int N, int s0, int e, int r) const
    {
        const size_t fo = (size_t)r * seq.H * seq.W, row = (size_t)N;
        return track_launch(k.d[0] + fo, k.d[1] + fo, k.d[2] + fo, k.d[3] + fo, e - s0, seq.H, seq.W, alpha, beta, s0, R.qt, R.qxy, N,
                            R.tr + (size_t)r * 2 * row, R.vis + (size_t)r * row, nullptr);
    }
};

constexpr auto no_part = [](auto &&...) -> int { return OFLK_OK; };   // a part that a source does not have

// The caller's queries: they go up, and no frame is a detection frame
struct GivenQueries {
    const int *qt;      // [N] or NULL
    const float *qxy;   // [N][2]
    int N;

    int check(const Seq &seq, const void *tracks, const void *visible) const
    {
        return check_queries(qt, seq.T, qxy, N, tracks, visible);
    }
    static int detect_every(int) { return 0; }
    int setup(HostCall &call, const Seq &, TrackRows &R, int) const
    {
        const int rc = call.upload(&R.qxy, qxy, 2 * (size_t)N);
        return rc || !qt ? rc : call.upload(&R.qt, qt, (size_t)N);
    }
    static constexpr auto first = no_part, begin = no_part, detect = no_part, down = no_part;
};

// One detection, on frame 0 as soon as the first chunk's frames are up; no frame of the walk is a detection frame.  Its xy
// go straight into the query buffer (N = K; the NaN rows are never-visible tracks), and count, xy and score come down with
// chunk 0.
struct DetectOnce {
    float q, md;
    int K;
    int *count;          // the caller's [1], [K][2] and [K]
    float *xy, *score;
    char *d_ws = nullptr;
    int *d_cnt = nullptr;
    float *d_sc = nullptr;

    int check(const Seq &seq, const void *tracks, const void *visible) const
    {
        if (!count || !xy || !score || !tracks || !visible) return fail(OFLK_ERR_INVALID, "NULL output argument");
        const int rc = check_select(q, md, K);
        // never a second text for a window on the sparse engine, whose own check of the same odd sizes 3 .. 11 comes first
        return rc ? rc : check_corner_window(seq.window_size);
    }
    static int detect_every(int) { return 0; }
    int setup(HostCall &call, const Seq &seq, TrackRows &R, int)
    {
        int rc;
        if ((rc = call.alloc(&R.qxy, 2 * (size_t)K)) || (rc = call.alloc(&d_ws, feat_ws(nullptr, 1, seq.H, seq.W, md, 0).bytes)) ||
            (rc = call.alloc(&d_cnt, 1)) || (rc = call.alloc(&d_sc, (size_t)K)))
            return rc;
        return OFLK_OK;
    }
    int first(HostCall &call, const Seq &seq, const TrackRows &R, const void *d_frame, int b0) const
    {
        if (b0 > 0) return OFLK_OK;
        int rc = detect_launch(d_frame, seq.u8, 1, seq.H, seq.W, seq.window_size, q, md, K, feat_ws(d_ws, 1, seq.H, seq.W, md, 0),
                               d_cnt, R.qxy, d_sc, nullptr, nullptr);
        if (rc || (rc = call.to_host(count, d_cnt, 1)) || (rc = call.to_host(xy, R.qxy, 2 * (size_t)K)) ||
            (rc = call.to_host(score, d_sc, (size_t)K)))
            return rc;
        return OFLK_OK;
    }
    static constexpr auto begin = no_part, detect = no_part, down = no_part;
};

// The slot side of replenished KLT: the K queries are slots, every one dead at first.  On every `every`-th frame s the
// detection fills free slots (qt = s, qxy) from the slots' row of s, born with them.  The selection's parameters, its
// workspace (feat_ws(.., 1, .., K)) and the per-row outputs of a pass of B+1 rows
struct Slots : Selection {
    void *ws = nullptr;
    unsigned char *born = nullptr;   // [B+1][K]
    int *detected = nullptr;         // [B+1]
};

// ahead of a pass of B+1 rows that begins on frame t0: the slots' first state (t0 = 0) and the pass's born and detected rows
// cleared, by kernels on stream s (a pass is captured into graphs: no memset)
int slots_begin(const Slots &k, const TrackRows &R, int t0, int B, hipStream_t s)
{
    if (t0 == 0) {
        hipLaunchKernelGGL(k_slots_init, dim3((unsigned)((k.K + 255) / 256)), dim3(256), 0, s, R.qt, reinterpret_cast<float2 *>(R.qxy),
                           reinterpret_cast<float2 *>(R.tr), R.vis, k.K);
        HIP_TRY(hipGetLastError());
    }
    const size_t nborn = (size_t)(B + 1) * k.K;
    hipLaunchKernelGGL(k_sparse_rows_clear, dim3((unsigned)std::min<size_t>((nborn + 255) / 256, 1024)), dim3(256), 0, s, k.born, nborn,
                       k.detected, (size_t)B + 1);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the detection on `frame`, which is frame s0 and row r of the pass
int slots_detect(const Slots &k, const TrackRows &R, const void *frame, bool u8, int H, int W, int window_size, int s0, int r,
                 hipStream_t s)
{
    const size_t row = (size_t)k.K;
    const SlotSide slots{R.tr + (size_t)r * 2 * row, R.vis + (size_t)r * row, R.qt, k.born + (size_t)r * row, k.detected + r, s0};
    return detect_launch(frame, u8, 1, H, W, window_size, k.q, k.md, k.K, feat_ws(k.ws, 1, H, W, k.md, k.K), nullptr, R.qxy, nullptr,
                         &slots, s);
}

// Replenished slots: a chunk is one pass of Slots; born and (the sparse engine's) residual rows come down beside the tracks.
// Residual row 0 of a later chunk is the previous chunk's last row, which is already on the host.  The chunks' detected
// rows are pieces of one [T] array that comes down once, with the last chunk: a download per chunk costs the dense engine's
// many small chunks a millisecond in all.
struct Replenished : Slots {
    unsigned char *h_born;   // the caller's [T][K], [T] and [T][K] or NULL
    int *h_detected;
    float *h_residual;
    int *d_det = nullptr;    // [T]

    int check(const Seq &seq, const void *tracks, const void *visible) const
    {
        if (!tracks || !visible || !h_born || !h_detected) return fail(OFLK_ERR_INVALID, "NULL output argument");
        if (every < 1) return fail(OFLK_ERR_INVALID, "detect_every must be >= 1 (got %d)", every);
        const int rc = check_select(*this);
        return rc ? rc : check_corner_window(seq.window_size);
    }
    int detect_every(int) const { return every; }
    static constexpr auto first = no_part;
    int setup(HostCall &call, const Seq &seq, TrackRows &R, int C)
    {
        const size_t row = (size_t)K, rows = (size_t)(C + 1) * row;
        char *d_ws = nullptr;
        int rc;
        if ((rc = call.alloc(&R.qxy, 2 * row)) || (rc = call.alloc(&R.qt, row)) ||
            (rc = call.alloc(&d_ws, feat_ws(nullptr, 1, seq.H, seq.W, md, K).bytes)) || (rc = call.alloc(&born, rows)) ||
            (rc = call.alloc(&d_det, (size_t)seq.T)) || (rc = call.alloc(&R.res, rows, h_residual != nullptr)))
            return rc;
        ws = d_ws;
        return OFLK_OK;
    }
    int begin(const TrackRows &R, int b0, int nb)
    {
        detected = d_det + b0;   // row b0 was the previous chunk's last row, which is no detection row: cleared again
        return slots_begin(*this, R, b0, nb, nullptr);
    }
    int detect(HostCall &, const Seq &seq, const TrackRows &R, const void *d_frame, int s, int r) const
    {
        return slots_detect(*this, R, d_frame, seq.u8, seq.H, seq.W, seq.window_size, s, r, nullptr);
    }
    int down(HostCall &call, const Seq &seq, const TrackRows &R, int b0, int nb, int r0) const
    {
        const size_t row = (size_t)K;
        int rc = call.to_host(h_born + (size_t)(b0 + r0) * row, born + (size_t)r0 * row, (size_t)(nb + 1 - r0) * row);
        if (!rc && b0 + nb == seq.T - 1) rc = call.to_host(h_detected, d_det, (size_t)seq.T);
        if (rc || !R.res) return rc;
        const int q0 = b0 > 0 ? 1 : 0;
        return call.to_host(h_residual + (size_t)(b0 + q0) * row, R.res + (size_t)q0 * row, (size_t)(nb + 1 - q0) * row);
    }
};
}  // namespace


OFLK_API int oflk_track_points(const float *d_uf, const float *d_vf, const float *d_ub, const float *d_vb, int B, int H, int W,
                               float alpha, float beta, int t0, const int *d_qt, const float *d_qxy, int N, float *d_tracks,
                               unsigned char *d_visible, void *stream)
{
    int rc = check_track(d_uf, d_vf, d_ub, d_vb, B, H, W, alpha, beta, nullptr, d_qxy, N, d_tracks, d_visible);
    if (rc) return rc;
    if (t0 < 0) return fail(OFLK_ERR_INVALID, "t0 must be >= 0 (got %d)", t0);
    if (reinterpret_cast<uintptr_t>(d_tracks) % 8 != 0) return fail(OFLK_ERR_INVALID, "d_tracks must be 8-byte aligned");
    return track_launch(d_uf, d_vf, d_ub, d_vb, B, H, W, alpha, beta, t0, d_qt, d_qxy, N, d_tracks, d_visible, (hipStream_t)stream);
}

OFLK_API int oflk_track_points_host(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W,
                                    float alpha, float beta, const int *qt, const float *qxy, int N, float *tracks,
                                    unsigned char *visible)
{
    int rc = check_track(uf, vf, ub, vb, B, H, W, alpha, beta, qt, qxy, N, tracks, visible);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)B * H * W, row = (size_t)N, rows = (size_t)(B + 1) * row;
    const float *in[4] = {uf, vf, ub, vb};
    float *d[4], *d_qxy, *d_tr;
    int *d_qt = nullptr;
    unsigned char *d_vis;
    for (int i = 0; i < 4; i++)
        if ((rc = call.upload(&d[i], in[i], n))) return rc;
    if ((rc = call.upload(&d_qxy, qxy, 2 * row)) || (qt && (rc = call.upload(&d_qt, qt, row))) ||
        (rc = call.alloc(&d_tr, 2 * rows)) || (rc = call.alloc(&d_vis, rows)))
        return rc;
    if ((rc = track_launch(d[0], d[1], d[2], d[3], B, H, W, alpha, beta, 0, d_qt, d_qxy, N, d_tr, d_vis, nullptr))) return rc;
    if ((rc = call.to_host(tracks, d_tr, 2 * rows)) || (rc = call.to_host(visible, d_vis, rows))) return rc;
    return call.sync();
}

OFLK_API int oflk_pyramidal_sequence_tracks(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                            float alpha, float beta, const int *qt, const float *qxy, int N, float *tracks,
                                            unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, false, T, H, W}, DenseTracks{alpha, beta},
                               GivenQueries{qt, qxy, N}, N, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_tracks_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                               int iters, float alpha, float beta, const int *qt, const float *qxy, int N,
                                               float *tracks, unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, true, T, H, W}, DenseTracks{alpha, beta},
                               GivenQueries{qt, qxy, N}, N, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                         float alpha, float beta, float quality_level, float min_distance, int max_corners,
                                         int *count, float *xy, float *score, float *tracks, unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, false, T, H, W}, DenseTracks{alpha, beta},
                               DetectOnce{quality_level, min_distance, max_corners, count, xy, score}, max_corners, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                            int iters, float alpha, float beta, float quality_level, float min_distance,
                                            int max_corners, int *count, float *xy, float *score, float *tracks,
                                            unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, true, T, H, W}, DenseTracks{alpha, beta},
                               DetectOnce{quality_level, min_distance, max_corners, count, xy, score}, max_corners, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_replenish(const float *frames, int T, int H, int W, int levels, int window_size,
                                                   int iters, float alpha, float beta, float quality_level, float min_distance,
                                                   int max_corners, int detect_every, float *tracks, unsigned char *visible,
                                                   unsigned char *born, int *detected)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, false, T, H, W}, DenseTracks{alpha, beta},
                               Replenished{{{quality_level, min_distance, max_corners, detect_every}}, born, detected, nullptr},
                               max_corners, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_replenish_u8(const unsigned char *frames, int T, int H, int W, int levels,
                                                      int window_size, int iters, float alpha, float beta, float quality_level,
                                                      float min_distance, int max_corners, int detect_every, float *tracks,
                                                      unsigned char *visible, unsigned char *born, int *detected)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, true, T, H, W}, DenseTracks{alpha, beta},
                               Replenished{{{quality_level, min_distance, max_corners, detect_every}}, born, detected, nullptr},
                               max_corners, tracks, visible);
}

// =============================================================================
// sparse pyramidal LK: points in, points out, no dense flow
// =============================================================================
namespace {
// The configuration's refusals, before any device call: levels, iterations (INVALID), the window (odd, 3..11) and the
// level sizes (every dimension >= 2: a level's linspace geometry divides by size - 1) (UNSUPPORTED)
int check_sparse_config(int H, int W, const PyrWindow &pw)
{
    const int levels = pw.levels, window_size = pw.window_size, iters = pw.iters;
    if (H < 1 || W < 1) return fail(OFLK_ERR_INVALID, "H and W must be >= 1 (got %d x %d)", H, W);
    if (levels < 1 || levels > OFLK_MAX_LEVELS)
        return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    if (iters < 1) return fail(OFLK_ERR_INVALID, "the sparse tracker needs iters >= 1 (got %d)", iters);
    if (window_size < 3 || window_size > 11 || window_size % 2 == 0)
        return fail(OFLK_ERR_UNSUPPORTED, "the sparse tracker is built for the odd windows 3 ... 11 (got %d)", window_size);
    int h = H, w = W;
    for (int l = levels - 1; l >= 0; l--) {
        if (h < 2 || w < 2)
            return fail(OFLK_ERR_UNSUPPORTED, "pyramid level %d of %dx%d would be %dx%d: the sparse tracker needs 2 x 2", l, W, H, w, h);
        h = (int)((double)h * 0.5);
        w = (int)((double)w * 0.5);
    }
    return OFLK_OK;
}

int check_sparse_test(const TrackTest &t)
{
    if (int rc = check_alpha_beta(t.alpha, t.beta)) return rc;
    if (!(t.max_residual >= 0.0f)) return fail(OFLK_ERR_INVALID, "max_residual must be >= 0 (+inf disables the test)");
    return OFLK_OK;
}

PyrWindow plan_window(const oflk_plan *p) { return {p->L, p->win, p->K}; }

// a pyramid's L levels as the sparse kernels take them: pointers, sizes and upsample_args' ratios
void sparse_levels(SparseArgs *a, int L, float *const *pyr, const int *dims)
{
    for (int l = 0; l < L; l++) {
        a->pyr[l] = pyr[l];
        a->dims[2 * l] = dims[2 * l];
        a->dims[2 * l + 1] = dims[2 * l + 1];
        if (l > 0) {
            a->sx[l] = (float)((double)dims[2 * l + 1] / (double)dims[2 * l - 1]);
            a->sy[l] = (float)((double)dims[2 * l] / (double)dims[2 * l - 2]);
        }
    }
}

// The plan's B+1 pyramids of d_frames [B+1][H][W] (build_pyramids, exact arithmetic always) and the kernel arguments
// that describe them.  Device workspace of a sparse pass: the plan's pyramid levels below the frame, nothing of frame
// size -- except where a level is too small for the fused pyramid kernel: then the blur temporaries for B+1 images and,
// for uint8 frames, their float32 copies.
int sparse_pyramids(oflk_plan *p, const void *d_frames, bool u8, hipStream_t s, SparseArgs *a)
{
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    if (u8 && u8_needs_stage(p)) {
        if ((rc = stage_u8(p, s, d_frames, nullptr, true))) return rc;
        d_frames = p->u8_stage[0];
        u8 = false;
    }
    if (pyr_first_unfused(p->dims, p->L, p->gauss) >= 0 && (rc = ensure_tmp(p, (size_t)p->B + 1))) return rc;
    PyrExtra first;
    first.u8 = u8;
    const int arith = p->arith;
    p->arith = OFLK_ARITH_EXACT;
    rc = build_pyramids(p, s, static_cast<const float *>(d_frames), nullptr, true, first);   // one buffer: no second pointer
    p->arith = arith;
    if (rc) return rc;
    *a = SparseArgs{};
    a->frames = d_frames;
    a->L = p->L; a->K = p->K; a->B = p->B; a->H = p->H; a->W = p->W;
    sparse_levels(a, p->L, p->pyr, p->dims);
    return u8 ? 1 : 0;   // > 0: the kernels read the finest level as uint8
}

// step_residual != NULL: the track kernel that also writes those rows
template <bool TRACK>
int sparse_launch(const oflk_plan *p, const SparseArgs &a, bool u8, hipStream_t s, float *step_residual = nullptr)
{
    const dim3 grid((unsigned)a.N);
    const bool built = with_half_window(p->hw, [&](auto HW) {
        with_pix(u8, [&](auto PIX) {
            using T = typename decltype(PIX)::type;
            constexpr int hw = decltype(HW)::value;
            if constexpr (!TRACK) hipLaunchKernelGGL((k_sparse_lk<hw, T>), grid, dim3(64), 0, s, a);
            else if (step_residual) hipLaunchKernelGGL((k_sparse_track_residual<hw, T>), grid, dim3(64), 0, s, a, step_residual);
            else hipLaunchKernelGGL((k_sparse_track<hw, T>), grid, dim3(64), 0, s, a);
        });
    });
    if (!built) return fail(OFLK_ERR_UNSUPPORTED, "half window %d not built", p->hw);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

int plan_sparse_tracks(oflk_plan *p, const void *d_frames, bool u8, const TrackTest &test, int t0, const int *d_qt,
                       const float *d_qxy, int N, float *d_tracks, unsigned char *d_visible, hipStream_t s)
{
    if (!p || !d_frames) return fail(OFLK_ERR_INVALID, "NULL argument");
    int rc = check_queries(nullptr, p->B + 1, d_qxy, N, d_tracks, d_visible);
    if (rc || (rc = check_sparse_test(test)) || (rc = check_sparse_config(p->H, p->W, plan_window(p)))) return rc;
    if (t0 < 0) return fail(OFLK_ERR_INVALID, "t0 must be >= 0 (got %d)", t0);
    SparseArgs a;
    if ((rc = sparse_pyramids(p, d_frames, u8, s, &a)) < 0) return rc;
    a.qt = d_qt; a.qxy = d_qxy; a.tracks = d_tracks; a.visible = d_visible;
    a.N = N; a.t0 = t0;
    a.alpha = test.alpha; a.beta = test.beta; a.max_residual = test.max_residual;
    return sparse_launch<true>(p, a, rc > 0, s);
}

// A sparse pass on a plan, one chain of launches on stream s with nothing synchronized: the plan's B+1 pyramids once
// (begin), then one track launch per segment (step).  The host driver's sparse engine and oflk_plan_sparse_klt_replenish.
struct SparsePass {
    TrackTest test;
    oflk_plan *p = nullptr;
    hipStream_t s = nullptr;
    SparseArgs base{};      // the whole pass's
    bool fine_u8 = false;   // the kernels read the finest level as uint8

    int begin(oflk_plan *plan, const void *d_frames, bool u8, hipStream_t stream)
    {
        p = plan;
        s = stream;
        const int rc = sparse_pyramids(p, d_frames, u8, s, &base);
        fine_u8 = rc > 0;
        return std::min(rc, 0);
    }
    // the segment of pairs s0 .. e-1 that begins on row r of the pass: one launch on the buffers offset to frame r (the
    // kernel's frame 0, row 0 and t0 = s0); with R.res, the kernel that also writes those rows
    int step(const TrackRows &R, int N, int s0, int e, int r) const
    {
        const size_t row = (size_t)N, fo = (size_t)r * p->H * p->W;
        SparseArgs a = base;
        a.frames = static_cast<const char *>(base.frames) + fo * (fine_u8 ? 1 : sizeof(float));
        for (int l = 0; l < p->L - 1; l++) a.pyr[l] = base.pyr[l] + (size_t)r * p->dims[2 * l] * (size_t)p->dims[2 * l + 1];
        a.B = e - s0; a.N = N; a.t0 = s0;
        a.qt = R.qt; a.qxy = R.qxy; a.tracks = R.tr + (size_t)r * 2 * row; a.visible = R.vis + (size_t)r * row;
        a.alpha = test.alpha; a.beta = test.beta; a.max_residual = test.max_residual;
        return sparse_launch<true>(p, a, fine_u8, s, R.res ? R.res + (size_t)r * row : nullptr);
    }
};

template <class PIXELS>
int sparse_lk_host(const PIXELS *prev, const PIXELS *curr, int H, int W, int levels, int window_size, int iters, const float *pts,
                   int N, float *next_pts, unsigned char *status, float *residual)
{
    int rc = check_hw(prev, curr, H, W);
    if (rc) return rc;
    if (!pts || !next_pts || !status || !residual) return fail(OFLK_ERR_INVALID, "NULL point or output argument");
    if (N < 1) return fail(OFLK_ERR_INVALID, "N must be >= 1 (got %d)", N);
    if ((rc = check_sparse_config(H, W, {levels, window_size, iters}))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t plane = (size_t)H * W, row = (size_t)N;
    PIXELS *d_frames;
    float *d_pts, *d_next, *d_res;
    unsigned char *d_st;
    oflk_plan *p = nullptr;
    if ((rc = call.alloc(&d_frames, 2 * plane)) || (rc = call.to_device(d_frames, prev, plane)) ||
        (rc = call.to_device(d_frames + plane, curr, plane)) || (rc = call.upload(&d_pts, pts, 2 * row)) ||
        (rc = call.alloc(&d_next, 2 * row)) || (rc = call.alloc(&d_st, row)) || (rc = call.alloc(&d_res, row)) ||
        (rc = host_plan(*call.c, call.dev, 1, H, W, levels, window_size, iters, &p)))
        return rc;
    SparseArgs a;
    if ((rc = sparse_pyramids(p, d_frames, sizeof(PIXELS) == 1, nullptr, &a)) < 0) return rc;
    a.pts = d_pts; a.next_pts = d_next; a.status = d_st; a.residual = d_res;
    a.N = N;
    if ((rc = sparse_launch<false>(p, a, rc > 0, nullptr))) return rc;
    if ((rc = call.to_host(next_pts, d_next, 2 * row)) || (rc = call.to_host(status, d_st, row)) ||
        (rc = call.to_host(residual, d_res, row)))
        return rc;
    return call.sync();
}

// Pairs per chunk of the sparse sequence call: a chunk holds C+1 frames and their pyramids and no flow, so it is sized by
// the frames alone (~128 MB of float32 frames: sixteen 1080p pairs, four times chunk_pairs' four), and capped at 64 pairs,
// which bounds a track launch's serial chain.  Below B exactly when the call is chunked.
int sparse_chunk_pairs(int B, int H, int W)
{
    const size_t frame = (size_t)H * W * sizeof(float);
    const int C = (int)std::min<size_t>(64, std::max<size_t>(1, ((size_t)128 << 20) / std::max<size_t>(frame, 1)));
    return std::min(B, C);
}

// The sparse engine of run_sequence_tracks: a chunk is its C+1 frames and their pyramids and no flow, a segment one
// SparsePass step
struct SparseTracks {
    SparsePass pass;
    char *frames = nullptr;   // [C+1][H][W] of the call's pixels

    int check(const Seq &seq) const
    {
        int rc = check_seq(seq);
        if (rc || (rc = check_sparse_test(pass.test))) return rc;
        return check_sparse_config(seq.H, seq.W, seq);
    }
    static int pairs(int B, int H, int W) { return sparse_chunk_pairs(B, H, W); }
    int alloc(HostCall &call, const Seq &seq, int C) { return call.alloc(&frames, (size_t)(C + 1) * seq.frame_bytes()); }
    int upload(HostCall &call, const Seq &seq, int b0, int nb)
    {
        const size_t fb = seq.frame_bytes();
        const int rc = host_plan(*call.c, call.dev, nb, seq.H, seq.W, seq.levels, seq.window_size, seq.iters, &pass.p);
        return rc ? rc : call.to_device(frames, static_cast<const char *>(seq.frames) + (size_t)b0 * fb, (size_t)(nb + 1) * fb);
    }
    int ready(const Seq &seq) { return pass.begin(pass.p, frames, seq.u8, nullptr); }
    const void *frame(const Seq &seq, int r) const { return frames + (size_t)r * seq.frame_bytes(); }
    int step(const Seq &, const TrackRows &R, int N, int s0, int e, int r) const { return pass.step(R, N, s0, e, r); }
};
}  // namespace

OFLK_API int oflk_sparse_lk(const float *prev, const float *curr, int H, int W, int levels, int window_size, int iters,
                            const float *pts, int N, float *next_pts, unsigned char *status, float *residual)
{
    return sparse_lk_host<float>(prev, curr, H, W, levels, window_size, iters, pts, N, next_pts, status, residual);
}

OFLK_API int oflk_sparse_lk_u8(const unsigned char *prev, const unsigned char *curr, int H, int W, int levels, int window_size,
                               int iters, const float *pts, int N, float *next_pts, unsigned char *status, float *residual)
{
    return sparse_lk_host<unsigned char>(prev, curr, H, W, levels, window_size, iters, pts, N, next_pts, status, residual);
}

OFLK_API int oflk_plan_sparse_tracks(oflk_plan *plan, const void *d_frames, int u8, float alpha, float beta, float max_residual,
                                     int t0, const int *d_qt, const float *d_qxy, int N, float *d_tracks,
                                     unsigned char *d_visible, void *stream)
{
    return plan_sparse_tracks(plan, d_frames, u8 != 0, {alpha, beta, max_residual}, t0, d_qt, d_qxy, N, d_tracks, d_visible,
                              (hipStream_t)stream);
}

OFLK_API int oflk_pyramidal_sequence_sparse_tracks(const float *frames, int T, int H, int W, int levels, int window_size,
                                                   int iters, float alpha, float beta, float max_residual, const int *qt,
                                                   const float *qxy, int N, float *tracks, unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, false, T, H, W}, SparseTracks{{{alpha, beta, max_residual}}},
                               GivenQueries{qt, qxy, N}, N, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_sparse_tracks_u8(const unsigned char *frames, int T, int H, int W, int levels,
                                                      int window_size, int iters, float alpha, float beta, float max_residual,
                                                      const int *qt, const float *qxy, int N, float *tracks,
                                                      unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, true, T, H, W}, SparseTracks{{{alpha, beta, max_residual}}},
                               GivenQueries{qt, qxy, N}, N, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_sparse(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                                float alpha, float beta, float max_residual, float quality_level,
                                                float min_distance, int max_corners, int *count, float *xy, float *score,
                                                float *tracks, unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, false, T, H, W}, SparseTracks{{{alpha, beta, max_residual}}},
                               DetectOnce{quality_level, min_distance, max_corners, count, xy, score}, max_corners, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_sparse_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                                   int iters, float alpha, float beta, float max_residual, float quality_level,
                                                   float min_distance, int max_corners, int *count, float *xy, float *score,
                                                   float *tracks, unsigned char *visible)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, true, T, H, W}, SparseTracks{{{alpha, beta, max_residual}}},
                               DetectOnce{quality_level, min_distance, max_corners, count, xy, score}, max_corners, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_sparse_replenish(const float *frames, int T, int H, int W, int levels, int window_size,
                                                          int iters, float alpha, float beta, float max_residual,
                                                          float quality_level, float min_distance, int max_corners,
                                                          int detect_every, float *tracks, unsigned char *visible,
                                                          unsigned char *born, int *detected, float *residual)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, false, T, H, W}, SparseTracks{{{alpha, beta, max_residual}}},
                               Replenished{{{quality_level, min_distance, max_corners, detect_every}}, born, detected, residual},
                               max_corners, tracks, visible);
}

OFLK_API int oflk_pyramidal_sequence_klt_sparse_replenish_u8(const unsigned char *frames, int T, int H, int W, int levels,
                                                             int window_size, int iters, float alpha, float beta,
                                                             float max_residual, float quality_level, float min_distance,
                                                             int max_corners, int detect_every, float *tracks,
                                                             unsigned char *visible, unsigned char *born, int *detected,
                                                             float *residual)
{
    return run_sequence_tracks(Seq{{levels, window_size, iters}, frames, true, T, H, W}, SparseTracks{{{alpha, beta, max_residual}}},
                               Replenished{{{quality_level, min_distance, max_corners, detect_every}}, born, detected, residual},
                               max_corners, tracks, visible);
}

OFLK_API int oflk_plan_sparse_klt_replenish(oflk_plan *plan, const void *d_frames, int u8, float alpha, float beta,
                                            float max_residual, float quality_level, float min_distance, int max_corners,
                                            int detect_every, int t0, void *d_workspace, size_t workspace_bytes, int *d_qt,
                                            float *d_qxy, float *d_tracks, unsigned char *d_visible, unsigned char *d_born,
                                            int *d_detected, float *d_residual, void *stream)
{
    if (!plan || !d_frames) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (!d_workspace || !d_qt || !d_qxy || !d_tracks || !d_visible || !d_born || !d_detected)
        return fail(OFLK_ERR_INVALID, "NULL workspace, slot state or output argument");
    const TrackTest test{alpha, beta, max_residual};
    const Selection select{quality_level, min_distance, max_corners, detect_every};
    int rc = check_sparse_test(test);
    if (rc || (rc = check_sparse_config(plan->H, plan->W, plan_window(plan))) || (rc = check_select(select))) return rc;
    if (detect_every < 1) return fail(OFLK_ERR_INVALID, "detect_every must be >= 1 (got %d)", detect_every);
    if (t0 < 0 || t0 > INT_MAX - plan->B) return fail(OFLK_ERR_INVALID, "t0 must be in [0, INT_MAX - B] (got %d)", t0);
    const size_t need = feat_ws(nullptr, 1, plan->H, plan->W, min_distance, max_corners).bytes;
    if (workspace_bytes < need)
        return fail(OFLK_ERR_INVALID, "workspace of %zu bytes, %zu needed (oflk_replenish_features_workspace)", workspace_bytes,
                    need);
    if (reinterpret_cast<uintptr_t>(d_workspace) % 256 != 0 || reinterpret_cast<uintptr_t>(d_qxy) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(d_tracks) % 8 != 0)
        return fail(OFLK_ERR_INVALID, "d_workspace must be 256-byte aligned, d_qxy and d_tracks 8-byte aligned");
    // the plan's B+1 pyramids once, then the pairs t0 .. t0+B-1 as the host driver walks a chunk's: one chain of launches
    const hipStream_t s = (hipStream_t)stream;
    const Slots k{select, d_workspace, d_born, d_detected};
    const TrackRows R{d_qt, d_qxy, d_tracks, d_visible, d_residual};
    const size_t fb = (size_t)plan->H * plan->W * (u8 ? 1 : sizeof(float));
    SparsePass pass{test};
    if ((rc = pass.begin(plan, d_frames, u8 != 0, s)) || (rc = slots_begin(k, R, t0, plan->B, s))) return rc;
    return walk_segments(
        t0, plan->B, detect_every,
        [&](int s0, int r) {
            return slots_detect(k, R, static_cast<const char *>(d_frames) + r * fb, u8 != 0, plan->H, plan->W, plan->win, s0, r, s);
        },
        [&](int s0, int e, int r) { return pass.step(R, max_corners, s0, e, r); });
}

// =============================================================================
// global motion from correspondences: RANSAC and refit, four models (oflk_motion.hpp, oflk_homography.hpp)
// =============================================================================
namespace {
// The workspace of the fit, 256-byte aligned pieces: M [S], the compacted correspondences [S][N], score [S][Hn] and the
// hypotheses' models [S][Hn][nc] -- nc = 6 coefficients, 9 for the homography fit
struct MotionWs {
    int *M;
    float4 *pts;
    int *score;
    float *hmodel;
    size_t bytes;
};

MotionWs motion_ws(void *base, int S, int N, int Hn, int nc = 6)
{
    MotionWs v{};
    auto take = [&](auto *&p, size_t n) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(base) + v.bytes);
        v.bytes += align256(n * sizeof(*p));
    };
    const size_t nS = (size_t)S;
    take(v.M, nS);
    take(v.pts, nS * (size_t)N);
    take(v.score, nS * (size_t)Hn);
    take(v.hmodel, nS * (size_t)Hn * (size_t)nc);
    return v;
}

// what every form of a fit refuses about its RANSAC parameters
int check_ransac(int hypotheses, float threshold)
{
    if (hypotheses < 1 || hypotheses > OFLK_MOTION_MAX_HYPOTHESES)
        return fail(OFLK_ERR_INVALID, "hypotheses must be in [1, %d] (got %d)", OFLK_MOTION_MAX_HYPOTHESES, hypotheses);
    if (!(std::isfinite(threshold) && threshold > 0.0f))
        return fail(OFLK_ERR_INVALID, "threshold must be finite and > 0 (got %g)", (double)threshold);
    return OFLK_OK;
}

// what every form of the motion fit refuses about its parameters
int check_motion(int model, int hypotheses, float threshold)
{
    if (model != OFLK_MOTION_TRANSLATION && model != OFLK_MOTION_SIMILARITY && model != OFLK_MOTION_AFFINE)
        return fail(OFLK_ERR_INVALID, "unknown motion model %d", model);
    return check_ransac(hypotheses, threshold);
}
int check_ransac(const FitConfig &f) { return check_ransac(f.hypotheses, f.threshold); }   // f.model is an internal code
int check_motion(const FitConfig &f) { return check_motion(f.model, f.hypotheses, f.threshold); }

int check_motion_shape(int S, int N)
{
    if (S < 1 || N < 1) return fail(OFLK_ERR_INVALID, "steps and correspondences must be >= 1 (got %d steps of %d)", S, N);
    return OFLK_OK;
}

int check_motion_workspace(const void *ws, size_t bytes, int S, int N, int Hn, int model)
{
    if (!ws) return fail(OFLK_ERR_INVALID, "NULL workspace");
    const size_t need = motion_ws(nullptr, S, N, Hn, motion_coeffs(model)).bytes;
    if (bytes < need)
        return fail(OFLK_ERR_INVALID, "workspace of %zu bytes, %zu needed (%s)", bytes, need,
                    model == kMotionHomography ? "oflk_homography_workspace" : "oflk_motion_workspace");
    if (!aligned(ws, 256)) return fail(OFLK_ERR_INVALID, "d_workspace must be 256-byte aligned");
    return OFLK_OK;
}

// What a step reads, at [s][N]: NULL masks do not decide.
struct MotionIn {
    const float *src, *dst;
    const unsigned char *va, *vb, *born;
};

// the T-1 steps of [T][K] track arrays: row t+1 of an array is row t of the array that begins K elements later, so one
// stride serves every input
MotionIn motion_rows(const float *d_tracks, const unsigned char *d_visible, const unsigned char *d_born, int K)
{
    return {d_tracks, d_tracks + 2 * (size_t)K, d_visible, d_visible + (size_t)K, d_born ? d_born + (size_t)K : nullptr};
}

// The three launches of S steps on stream s; the arguments are checked.  `model` is an internal code (kMotionTranslation ..
// kMotionHomography); ws is motion_ws with its motion_coeffs(model) coefficients per model, as is d_model [S][coeffs]
int motion_launch(const MotionIn &in, int S, int N, unsigned index0, int model, int Hn, float threshold, unsigned seed,
                  const MotionWs &ws, float *d_model, unsigned char *d_inlier, int *d_counts, hipStream_t s)
{
    MotionArgs a{};
    a.src = reinterpret_cast<const float2 *>(in.src);
    a.dst = reinterpret_cast<const float2 *>(in.dst);
    a.va = in.va; a.vb = in.vb; a.born = in.born;
    a.S = S; a.N = N; a.Hn = Hn;
    a.index0 = index0; a.seed = seed;
    a.thr2 = threshold * threshold;
    a.M = ws.M; a.pts = ws.pts; a.score = ws.score; a.hmodel = ws.hmodel;
    a.model = d_model; a.inlier = d_inlier; a.counts = d_counts;
    const unsigned steps = (unsigned)std::min(S, 65535);
    hipLaunchKernelGGL(k_motion_compact, dim3(steps), dim3(kMotionCompact), 0, s, a);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((Hn + kMotionWaves - 1) / kMotionWaves), steps);
    const bool built = with_int<kMotionTranslation, kMotionSimilarity, kMotionAffine, kMotionHomography>(model, [&](auto MODEL) {
        hipLaunchKernelGGL(k_motion_score<decltype(MODEL)::value>, grid, dim3(64 * kMotionWaves), 0, s, a);
        hipLaunchKernelGGL(k_motion_refit<decltype(MODEL)::value>, dim3(steps), dim3(kMotionLanes), 0, s, a);
    });
    if (!built) return fail(OFLK_ERR_INVALID, "unknown motion model %d", model);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// The fit an entry point asks for.  The motion fit's entry points pass their `model` argument on, and the values
// check_motion accepts are internal codes as they stand; the homography's have no such argument
struct FitKind {
    bool homography;
    int model;
    int code() const { return homography ? kMotionHomography : model; }
    int check(int hypotheses, float threshold) const
    {
        return homography ? check_ransac(hypotheses, threshold) : check_motion(model, hypotheses, threshold);
    }
};
constexpr FitKind kHomographyFit{true, 0};

// ---- one body for each form of an entry point ----
int fit_workspace(int model, int S, int N, int hypotheses, size_t *bytes)
{
    if (!bytes) return fail(OFLK_ERR_INVALID, "NULL bytes");
    int rc = check_motion_shape(S, N);
    if (rc || (rc = check_ransac(hypotheses, 1.0f))) return rc;
    *bytes = motion_ws(nullptr, S, N, hypotheses, motion_coeffs(model)).bytes;
    return OFLK_OK;
}

// the device forms behind their shape and parameter checks: `in` holds S steps of N
int fit_device(const MotionIn &in, const char *alignment, int S, int N, int index0, int model, int hypotheses, float threshold,
               unsigned seed, void *d_workspace, size_t workspace_bytes, float *d_model, unsigned char *d_inlier, int *d_counts,
               void *stream)
{
    if (!in.src || !in.dst || !d_model || !d_inlier || !d_counts) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    if (!aligned(in.src, 8) || !aligned(in.dst, 8)) return fail(OFLK_ERR_INVALID, "%s must be 8-byte aligned", alignment);
    if (int rc = check_motion_workspace(d_workspace, workspace_bytes, S, N, hypotheses, model)) return rc;
    return motion_launch(in, S, N, (unsigned)index0, model, hypotheses, threshold, seed,
                         motion_ws(d_workspace, S, N, hypotheses, motion_coeffs(model)), d_model, d_inlier, d_counts,
                         (hipStream_t)stream);
}

int estimate_device(FitKind fit, const float *d_src, const float *d_dst, const unsigned char *d_valid, int S, int N, int step0,
                    int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes, float *d_model,
                    unsigned char *d_inlier, int *d_counts, void *stream)
{
    int rc = check_motion_shape(S, N);
    if (rc || (rc = fit.check(hypotheses, threshold))) return rc;
    return fit_device({d_src, d_dst, d_valid, nullptr, nullptr}, "d_src and d_dst", S, N, step0, fit.code(), hypotheses, threshold, seed,
                      d_workspace, workspace_bytes, d_model, d_inlier, d_counts, stream);
}

int tracks_device(FitKind fit, const float *d_tracks, const unsigned char *d_visible, const unsigned char *d_born, int T, int K, int t0,
                  int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes, float *d_model,
                  unsigned char *d_inlier, int *d_counts, void *stream)
{
    if (T < 2) return fail(OFLK_ERR_INVALID, "T must be >= 2 (got %d)", T);
    int rc = check_motion_shape(T - 1, K);
    if (rc || (rc = fit.check(hypotheses, threshold))) return rc;
    if (!d_tracks || !d_visible) return fail(OFLK_ERR_INVALID, "NULL input or output argument");   // ahead of the row cut
    return fit_device(motion_rows(d_tracks, d_visible, d_born, K), "d_tracks", T - 1, K, t0, fit.code(), hypotheses, threshold, seed,
                      d_workspace, workspace_bytes, d_model, d_inlier, d_counts, stream);
}

int estimate_host(FitKind fit, const float *src, const float *dst, const unsigned char *valid, int S, int N, int step0, int hypotheses,
                  float threshold, unsigned seed, float *model_out, unsigned char *inlier, int *counts)
{
    int rc = check_motion_shape(S, N);
    if (rc || (rc = fit.check(hypotheses, threshold))) return rc;
    const int model = fit.code();
    const size_t nc = (size_t)motion_coeffs(model);
    if (!src || !dst || !model_out || !inlier || !counts) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)S * (size_t)N;
    float *d_src, *d_dst, *d_model;
    unsigned char *d_valid = nullptr, *d_inl;
    char *d_ws;
    int *d_cnt;
    if ((rc = call.upload(&d_src, src, 2 * n)) || (rc = call.upload(&d_dst, dst, 2 * n)) ||
        (valid && (rc = call.upload(&d_valid, valid, n))) ||
        (rc = call.alloc(&d_ws, motion_ws(nullptr, S, N, hypotheses, (int)nc).bytes)) || (rc = call.alloc(&d_model, nc * (size_t)S)) ||
        (rc = call.alloc(&d_inl, n)) || (rc = call.alloc(&d_cnt, 3 * (size_t)S)))
        return rc;
    if ((rc = motion_launch({d_src, d_dst, d_valid, nullptr, nullptr}, S, N, (unsigned)step0, model, hypotheses, threshold, seed,
                            motion_ws(d_ws, S, N, hypotheses, (int)nc), d_model, d_inl, d_cnt, nullptr)))
        return rc;
    if ((rc = call.to_host(model_out, d_model, nc * (size_t)S)) || (rc = call.to_host(inlier, d_inl, n)) ||
        (rc = call.to_host(counts, d_cnt, 3 * (size_t)S)))
        return rc;
    return call.sync();
}
}  // namespace

OFLK_API int oflk_motion_workspace(int S, int N, int hypotheses, size_t *bytes)
{
    return fit_workspace(kMotionAffine, S, N, hypotheses, bytes);
}

OFLK_API int oflk_estimate_motion(const float *d_src, const float *d_dst, const unsigned char *d_valid, int S, int N, int step0,
                                  int model, int hypotheses, float threshold, unsigned seed, void *d_workspace,
                                  size_t workspace_bytes, float *d_model, unsigned char *d_inlier, int *d_counts, void *stream)
{
    return estimate_device({false, model}, d_src, d_dst, d_valid, S, N, step0, hypotheses, threshold, seed, d_workspace, workspace_bytes,
                           d_model, d_inlier, d_counts, stream);
}

OFLK_API int oflk_tracks_motion(const float *d_tracks, const unsigned char *d_visible, const unsigned char *d_born, int T, int K,
                                int t0, int model, int hypotheses, float threshold, unsigned seed, void *d_workspace,
                                size_t workspace_bytes, float *d_model, unsigned char *d_inlier, int *d_counts, void *stream)
{
    return tracks_device({false, model}, d_tracks, d_visible, d_born, T, K, t0, hypotheses, threshold, seed, d_workspace,
                         workspace_bytes, d_model, d_inlier, d_counts, stream);
}

OFLK_API int oflk_estimate_motion_host(const float *src, const float *dst, const unsigned char *valid, int S, int N, int step0,
                                       int model, int hypotheses, float threshold, unsigned seed, float *model_out,
                                       unsigned char *inlier, int *counts)
{
    return estimate_host({false, model}, src, dst, valid, S, N, step0, hypotheses, threshold, seed, model_out, inlier, counts);
}

// ---- the homography fit: the same four forms with the internal model code ----
OFLK_API int oflk_homography_workspace(int S, int N, int hypotheses, size_t *bytes)
{
    return fit_workspace(kMotionHomography, S, N, hypotheses, bytes);
}

OFLK_API int oflk_estimate_homography(const float *d_src, const float *d_dst, const unsigned char *d_valid, int S, int N, int step0,
                                      int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes,
                                      float *d_model, unsigned char *d_inlier, int *d_counts, void *stream)
{
    return estimate_device(kHomographyFit, d_src, d_dst, d_valid, S, N, step0, hypotheses, threshold, seed, d_workspace,
                           workspace_bytes, d_model, d_inlier, d_counts, stream);
}

OFLK_API int oflk_tracks_homography(const float *d_tracks, const unsigned char *d_visible, const unsigned char *d_born, int T, int K,
                                    int t0, int hypotheses, float threshold, unsigned seed, void *d_workspace,
                                    size_t workspace_bytes, float *d_model, unsigned char *d_inlier, int *d_counts, void *stream)
{
    return tracks_device(kHomographyFit, d_tracks, d_visible, d_born, T, K, t0, hypotheses, threshold, seed, d_workspace,
                         workspace_bytes, d_model, d_inlier, d_counts, stream);
}

OFLK_API int oflk_estimate_homography_host(const float *src, const float *dst, const unsigned char *valid, int S, int N, int step0,
                                           int hypotheses, float threshold, unsigned seed, float *model_out, unsigned char *inlier,
                                           int *counts)
{
    return estimate_host(kHomographyFit, src, dst, valid, S, N, step0, hypotheses, threshold, seed, model_out, inlier, counts);
}

// =============================================================================
// video stabilisation: the smoothed trajectory and the affine warp (oflk_stabilize.hpp)
// =============================================================================
namespace {
int check_stab_window(const double *weights, int radius)
{
    if (radius < 0 || radius > OFLK_STABILIZE_MAX_RADIUS)
        return fail(OFLK_ERR_INVALID, "radius must be in [0, %d] (got %d)", OFLK_STABILIZE_MAX_RADIUS, radius);
    if (!weights) return fail(OFLK_ERR_INVALID, "NULL weights");
    for (int i = 0; i <= radius; i++)
        if (!(std::isfinite(weights[i]) && weights[i] > 0.0))
            return fail(OFLK_ERR_INVALID, "weights[%d] must be finite and > 0 (got %g)", i, weights[i]);
    return OFLK_OK;
}
int check_stab_window(const TrajWindow &w) { return check_stab_window(w.weights, w.radius); }

int check_trajectory(const void *model, int T, const double *weights, int radius, const void *correction, const void *map)
{
    if (T < 1) return fail(OFLK_ERR_INVALID, "T must be >= 1 (got %d)", T);
    if (int rc = check_stab_window(weights, radius)) return rc;
    if ((T > 1 && !model) || !correction || !map) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    return OFLK_OK;
}

// the one launch of the trajectory on stream s; the arguments are checked
int trajectory_launch(const float *d_model, const int *d_counts, int T, const double *weights, int radius, float *d_correction,
                      double *d_map, unsigned char *d_held, hipStream_t s)
{
    StabWeights wt{};
    for (int i = 0; i <= radius; i++) wt.w[i] = weights[i];
    hipLaunchKernelGGL(k_stab_trajectory, dim3((unsigned)((T + kStabBlock - 1) / kStabBlock)), dim3(kStabBlock), 0, s, d_model,
                       d_counts, T, radius, wt, d_correction, d_map, d_held);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// ---- frame layouts ----
// How a frame of the warps, the sequence stabilisers and the online stabiliser lies in memory.  The layouts share one host
// path (below the NV12 launcher: warp_launch, warp_chunks, warp_host, warp_device, stabilize_sequence), and every function
// that tells them apart does so in one switch with one `case` a layout.
enum class FrameKind { Planar, Packed, Nv12 };

struct FrameLayout {
    FrameKind kind;
    int pix_bytes;   // Planar: 1 (uint8) or 4 (float32) bytes a pixel; Packed and Nv12 are bytes
    int channels;    // Packed: 3 or 4 interleaved bytes a pixel; else 0
    int order;       // Packed: OFLK_ORDER_*, what the luma weighs
    int siting;      // Nv12: OFLK_SITING_*

    static FrameLayout planar(bool u8) { return {FrameKind::Planar, u8 ? 1 : 4, 0, OFLK_ORDER_RGB, OFLK_SITING_LEFT}; }
    static FrameLayout packed(int channels, int order) { return {FrameKind::Packed, 1, channels, order, OFLK_SITING_LEFT}; }
    static FrameLayout nv12(int siting) { return {FrameKind::Nv12, 1, 0, OFLK_ORDER_RGB, siting}; }

    size_t inside_bytes(int H, int W) const { return (size_t)H * (size_t)W; }   // the mask is a byte a pixel of every layout
    size_t frame_bytes(int H, int W) const
    {
        const size_t px = (size_t)H * (size_t)W;
        switch (kind) {
        case FrameKind::Planar: return px * (size_t)pix_bytes;
        case FrameKind::Packed: return px * (size_t)channels;
        case FrameKind::Nv12: return px + px / 2;   // Y[H][W], then UV[H/2][W/2][2]
        }
        return 0;
    }
};

int check_channels(int channels)
{
    if (channels != 3 && channels != 4) return fail(OFLK_ERR_INVALID, "channels must be 3 or 4 (got %d)", channels);
    return OFLK_OK;
}

int check_order(int order)
{
    if (order != OFLK_ORDER_RGB && order != OFLK_ORDER_BGR)
        return fail(OFLK_ERR_INVALID, "order must be OFLK_ORDER_RGB or OFLK_ORDER_BGR (got %d)", order);
    return OFLK_OK;
}

int check_nv12_shape(int H, int W, int siting)
{
    if (H < 4 || W < 4 || H % 2 || W % 2) return fail(OFLK_ERR_INVALID, "NV12 frames need even H and W >= 4 (got %d x %d)", H, W);
    if (siting != OFLK_SITING_LEFT && siting != OFLK_SITING_CENTER)
        return fail(OFLK_ERR_INVALID, "siting must be OFLK_SITING_LEFT or OFLK_SITING_CENTER (got %d)", siting);
    return OFLK_OK;
}

// what a layout refuses of its own parameters and of the shape it needs: the first refusals of every call that names one
int check_layout(const FrameLayout &L, int H, int W)
{
    switch (L.kind) {
    case FrameKind::Planar: break;
    case FrameKind::Packed:
        if (int rc = check_channels(L.channels)) return rc;
        return check_order(L.order);
    case FrameKind::Nv12: return check_nv12_shape(H, W, L.siting);
    }
    return OFLK_OK;
}

// The frame refusals of a layout, in one order for every call that takes frames (tools/warp_host_check.hip holds the order and
// the texts).  no_map: the call has a map and it is NULL (a call without one leaves it false): a planar call refuses that
// with its other pointers, ahead of the size limits, a packed or NV12 call behind them.
int check_frames(const FrameLayout &L, const void *frames, int F, int H, int W, const void *out, bool no_map = false)
{
    if (int rc = check_layout(L, H, W)) return rc;
    if (F < 1) return fail(OFLK_ERR_INVALID, "F must be >= 1 (got %d)", F);
    if (H < 2 || W < 2) return fail(OFLK_ERR_INVALID, "H and W must be >= 2 (got %d x %d)", H, W);
    if (!frames || !out || (L.kind == FrameKind::Planar && no_map)) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    if (int rc = check_hw(frames, out, H, W)) return rc;   // H W < 2^30, so an NV12 frame's H W 3 / 2 bytes are counted by 32-bit offsets
    if (L.kind == FrameKind::Packed && L.frame_bytes(H, W) >= ((size_t)1 << 31))
        return fail(OFLK_ERR_UNSUPPORTED, "packed frames of 2^31 bytes or more are not supported");   // 32-bit byte offsets
    if (no_map) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    return OFLK_OK;
}

// warp_frames' grid, which the packed warp shares: 4 rows of 64 lanes a block, kWarpPx pixels a lane, the frames in z
dim3 warp_grid(int F, int H, int W)
{
    return dim3((unsigned)((H + 3) / 4), (unsigned)((W + 64 * kWarpPx - 1) / (64 * kWarpPx)), (unsigned)std::min(F, 65535));
}

// the one launch of the planar warp of F frames on stream s; the arguments are checked.  persp: d_map is [F][9] and the kernel
// k_warp_perspective
template <class PIX>
int warp_planar_launch(bool persp, const PIX *d_frames, int F, int H, int W, const double *d_map, PIX *d_out, unsigned char *d_inside,
                       hipStream_t s)
{
    WarpAffineArgs<PIX> a{};
    a.in = d_frames; a.map = d_map; a.out = d_out; a.inside = d_inside;
    a.F = F; a.H = H; a.W = W;
    const bool vec = W % kWarpPx == 0 && aligned(d_out, (unsigned)(kWarpPx * sizeof(PIX))) && (!d_inside || aligned(d_inside, kWarpPx));
    with_bool(persp, [&](auto PERSP) {
        with_bool(vec, [&](auto VEC) {
            if constexpr (decltype(PERSP)::value)
                hipLaunchKernelGGL((k_warp_perspective<PIX, decltype(VEC)::value>), warp_grid(F, H, W), dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL((k_warp_affine<PIX, decltype(VEC)::value>), warp_grid(F, H, W), dim3(256), 0, s, a);
        });
    });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// oflk_stabilize_sequence and its packed and NV12 forms: pass 1 is the replenish call itself (its chunk loop; only rows come
// down, into this call's own arrays); the rows go up again for the fit and the trajectory of all T frames, and pass 2 warps
// the frames chunk by chunk.
// What the sequence calls refuse behind their frames, before any device call
// the replenish call's own refusals, ahead of the arrays of a call that runs it as its pass 1 (it repeats them)
int check_klt(int H, int W, const KltConfig &klt)
{
    if (klt.select.every < 1) return fail(OFLK_ERR_INVALID, "detect_every must be >= 1 (got %d)", klt.select.every);
    int rc = check_select(klt.select);
    if (rc || (rc = check_sparse_test(klt.test))) return rc;
    return check_sparse_config(H, W, klt.pyr);
}

int check_stabilize_config(int H, int W, const KltConfig &klt, const FitConfig &fit, const TrajWindow &window)
{
    int rc = check_motion(fit);
    if (rc || (rc = check_stab_window(window))) return rc;
    return check_klt(H, W, klt);
}

// What the sequence stabilisers and the mosaics do up to and including the fit's launch, on checked grey frames: pass 1 is
// the replenish call itself (its chunk loop; only rows come down, into the host arrays here, which live as long as the
// caller keeps this); then `call` begins, the rows go up again and the fit of the internal `model` code runs over the T-1
// steps on the null stream.  Nothing is synchronised.
struct SequenceFit {
    std::vector<float> tracks;
    std::vector<unsigned char> visible, born;
    std::vector<int> detected;
    float *d_model = nullptr;   // [T-1][motion_coeffs(model)]
    int *d_counts = nullptr;    // [T-1][3]

    int run(HostCall &call, const void *frames, bool u8, int T, int H, int W, const KltConfig &klt, const FitConfig &fit)
    {
        int rc;
        const int K = klt.select.K;
        const size_t row = (size_t)K, nT = (size_t)T, S = nT - 1;
        try {
            tracks.resize(nT * 2 * row);
            visible.resize(nT * row);
            born.resize(nT * row);
            detected.resize(nT);
        } catch (const std::exception &) {
            return fail(OFLK_ERR_NOMEM, "no host memory for the rows of %d frames of %d slots", T, K);
        }
        if ((rc = run_sequence_tracks(Seq{klt.pyr, frames, u8, T, H, W}, SparseTracks{{klt.test}},
                                      Replenished{{klt.select}, born.data(), detected.data(), nullptr}, K, tracks.data(), visible.data())))
            return rc;
        if ((rc = call.begin())) return rc;
        float *d_tr;
        unsigned char *d_vis, *d_born, *d_inl;
        char *d_ws;
        const int nc = motion_coeffs(fit.model);
        if ((rc = call.upload(&d_tr, (const float *)tracks.data(), nT * 2 * row)) ||
            (rc = call.upload(&d_vis, (const unsigned char *)visible.data(), nT * row)) ||
            (rc = call.upload(&d_born, (const unsigned char *)born.data(), nT * row)) ||
            (rc = call.alloc(&d_ws, motion_ws(nullptr, T - 1, K, fit.hypotheses, nc).bytes)) ||
            (rc = call.alloc(&d_model, (size_t)nc * S)) || (rc = call.alloc(&d_inl, S * row)) || (rc = call.alloc(&d_counts, 3 * S)))
            return rc;
        return motion_launch(motion_rows(d_tr, d_vis, d_born, K), T - 1, K, 0u, fit.model, fit.hypotheses, fit.threshold, fit.seed,
                             motion_ws(d_ws, T - 1, K, fit.hypotheses, nc), d_model, d_inl, d_counts, nullptr);
    }
};

// Pass 1 and the trajectory of a sequence call on the checked grey frames: begins `call`, leaves the maps of all T frames in
// its *d_map_out [T][6] and sends the four small outputs on their way (the caller's last chunk synchronises)
int stabilize_maps(HostCall &call, const void *frames, bool u8, int T, int H, int W, const KltConfig &klt, const FitConfig &fit,
                   const TrajWindow &window, float *correction, float *model_out, int *counts_out, unsigned char *held,
                   double **d_map_out)
{
    int rc;
    const size_t nT = (size_t)T, S = nT - 1;
    SequenceFit steps;
    if ((rc = steps.run(call, frames, u8, T, H, W, klt, fit))) return rc;
    float *const d_model = steps.d_model, *d_corr;
    int *const d_cnt = steps.d_counts;
    unsigned char *d_held;
    double *d_map;
    if ((rc = call.alloc(&d_corr, 6 * nT)) || (rc = call.alloc(&d_map, 6 * nT)) || (rc = call.alloc(&d_held, S)) ||
        (rc = trajectory_launch(d_model, d_cnt, T, window.weights, window.radius, d_corr, d_map, d_held, nullptr)))
        return rc;
    if ((correction && (rc = call.to_host(correction, d_corr, 6 * nT))) || (model_out && (rc = call.to_host(model_out, d_model, 6 * S))) ||
        (counts_out && (rc = call.to_host(counts_out, d_cnt, 3 * S))) || (held && (rc = call.to_host(held, d_held, S))))
        return rc;
    *d_map_out = d_map;
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_stabilize_trajectory(const float *d_model, const int *d_counts, int T, const double *weights, int radius,
                                       float *d_correction, double *d_map, unsigned char *d_held, void *stream)
{
    if (int rc = check_trajectory(d_model, T, weights, radius, d_correction, d_map)) return rc;
    if (!aligned(d_map, 8)) return fail(OFLK_ERR_INVALID, "d_map must be 8-byte aligned");
    return trajectory_launch(d_model, d_counts, T, weights, radius, d_correction, d_map, d_held, (hipStream_t)stream);
}


OFLK_API int oflk_stabilize_trajectory_host(const float *model, const int *counts, int T, const double *weights, int radius,
                                            float *correction, double *map, unsigned char *held)
{
    int rc = check_trajectory(model, T, weights, radius, correction, map);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t nT = (size_t)T, S = nT - 1;
    float *d_model = nullptr, *d_corr;
    int *d_cnt = nullptr;
    double *d_map;
    unsigned char *d_held;
    if ((S && (rc = call.upload(&d_model, model, 6 * S))) || (S && counts && (rc = call.upload(&d_cnt, counts, 3 * S))) ||
        (rc = call.alloc(&d_corr, 6 * nT)) || (rc = call.alloc(&d_map, 6 * nT)) || (rc = call.alloc(&d_held, S, held && S)))
        return rc;
    if ((rc = trajectory_launch(d_model, d_cnt, T, weights, radius, d_corr, d_map, d_held, nullptr))) return rc;
    if ((rc = call.to_host(correction, d_corr, 6 * nT)) || (rc = call.to_host(map, d_map, 6 * nT)) ||
        (d_held && (rc = call.to_host(held, d_held, S))))
        return rc;
    return call.sync();
}

// =============================================================================
// colour video: interleaved bytes [F][H][W][C] -- luma and the packed warp's launch (oflk_colour.hpp)
// =============================================================================
namespace {
// the one launch of the luma of F frames on stream s; the arguments are checked
int luma_launch(const unsigned char *d_frames, int F, int H, int W, int channels, int order, unsigned char *d_luma, hipStream_t s)
{
    LumaArgs a{};
    a.in = d_frames; a.out = d_luma;
    a.n = (size_t)F * (size_t)H * (size_t)W;
    a.bgr = order == OFLK_ORDER_BGR;
    const bool vec = W % kLumaPx == 0 && aligned(d_frames, channels == 4 ? 16 : 4) && aligned(d_luma, 4);
    const size_t work = vec ? a.n / kLumaPx : a.n;
    const dim3 grid((unsigned)std::min<size_t>((work + kLumaBlock - 1) / kLumaBlock, (size_t)65535 * 16));
    with_int<3, 4>(channels, [&](auto C) {
        with_bool(vec, [&](auto VEC) {
            hipLaunchKernelGGL((k_luma<decltype(C)::value, decltype(VEC)::value>), grid, dim3(kLumaBlock), 0, s, a);
        });
    });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the one launch of the packed warp of F frames on stream s; the arguments are checked
int warp_packed_launch(bool persp, const unsigned char *d_frames, int F, int H, int W, int channels, const double *d_map,
                       unsigned char *d_out, unsigned char *d_inside, hipStream_t s)
{
    WarpPackedArgs a{};
    a.in = d_frames; a.map = d_map; a.out = d_out; a.inside = d_inside;
    a.F = F; a.H = H; a.W = W;
    // a lane's store: three dwords (C = 3) or one dwordx4 (C = 4), and the inside dword
    const bool vec = W % kWarpPx == 0 && aligned(d_out, channels == 4 ? 16 : 4) &&
                     (!d_inside || aligned(d_inside, kWarpPx));
    with_int<3, 4>(channels, [&](auto C) {
        with_bool(persp, [&](auto PERSP) {
            with_bool(vec, [&](auto VEC) {
                hipLaunchKernelGGL((k_warp_packed<decltype(C)::value, decltype(PERSP)::value, decltype(VEC)::value>), warp_grid(F, H, W),
                                   dim3(256), 0, s, a);
            });
        });
    });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the luma of F packed host frames in the warp's chunks: a chunk goes up, is converted and its luma comes down
int luma_chunks(HostCall &call, const unsigned char *frames, int F, int H, int W, int channels, int order, unsigned char *luma)
{
    const int C = sparse_chunk_pairs(F, H, W);
    const size_t plane = (size_t)H * W, fb = plane * (size_t)channels;
    unsigned char *d_in = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = call.alloc(&d_in, (size_t)C * fb)) || (rc = call.alloc(&d_out, (size_t)C * plane))) return rc;
    for (int f0 = 0; f0 < F; f0 += C) {
        const int n = std::min(C, F - f0);
        if ((rc = call.to_device(d_in, frames + (size_t)f0 * fb, (size_t)n * fb)) ||
            (rc = luma_launch(d_in, n, H, W, channels, order, d_out, nullptr)) ||
            (rc = call.to_host(luma + (size_t)f0 * plane, d_out, (size_t)n * plane)) || (rc = call.sync()))
            return rc;
    }
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_luma_u8(const unsigned char *d_frames, int F, int H, int W, int channels, int order, unsigned char *d_luma,
                          void *stream)
{
    int rc = check_frames(FrameLayout::packed(channels, OFLK_ORDER_RGB), d_frames, F, H, W, d_luma);
    if (rc || (rc = check_order(order))) return rc;
    return luma_launch(d_frames, F, H, W, channels, order, d_luma, (hipStream_t)stream);
}

OFLK_API int oflk_luma_u8_host(const unsigned char *frames, int F, int H, int W, int channels, int order, unsigned char *luma)
{
    int rc = check_frames(FrameLayout::packed(channels, OFLK_ORDER_RGB), frames, F, H, W, luma);
    if (rc || (rc = check_order(order))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    return luma_chunks(call, frames, F, H, W, channels, order, luma);
}

// =============================================================================
// NV12 video: Y[H][W] then UV[H/2][W/2][2] in H W 3 / 2 contiguous bytes -- the fused two-plane warp's launch (oflk_nv12.hpp)
// =============================================================================
namespace {
// the one launch of both planes of F frames on stream s; the arguments are checked
int warp_nv12_launch(bool persp, const unsigned char *d_frames, int F, int H, int W, int siting, const double *d_map,
                     unsigned char *d_out, unsigned char *d_inside, hipStream_t s)
{
    WarpNv12Args a{};
    a.in = d_frames; a.map = d_map; a.out = d_out; a.inside = d_inside;
    a.F = F; a.H = H; a.W = W;
    a.sx = siting == OFLK_SITING_CENTER ? 0.5 : 0.0;
    a.sy = 0.5;
    const unsigned cols = (unsigned)((W + 64 * kWarpPx - 1) / (64 * kWarpPx));
    a.luma_groups = (unsigned)((H + 3) / 4);
    a.chroma_cols = (unsigned)((W / 2 + 64 * kWarpPx - 1) / (64 * kWarpPx));
    const unsigned chroma_blocks = (unsigned)((H / 2 + 3) / 4) * a.chroma_cols;
    // a luma lane's store: a dword of Y and the inside dword; a chroma lane's: one dwordx2.  W % 8 == 0 keeps H W and every
    // frame's and row's offset a multiple of 8
    const bool vec_luma = W % kWarpPx == 0 && aligned(d_out, kWarpPx) && (!d_inside || aligned(d_inside, kWarpPx));
    const int vec = !vec_luma ? 0 : W % (2 * kWarpPx) == 0 && aligned(d_out, 2 * kWarpPx) ? 2 : 1;
    const dim3 grid(a.luma_groups + (chroma_blocks + cols - 1) / cols, cols, (unsigned)std::min(F, 65535));
    with_bool(persp, [&](auto PERSP) {
        with_int<0, 1, 2>(vec, [&](auto VEC) {
            hipLaunchKernelGGL((k_warp_nv12<decltype(PERSP)::value, decltype(VEC)::value>), grid, dim3(256), 0, s, a);
        });
    });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}
}  // namespace

OFLK_API size_t oflk_nv12_frame_bytes(int H, int W)
{
    if (H < 4 || W < 4 || H % 2 || W % 2 || (size_t)H * (size_t)W >= ((size_t)1 << 30) || H >= kMaxDim || W >= kMaxDim) return 0;
    return (size_t)H * (size_t)W / 2 * 3;
}

// =============================================================================
// frames of any layout: the one path of the warps and the sequence stabilisers
// =============================================================================
namespace {
// the one launch of the warp of F frames of layout L on stream s: the single point that picks among the three launchers.  The
// arguments are checked.  persp: d_map is [F][9]
int warp_launch(const FrameLayout &L, bool persp, const void *d_frames, int F, int H, int W, const double *d_map, void *d_out,
                unsigned char *d_inside, hipStream_t s)
{
    const unsigned char *in = static_cast<const unsigned char *>(d_frames);
    unsigned char *out = static_cast<unsigned char *>(d_out);
    switch (L.kind) {
    case FrameKind::Planar: {
        int rc = OFLK_OK;
        with_pix(L.pix_bytes == 1, [&](auto PIX) {
            using P = typename decltype(PIX)::type;
            rc = warp_planar_launch<P>(persp, (const P *)d_frames, F, H, W, d_map, (P *)d_out, d_inside, s);
        });
        return rc;
    }
    case FrameKind::Packed: return warp_packed_launch(persp, in, F, H, W, L.channels, d_map, out, d_inside, s);
    case FrameKind::Nv12: return warp_nv12_launch(persp, in, F, H, W, L.siting, d_map, out, d_inside, s);
    }
    return OFLK_OK;
}

// F host frames under the device maps d_map [F][6] (persp: [F][9]), in chunks of frames through one pair of device buffers: a
// chunk goes up, is warped and comes down.  Frames are independent, so the result does not depend on the cut.
int warp_chunks(HostCall &call, const FrameLayout &L, bool persp, const void *frames, int F, int H, int W, const double *d_map,
                void *out, unsigned char *inside)
{
    const int C = sparse_chunk_pairs(F, H, W);
    const size_t fb = L.frame_bytes(H, W), ib = L.inside_bytes(H, W);
    const unsigned char *src = static_cast<const unsigned char *>(frames);
    unsigned char *dst = static_cast<unsigned char *>(out), *d_in = nullptr, *d_out = nullptr, *d_inside = nullptr;
    int rc;
    if ((rc = call.alloc(&d_in, (size_t)C * fb)) || (rc = call.alloc(&d_out, (size_t)C * fb)) ||
        (rc = call.alloc(&d_inside, (size_t)C * ib, inside != nullptr)))
        return rc;
    for (int f0 = 0; f0 < F; f0 += C) {
        const int n = std::min(C, F - f0);
        const size_t o = (size_t)f0 * fb, len = (size_t)n * fb;
        if ((rc = call.to_device(d_in, src + o, len)) ||
            (rc = warp_launch(L, persp, d_in, n, H, W, d_map + (persp ? 9 : 6) * (size_t)f0, d_out, d_inside, nullptr)) ||
            (rc = call.to_host(dst + o, d_out, len)) ||
            (inside && (rc = call.to_host(inside + (size_t)f0 * ib, d_inside, (size_t)n * ib))) || (rc = call.sync()))
            return rc;
    }
    return OFLK_OK;
}

int warp_host(const FrameLayout &L, bool persp, const void *frames, int F, int H, int W, const double *map, void *out,
              unsigned char *inside)
{
    int rc = check_frames(L, frames, F, H, W, out, !map);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    double *d_map = nullptr;
    if ((rc = call.upload(&d_map, map, (persp ? 9 : 6) * (size_t)F))) return rc;
    return warp_chunks(call, L, persp, frames, F, H, W, d_map, out, inside);
}

int warp_device(const FrameLayout &L, bool persp, const void *d_frames, int F, int H, int W, const double *d_map, void *d_out,
                unsigned char *d_inside, void *stream)
{
    if (int rc = check_frames(L, d_frames, F, H, W, d_out, !d_map)) return rc;
    if (!aligned(d_map, 8)) return fail(OFLK_ERR_INVALID, "d_map must be 8-byte aligned");
    if (L.kind == FrameKind::Planar && L.pix_bytes == 4 && (!aligned(d_frames, 4) || !aligned(d_out, 4)))
        return fail(OFLK_ERR_INVALID, "float32 frames must be 4-byte aligned");
    return warp_launch(L, persp, d_frames, F, H, W, d_map, d_out, d_inside, (hipStream_t)stream);
}

// The sequence stabiliser of every layout.  Pass 1 is the grey call's, on the frames themselves (planar) or on a host array
// of luma of this call's own, one byte a pixel: the packed frames' luma comes down in a chunked pass ahead of pass 1 (a
// third or a quarter of the caller's frames), the NV12 frames' Y planes are gathered with no device work (two thirds).
// Pass 2 warps the caller's frames in their own layout.
int stabilize_sequence(const FrameLayout &L, const void *frames, int T, int H, int W, const KltConfig &klt, const FitConfig &fit,
                       const TrajWindow &window, void *out, float *correction, float *model_out, int *counts_out,
                       unsigned char *held)
{
    int rc = check_layout(L, H, W);
    if (rc) return rc;
    if (T < 2) return fail(OFLK_ERR_INVALID, "a sequence needs T >= 2 frames (got %d)", T);
    if ((rc = check_frames(L, frames, T, H, W, out)) || (rc = check_stabilize_config(H, W, klt, fit, window))) return rc;
    const unsigned char *bytes = static_cast<const unsigned char *>(frames);
    const size_t plane = (size_t)H * W;
    std::vector<unsigned char> luma;
    switch (L.kind) {
    case FrameKind::Planar: break;
    case FrameKind::Packed: {
        try {
            luma.resize((size_t)T * plane);
        } catch (const std::exception &) {
            return fail(OFLK_ERR_NOMEM, "no host memory for the luma of %d frames of %d x %d", T, W, H);
        }
        HostCall call;
        if ((rc = call.begin()) || (rc = luma_chunks(call, bytes, T, H, W, L.channels, L.order, luma.data()))) return rc;
        break;
    }
    case FrameKind::Nv12:
        try {
            luma.resize((size_t)T * plane);
        } catch (const std::exception &) {
            return fail(OFLK_ERR_NOMEM, "no host memory for the Y planes of %d frames of %d x %d", T, W, H);
        }
        for (int t = 0; t < T; t++) std::memcpy(luma.data() + (size_t)t * plane, bytes + (size_t)t * L.frame_bytes(H, W), plane);
        break;
    }
    const bool planar = L.kind == FrameKind::Planar;
    HostCall call;
    double *d_map = nullptr;
    if ((rc = stabilize_maps(call, planar ? frames : luma.data(), planar ? L.pix_bytes == 1 : true, T, H, W, klt, fit, window,
                             correction, model_out, counts_out, held, &d_map)))
        return rc;
    return warp_chunks(call, L, false, frames, T, H, W, d_map, out, nullptr);
}
}  // namespace

// ---- the twelve warps: affine and perspective, device and host, of the four layouts ----
OFLK_API int oflk_warp_affine(const void *d_frames, int u8, int F, int H, int W, const double *d_map, void *d_out,
                              unsigned char *d_inside, void *stream)
{
    return warp_device(FrameLayout::planar(u8 != 0), false, d_frames, F, H, W, d_map, d_out, d_inside, stream);
}

OFLK_API int oflk_warp_perspective(const void *d_frames, int u8, int F, int H, int W, const double *d_map, void *d_out,
                                   unsigned char *d_inside, void *stream)
{
    return warp_device(FrameLayout::planar(u8 != 0), true, d_frames, F, H, W, d_map, d_out, d_inside, stream);
}

OFLK_API int oflk_warp_affine_host(const float *frames, int F, int H, int W, const double *map, float *out, unsigned char *inside)
{
    return warp_host(FrameLayout::planar(false), false, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_affine_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, unsigned char *out,
                                      unsigned char *inside)
{
    return warp_host(FrameLayout::planar(true), false, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_perspective_host(const float *frames, int F, int H, int W, const double *map, float *out, unsigned char *inside)
{
    return warp_host(FrameLayout::planar(false), true, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_perspective_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, unsigned char *out,
                                           unsigned char *inside)
{
    return warp_host(FrameLayout::planar(true), true, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_affine_packed(const unsigned char *d_frames, int F, int H, int W, int channels, const double *d_map,
                                     unsigned char *d_out, unsigned char *d_inside, void *stream)
{
    return warp_device(FrameLayout::packed(channels, OFLK_ORDER_RGB), false, d_frames, F, H, W, d_map, d_out, d_inside, stream);
}

OFLK_API int oflk_warp_perspective_packed(const unsigned char *d_frames, int F, int H, int W, int channels, const double *d_map,
                                          unsigned char *d_out, unsigned char *d_inside, void *stream)
{
    return warp_device(FrameLayout::packed(channels, OFLK_ORDER_RGB), true, d_frames, F, H, W, d_map, d_out, d_inside, stream);
}

OFLK_API int oflk_warp_affine_packed_host(const unsigned char *frames, int F, int H, int W, int channels, const double *map,
                                          unsigned char *out, unsigned char *inside)
{
    return warp_host(FrameLayout::packed(channels, OFLK_ORDER_RGB), false, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_perspective_packed_host(const unsigned char *frames, int F, int H, int W, int channels, const double *map,
                                               unsigned char *out, unsigned char *inside)
{
    return warp_host(FrameLayout::packed(channels, OFLK_ORDER_RGB), true, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_affine_nv12(const unsigned char *d_frames, int F, int H, int W, int siting, const double *d_map,
                                   unsigned char *d_out, unsigned char *d_inside, void *stream)
{
    return warp_device(FrameLayout::nv12(siting), false, d_frames, F, H, W, d_map, d_out, d_inside, stream);
}

OFLK_API int oflk_warp_perspective_nv12(const unsigned char *d_frames, int F, int H, int W, int siting, const double *d_map,
                                        unsigned char *d_out, unsigned char *d_inside, void *stream)
{
    return warp_device(FrameLayout::nv12(siting), true, d_frames, F, H, W, d_map, d_out, d_inside, stream);
}

OFLK_API int oflk_warp_affine_nv12_host(const unsigned char *frames, int F, int H, int W, int siting, const double *map,
                                        unsigned char *out, unsigned char *inside)
{
    return warp_host(FrameLayout::nv12(siting), false, frames, F, H, W, map, out, inside);
}

OFLK_API int oflk_warp_perspective_nv12_host(const unsigned char *frames, int F, int H, int W, int siting, const double *map,
                                             unsigned char *out, unsigned char *inside)
{
    return warp_host(FrameLayout::nv12(siting), true, frames, F, H, W, map, out, inside);
}

// ---- the four sequence stabilisers ----
OFLK_API int oflk_stabilize_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                                     float beta, float max_residual, float quality_level, float min_distance, int max_corners,
                                     int detect_every, int model, int hypotheses, float threshold, unsigned seed,
                                     const double *weights, int radius, float *out, float *correction, float *model_out,
                                     int *counts_out, unsigned char *held)
{
    return stabilize_sequence(FrameLayout::planar(false), frames, T, H, W,
                              {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                              {model, hypotheses, threshold, seed}, {weights, radius}, out, correction, model_out, counts_out, held);
}

OFLK_API int oflk_stabilize_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                        float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                        int max_corners, int detect_every, int model, int hypotheses, float threshold,
                                        unsigned seed, const double *weights, int radius, unsigned char *out, float *correction,
                                        float *model_out, int *counts_out, unsigned char *held)
{
    return stabilize_sequence(FrameLayout::planar(true), frames, T, H, W,
                              {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                              {model, hypotheses, threshold, seed}, {weights, radius}, out, correction, model_out, counts_out, held);
}

OFLK_API int oflk_stabilize_sequence_packed(const unsigned char *frames, int T, int H, int W, int channels, int order, int levels,
                                            int window_size, int iters, float alpha, float beta, float max_residual,
                                            float quality_level, float min_distance, int max_corners, int detect_every, int model,
                                            int hypotheses, float threshold, unsigned seed, const double *weights, int radius,
                                            unsigned char *out, float *correction, float *model_out, int *counts_out,
                                            unsigned char *held)
{
    return stabilize_sequence(FrameLayout::packed(channels, order), frames, T, H, W,
                              {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                              {model, hypotheses, threshold, seed}, {weights, radius}, out, correction, model_out, counts_out, held);
}

OFLK_API int oflk_stabilize_sequence_nv12(const unsigned char *frames, int T, int H, int W, int siting, int levels, int window_size,
                                          int iters, float alpha, float beta, float max_residual, float quality_level,
                                          float min_distance, int max_corners, int detect_every, int model, int hypotheses,
                                          float threshold, unsigned seed, const double *weights, int radius, unsigned char *out,
                                          float *correction, float *model_out, int *counts_out, unsigned char *held)
{
    return stabilize_sequence(FrameLayout::nv12(siting), frames, T, H, W,
                              {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                              {model, hypotheses, threshold, seed}, {weights, radius}, out, correction, model_out, counts_out, held);
}

// =============================================================================
// motion-compensated frame interpolation of every layout (oflk_interp.hpp)
// =============================================================================
namespace {
// the times, the refinement count and the test's parameters of an interpolation call
struct InterpConfig { float alpha, beta; int refine; const double *taus; int n; };
// the four flows of the pairs of an interpolation call, [B][H][W] each
struct InterpFlows {
    const float *uf, *vf, *ub, *vb;
    bool any_null() const { return !uf || !vf || !ub || !vb; }
};

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

// what every form refuses of its settings and of its output (every value OFLK_ERR_INVALID); F frames of frame_bytes each
int check_interp(const InterpConfig &cfg, const void *frames, int F, size_t frame_bytes, const void *out)
{
    if (cfg.n < 1 || cfg.n > OFLK_INTERP_MAX_TAUS)
        return fail(OFLK_ERR_INVALID, "n must be in [1, %d] (got %d)", OFLK_INTERP_MAX_TAUS, cfg.n);
    if (!cfg.taus) return fail(OFLK_ERR_INVALID, "NULL taus");
    for (int j = 0; j < cfg.n; j++)
        if (!(std::isfinite(cfg.taus[j]) && cfg.taus[j] > 0.0 && cfg.taus[j] < 1.0))
            return fail(OFLK_ERR_INVALID, "taus[%d] must be finite and strictly between 0 and 1 (got %g)", j, cfg.taus[j]);
    if (cfg.refine < 1 || cfg.refine > 8) return fail(OFLK_ERR_INVALID, "refine must be in [1, 8] (got %d)", cfg.refine);
    if (int rc = check_alpha_beta(cfg.alpha, cfg.beta)) return rc;
    if (!out) return fail(OFLK_ERR_INVALID, "NULL output");
    if (ranges_overlap(out, (size_t)(F - 1) * cfg.n * frame_bytes, frames, (size_t)F * frame_bytes))
        return fail(OFLK_ERR_INVALID, "the output overlaps the frames");
    return OFLK_OK;
}

// The checks of the forms that take flows: B pairs of frames [B+1] of layout L.  A packed or NV12 call refuses its layout
// first and its frames as every call of that layout does (check_frames), then what the grey forms refuse.
int check_interp_flows(const FrameLayout &L, const void *frames, int B, int H, int W, const InterpFlows &fl, const InterpConfig &cfg,
                       const void *out)
{
    if (L.kind == FrameKind::Planar) {
        if (fl.any_null()) return fail(OFLK_ERR_INVALID, "NULL flow argument");
        if (int rc = check_hw(frames, frames, H, W)) return rc;
        if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1 (got %d)", B);
    } else {
        if (int rc = check_layout(L, H, W)) return rc;
        if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1 (got %d)", B);
        if (int rc = check_frames(L, frames, B + 1, H, W, out)) return rc;
        if (fl.any_null()) return fail(OFLK_ERR_INVALID, "NULL flow argument");
    }
    return check_interp(cfg, frames, B + 1, L.frame_bytes(H, W), out);
}

// B * n slices of the layout's kernel, cut at the grid's z limit; the arguments are checked
int interp_launch(const FrameLayout &L, const void *frames, int B, int H, int W, const InterpFlows &fl, const InterpConfig &cfg,
                  void *out, unsigned char *status, hipStream_t s)
{
    constexpr unsigned kMaxZ = 65535;
    InterpNv12Args nv{};
    InterpArgs &a = nv.g;
    a.H = H; a.W = W; a.n = cfg.n;
    a.refine = cfg.refine;
    a.alpha = cfg.alpha; a.beta = cfg.beta;
    for (int j = 0; j < cfg.n; j++) a.tau[j] = cfg.taus[j];
    nv.sx = L.siting == OFLK_SITING_CENTER ? 0.5 : 0.0;
    nv.sy = 0.5;
    const unsigned cols = (unsigned)((W + 63) / 64);
    nv.luma_groups = (unsigned)((H + 3) / 4);
    nv.chroma_cols = (unsigned)((W / 2 + 63) / 64);
    const unsigned chroma_blocks = (unsigned)((H / 2 + 3) / 4) * nv.chroma_cols;
    const size_t plane = (size_t)H * W, fb = L.frame_bytes(H, W), slices = (size_t)B * cfg.n;
    for (size_t z0 = 0; z0 < slices; z0 += kMaxZ) {
        // a launch starts at its first pair: the arrays move there, and the kernel counts slices from that pair's time z0 % n
        const size_t b0 = z0 / cfg.n;
        a.z0 = (unsigned)(z0 % cfg.n);
        a.frames = static_cast<const char *>(frames) + b0 * fb;
        a.uf = fl.uf + b0 * plane; a.vf = fl.vf + b0 * plane; a.ub = fl.ub + b0 * plane; a.vb = fl.vb + b0 * plane;
        a.out = static_cast<char *>(out) + b0 * cfg.n * fb;
        a.status = status ? status + b0 * cfg.n * plane : nullptr;
        const int nz = (int)std::min<size_t>(kMaxZ, slices - z0);
        with_bool(status != nullptr, [&](auto STATUS) {
            constexpr bool ST = decltype(STATUS)::value;
            switch (L.kind) {
            case FrameKind::Planar:
                with_pix(L.pix_bytes == 1, [&](auto PIX) {
                    with_bool(W == 1, [&](auto NARROW) {
                        hipLaunchKernelGGL((k_interp<typename decltype(PIX)::type, ST, decltype(NARROW)::value>), grid2d(W, H, nz),
                                           dim3(256), 0, s, a);
                    });
                });
                break;
            case FrameKind::Packed:   // a lane's store: one dword for C = 4 where out is 4-byte aligned, else bytes
                with_int<3, 4>(L.channels, [&](auto C) {
                    with_bool(L.channels == 4 && aligned(a.out, 4), [&](auto VEC) {
                        if constexpr (decltype(C)::value == 4 || !decltype(VEC)::value)
                            hipLaunchKernelGGL((k_interp_packed<decltype(C)::value, ST, decltype(VEC)::value>), grid2d(W, H, nz),
                                               dim3(256), 0, s, a);
                    });
                });
                break;
            case FrameKind::Nv12:   // a chroma lane's store: its pair as 2 bytes at once where out is 2-byte aligned
                with_bool(aligned(a.out, 2), [&](auto VEC) {
                    hipLaunchKernelGGL((k_interp_nv12<ST, decltype(VEC)::value>),
                                       dim3(nv.luma_groups + (chroma_blocks + cols - 1) / cols, cols, (unsigned)nz), dim3(256), 0, s, nv);
                });
                break;
            }
        });
        HIP_TRY(hipGetLastError());
    }
    return OFLK_OK;
}

int interp_device(const FrameLayout &L, const void *d_frames, int B, int H, int W, const InterpFlows &fl, const InterpConfig &cfg,
                  void *d_out, unsigned char *d_status, void *stream)
{
    if (int rc = check_interp_flows(L, d_frames, B, H, W, fl, cfg, d_out)) return rc;
    return interp_launch(L, d_frames, B, H, W, fl, cfg, d_out, d_status, (hipStream_t)stream);
}

int interp_host(const FrameLayout &L, const void *frames, int B, int H, int W, const InterpFlows &fl, const InterpConfig &cfg,
                void *out, unsigned char *status)
{
    int rc = check_interp_flows(L, frames, B, H, W, fl, cfg, out);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t plane = (size_t)H * W, fb = L.frame_bytes(H, W), n_out = (size_t)B * cfg.n;
    const float *in[4] = {fl.uf, fl.vf, fl.ub, fl.vb};
    char *d_frames, *d_out;
    float *d[4];
    unsigned char *d_status;
    if ((rc = call.upload(&d_frames, static_cast<const char *>(frames), (size_t)(B + 1) * fb))) return rc;
    for (int i = 0; i < 4; i++)
        if ((rc = call.upload(&d[i], in[i], (size_t)B * plane))) return rc;
    if ((rc = call.alloc(&d_out, n_out * fb)) || (rc = call.alloc(&d_status, n_out * plane, status)) ||
        (rc = interp_launch(L, d_frames, B, H, W, {d[0], d[1], d[2], d[3]}, cfg, d_out, d_status, nullptr)) ||
        (rc = call.to_host(static_cast<char *>(out), d_out, n_out * fb)) ||
        (status && (rc = call.to_host(status, d_status, n_out * plane))))
        return rc;
    return call.sync();
}

// Frames in, in-between frames out, host pointers: run_sequence_fb's chunk loop with one interpolation launch per chunk in
// the place of the check launch; only out and status come down.  Grey frames are the flow pass's own.  A chunk of packed or
// NV12 frames goes up once into a buffer of the layout; the planes the flows are tracked on are formed from it on the device
// (the luma of packed frames by luma_launch, the Y planes of NV12 frames by one strided copy) and the interpolation reads
// the chunk where it lies.
int run_sequence_interp(const FrameLayout &L, const void *frames, int T, int H, int W, const PyrWindow &pyr, const InterpConfig &cfg,
                        void *out, unsigned char *status, int flow_median = 0)
{
    const bool planar = L.kind == FrameKind::Planar;
    const Seq seq{pyr, frames, L.pix_bytes == 1, T, H, W, flow_median};
    t_resolved = 0;
    int rc = OFLK_OK;
    if (!planar) {
        if ((rc = check_layout(L, H, W))) return rc;
        if (T < 2) return fail(OFLK_ERR_INVALID, "a sequence needs T >= 2 frames (got %d)", T);
        if ((rc = check_frames(L, frames, T, H, W, out))) return rc;
    }
    const size_t plane = (size_t)H * W, fb = L.frame_bytes(H, W);
    if ((rc = BidirChunk::check(seq)) || (rc = check_interp(cfg, frames, T, fb, out))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int B = T - 1, C = chunk_pairs(B, H, W);
    BidirChunk k{};
    char *d_out;
    unsigned char *d_status, *d_video = nullptr;
    if ((rc = k.alloc(call, seq, C)) || (rc = call.alloc(&d_video, (size_t)(C + 1) * fb, !planar)) ||
        (rc = call.alloc(&d_out, (size_t)C * cfg.n * fb)) || (rc = call.alloc(&d_status, (size_t)C * cfg.n * plane, status)))
        return rc;
    const unsigned char *src = static_cast<const unsigned char *>(frames);
    unsigned char *luma = reinterpret_cast<unsigned char *>(k.frames);
    for (int b0 = 0; b0 < B; b0 += C) {
        const int nb = std::min(C, B - b0);
        const size_t o = (size_t)b0 * cfg.n, cnt = (size_t)nb * cfg.n;
        if (planar) {
            rc = k.run(call, seq, b0, nb);
        } else {
            rc = k.compute(call, seq, nb, [&] {
                if (int e = call.to_device(d_video, src + (size_t)b0 * fb, (size_t)(nb + 1) * fb)) return e;
                if (L.kind == FrameKind::Packed) return luma_launch(d_video, nb + 1, H, W, L.channels, L.order, luma, nullptr);
                HIP_TRY(hipMemcpy2DAsync(luma, plane, d_video, fb, plane, (size_t)(nb + 1), hipMemcpyDeviceToDevice, nullptr));
                return (int)OFLK_OK;
            });
        }
        if (rc || (rc = interp_launch(L, planar ? k.frames : reinterpret_cast<char *>(d_video), nb, H, W, {k.d[0], k.d[1], k.d[2], k.d[3]},
                                      cfg, d_out, d_status, nullptr)) ||
            (rc = call.to_host(static_cast<char *>(out) + o * fb, d_out, cnt * fb)) ||
            (status && (rc = call.to_host(status + o * plane, d_status, cnt * plane))) || (rc = call.sync()))
            return rc;
    }
    return OFLK_OK;
}
}  // namespace

// ---- the interpolation calls: device, host and sequence forms of the four layouts ----
OFLK_API int oflk_interpolate_frames(const void *d_frames, int u8, int B, int H, int W, const float *d_uf, const float *d_vf,
                                     const float *d_ub, const float *d_vb, float alpha, float beta, int refine,
                                     const double *taus, int n, void *d_out, unsigned char *d_status, void *stream)
{
    return interp_device(FrameLayout::planar(u8 != 0), d_frames, B, H, W, {d_uf, d_vf, d_ub, d_vb}, {alpha, beta, refine, taus, n},
                         d_out, d_status, stream);
}

OFLK_API int oflk_interpolate_frames_packed(const unsigned char *d_frames, int B, int H, int W, int channels, const float *d_uf,
                                            const float *d_vf, const float *d_ub, const float *d_vb, float alpha, float beta,
                                            int refine, const double *taus, int n, unsigned char *d_out, unsigned char *d_status,
                                            void *stream)
{
    return interp_device(FrameLayout::packed(channels, OFLK_ORDER_RGB), d_frames, B, H, W, {d_uf, d_vf, d_ub, d_vb},
                         {alpha, beta, refine, taus, n}, d_out, d_status, stream);
}

OFLK_API int oflk_interpolate_frames_nv12(const unsigned char *d_frames, int B, int H, int W, int siting, const float *d_uf,
                                          const float *d_vf, const float *d_ub, const float *d_vb, float alpha, float beta,
                                          int refine, const double *taus, int n, unsigned char *d_out, unsigned char *d_status,
                                          void *stream)
{
    return interp_device(FrameLayout::nv12(siting), d_frames, B, H, W, {d_uf, d_vf, d_ub, d_vb}, {alpha, beta, refine, taus, n}, d_out,
                         d_status, stream);
}

OFLK_API int oflk_interpolate_frames_host(const float *frames, int B, int H, int W, const float *uf, const float *vf,
                                          const float *ub, const float *vb, float alpha, float beta, int refine,
                                          const double *taus, int n, float *out, unsigned char *status)
{
    return interp_host(FrameLayout::planar(false), frames, B, H, W, {uf, vf, ub, vb}, {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_frames_host_u8(const unsigned char *frames, int B, int H, int W, const float *uf, const float *vf,
                                             const float *ub, const float *vb, float alpha, float beta, int refine,
                                             const double *taus, int n, unsigned char *out, unsigned char *status)
{
    return interp_host(FrameLayout::planar(true), frames, B, H, W, {uf, vf, ub, vb}, {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_frames_packed_host(const unsigned char *frames, int B, int H, int W, int channels, const float *uf,
                                                 const float *vf, const float *ub, const float *vb, float alpha, float beta,
                                                 int refine, const double *taus, int n, unsigned char *out, unsigned char *status)
{
    return interp_host(FrameLayout::packed(channels, OFLK_ORDER_RGB), frames, B, H, W, {uf, vf, ub, vb},
                       {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_frames_nv12_host(const unsigned char *frames, int B, int H, int W, int siting, const float *uf,
                                               const float *vf, const float *ub, const float *vb, float alpha, float beta,
                                               int refine, const double *taus, int n, unsigned char *out, unsigned char *status)
{
    return interp_host(FrameLayout::nv12(siting), frames, B, H, W, {uf, vf, ub, vb}, {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                       float alpha, float beta, int refine, const double *taus, int n, float *out,
                                       unsigned char *status)
{
    return run_sequence_interp(FrameLayout::planar(false), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                          int iters, float alpha, float beta, int refine, const double *taus, int n,
                                          unsigned char *out, unsigned char *status)
{
    return run_sequence_interp(FrameLayout::planar(true), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_sequence_packed(const unsigned char *frames, int T, int H, int W, int channels, int order,
                                              int levels, int window_size, int iters, float alpha, float beta, int refine,
                                              const double *taus, int n, unsigned char *out, unsigned char *status)
{
    return run_sequence_interp(FrameLayout::packed(channels, order), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status);
}

OFLK_API int oflk_interpolate_sequence_nv12(const unsigned char *frames, int T, int H, int W, int siting, int levels,
                                            int window_size, int iters, float alpha, float beta, int refine, const double *taus,
                                            int n, unsigned char *out, unsigned char *status)
{
    return run_sequence_interp(FrameLayout::nv12(siting), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status);
}

// the same four with the flows of every chunk median filtered before they are used (flow_median: 0, 3, 5, 7 or 9)
OFLK_API int oflk_interpolate_sequence_median(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                              float alpha, float beta, int refine, const double *taus, int n, int flow_median,
                                              float *out, unsigned char *status)
{
    return run_sequence_interp(FrameLayout::planar(false), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status, flow_median);
}

OFLK_API int oflk_interpolate_sequence_median_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                                 int iters, float alpha, float beta, int refine, const double *taus, int n,
                                                 int flow_median, unsigned char *out, unsigned char *status)
{
    return run_sequence_interp(FrameLayout::planar(true), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status, flow_median);
}

OFLK_API int oflk_interpolate_sequence_packed_median(const unsigned char *frames, int T, int H, int W, int channels, int order,
                                                     int levels, int window_size, int iters, float alpha, float beta, int refine,
                                                     const double *taus, int n, int flow_median, unsigned char *out,
                                                     unsigned char *status)
{
    return run_sequence_interp(FrameLayout::packed(channels, order), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status, flow_median);
}

OFLK_API int oflk_interpolate_sequence_nv12_median(const unsigned char *frames, int T, int H, int W, int siting, int levels,
                                                   int window_size, int iters, float alpha, float beta, int refine,
                                                   const double *taus, int n, int flow_median, unsigned char *out,
                                                   unsigned char *status)
{
    return run_sequence_interp(FrameLayout::nv12(siting), frames, T, H, W, {levels, window_size, iters},
                               {alpha, beta, refine, taus, n}, out, status, flow_median);
}

// =============================================================================
// motion-compensated temporal denoising on the dense flows (oflk_denoise.hpp): the host and the sequence forms
// =============================================================================
namespace {
// the test's parameters, the reach in frames and the weight's cutoff of a denoising call
struct DenoiseConfig { float alpha, beta; int radius; float strength; };

// what every form refuses of its settings and of its output (every value OFLK_ERR_INVALID); F frames of frame_bytes each
int check_denoise(const DenoiseConfig &cfg, const void *frames, int F, size_t frame_bytes, const void *out)
{
    if (cfg.radius < 1 || cfg.radius > OFLK_DENOISE_MAX_RADIUS)
        return fail(OFLK_ERR_INVALID, "radius must be in [1, %d] (got %d)", OFLK_DENOISE_MAX_RADIUS, cfg.radius);
    if (!(std::isfinite(cfg.strength) && cfg.strength > 0.0f))
        return fail(OFLK_ERR_INVALID, "strength must be finite and > 0 (got %g)", (double)cfg.strength);
    if (int rc = check_alpha_beta(cfg.alpha, cfg.beta)) return rc;
    if (!out) return fail(OFLK_ERR_INVALID, "NULL output");
    if (ranges_overlap(out, (size_t)F * frame_bytes, frames, (size_t)F * frame_bytes))
        return fail(OFLK_ERR_INVALID, "the output overlaps the frames");
    return OFLK_OK;
}

// The device arrays a launch reads: rings of fcap frames and of pcap pairs' flows (oflk_denoise.hpp: frame s in slot
// s % fcap, pair s in slot s % pcap)
struct DenoiseRings {
    const void *frames;
    InterpFlows fl;
    int fcap, pcap;
};

// Output frames t0 .. t0+n-1 of a sequence of T frames into out [n][H][W] (and count), cut at the grid's z limit; the
// rings hold every frame and pair within cfg.radius of those frames.  The arguments are checked.
int denoise_launch(bool u8, const DenoiseRings &r, int T, int t0, int n, int H, int W, const DenoiseConfig &cfg, void *out,
                   unsigned char *count, hipStream_t s)
{
    constexpr int kMaxZ = 65535;
    DenoiseArgs a{};
    a.frames = r.frames;
    a.uf = r.fl.uf; a.vf = r.fl.vf; a.ub = r.fl.ub; a.vb = r.fl.vb;
    a.H = H; a.W = W; a.T = T;
    a.fcap = r.fcap; a.pcap = r.pcap;
    a.radius = cfg.radius;
    a.alpha = cfg.alpha; a.beta = cfg.beta;
    a.h2 = cfg.strength * cfg.strength;
    const size_t plane = (size_t)H * W, fb = plane * (u8 ? 1 : sizeof(float));
    for (int z0 = 0; z0 < n; z0 += kMaxZ) {
        a.t0 = t0 + z0;
        a.out = static_cast<char *>(out) + (size_t)z0 * fb;
        a.count = count ? count + (size_t)z0 * plane : nullptr;
        const int nz = std::min(kMaxZ, n - z0);
        with_pix(u8, [&](auto PIX) {
            with_bool(count != nullptr, [&](auto COUNT) {
                with_bool(W == 1, [&](auto NARROW) {
                    hipLaunchKernelGGL((k_denoise<typename decltype(PIX)::type, decltype(COUNT)::value, decltype(NARROW)::value>),
                                       grid2d(W, H, nz), dim3(256), 0, s, a);
                });
            });
        });
        HIP_TRY(hipGetLastError());
    }
    return OFLK_OK;
}

int denoise_host(bool u8, const void *frames, int B, int H, int W, const InterpFlows &fl, const DenoiseConfig &cfg, void *out,
                 unsigned char *count)
{
    if (fl.any_null()) return fail(OFLK_ERR_INVALID, "NULL flow argument");
    int rc = check_hw(frames, frames, H, W);
    if (rc) return rc;
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1 (got %d)", B);
    const size_t plane = (size_t)H * W, fb = plane * (u8 ? 1 : sizeof(float)), F = (size_t)B + 1;
    if ((rc = check_denoise(cfg, frames, B + 1, fb, out))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const float *in[4] = {fl.uf, fl.vf, fl.ub, fl.vb};
    char *d_frames, *d_out;
    float *d[4];
    unsigned char *d_count;
    if ((rc = call.upload(&d_frames, static_cast<const char *>(frames), F * fb))) return rc;
    for (int i = 0; i < 4; i++)
        if ((rc = call.upload(&d[i], in[i], (size_t)B * plane))) return rc;
    if ((rc = call.alloc(&d_out, F * fb)) || (rc = call.alloc(&d_count, F * plane, count)) ||
        (rc = denoise_launch(u8, {d_frames, {d[0], d[1], d[2], d[3]}, B + 1, B}, B + 1, 0, B + 1, H, W, cfg, d_out, d_count, nullptr)) ||
        (rc = call.to_host(static_cast<char *>(out), d_out, F * fb)) || (count && (rc = call.to_host(count, d_count, F * plane))))
        return rc;
    return call.sync();
}

// Frames in, denoised frames out, host pointers: run_sequence_fb's chunk loop on its chunks, so that every pair's flows are
// computed exactly once and are that call's.  A frame needs the flows of R = radius pairs on either side, more than a chunk
// may hold, so the flows and frames a later frame still needs stay on the device in rings: after the chunk that ends with
// frame `top`, frames next .. top - R have all their pairs and are emitted (next .. T - 1 after the last chunk).  The oldest
// frame and pair they read is next - R, and next is the chunk before's top - R + 1: with this chunk's C pairs the rings span
// C + 2 R pairs and C + 2 R + 1 frames at most, which is their size, and a chunk's slots replace only what no frame still to
// be emitted reads.  What a frame reads does not depend on the cut.  Only out and count come down.
int run_sequence_denoise(bool u8, const void *frames, int T, int H, int W, const PyrWindow &pyr, const DenoiseConfig &cfg,
                         int flow_median, void *out, unsigned char *count)
{
    const Seq seq{pyr, frames, u8, T, H, W, flow_median};
    const size_t plane = (size_t)H * W, fb = seq.frame_bytes();
    int rc = BidirChunk::check(seq);
    if (rc || (rc = check_denoise(cfg, frames, T, fb, out))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int B = T - 1, C = chunk_pairs(B, H, W), R = cfg.radius;
    const int pcap = C + 2 * R, fcap = pcap + 1, ocap = std::min(T, C + R + 1);   // a step emits C + R + 1 frames at most
    BidirChunk k{};
    char *ring_frames, *d_out;
    float *ring[4];
    unsigned char *d_count;
    if ((rc = k.alloc(call, seq, C)) || (rc = call.alloc(&ring_frames, (size_t)fcap * fb))) return rc;
    for (auto &q : ring)
        if ((rc = call.alloc(&q, (size_t)pcap * plane))) return rc;
    if ((rc = call.alloc(&d_out, (size_t)ocap * fb)) || (rc = call.alloc(&d_count, (size_t)ocap * plane, count))) return rc;
    // planes s0 .. s0+n-1 of a chunk's buffer into their slots of a ring of cap planes
    auto to_ring = [&](char *dst, int cap, const char *src, int s0, int n, size_t bytes) {
        for (int i = 0; i < n; i++)
            HIP_TRY(hipMemcpyAsync(dst + (size_t)((s0 + i) % cap) * bytes, src + (size_t)i * bytes, bytes, hipMemcpyDeviceToDevice, nullptr));
        return (int)OFLK_OK;
    };
    int next = 0;
    for (int b0 = 0; b0 < B; b0 += C) {
        const int nb = std::min(C, B - b0), top = b0 + nb;
        if ((rc = k.run(call, seq, b0, nb)) || (rc = to_ring(ring_frames, fcap, k.frames, b0, nb + 1, fb))) return rc;
        for (int i = 0; i < 4; i++)
            if ((rc = to_ring(reinterpret_cast<char *>(ring[i]), pcap, reinterpret_cast<const char *>(k.d[i]), b0, nb, plane * sizeof(float))))
                return rc;
        const int end = top == B ? T : top - R + 1;   // one past the last frame whose R pairs ahead exist
        if (end > next) {
            const int n = end - next;
            if ((rc = denoise_launch(u8, {ring_frames, {ring[0], ring[1], ring[2], ring[3]}, fcap, pcap}, T, next, n, H, W, cfg, d_out,
                                     d_count, nullptr)) ||
                (rc = call.to_host(static_cast<char *>(out) + (size_t)next * fb, d_out, (size_t)n * fb)) ||
                (count && (rc = call.to_host(count + (size_t)next * plane, d_count, (size_t)n * plane))))
                return rc;
            next = end;
        }
        if ((rc = call.sync())) return rc;
    }
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_denoise_frames_host(const float *frames, int B, int H, int W, const float *uf, const float *vf, const float *ub,
                                      const float *vb, float alpha, float beta, int radius, float strength, float *out,
                                      unsigned char *count)
{
    return denoise_host(false, frames, B, H, W, {uf, vf, ub, vb}, {alpha, beta, radius, strength}, out, count);
}

OFLK_API int oflk_denoise_frames_host_u8(const unsigned char *frames, int B, int H, int W, const float *uf, const float *vf,
                                         const float *ub, const float *vb, float alpha, float beta, int radius, float strength,
                                         unsigned char *out, unsigned char *count)
{
    return denoise_host(true, frames, B, H, W, {uf, vf, ub, vb}, {alpha, beta, radius, strength}, out, count);
}

OFLK_API int oflk_denoise_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                                   float beta, int flow_median, int radius, float strength, float *out, unsigned char *count)
{
    return run_sequence_denoise(false, frames, T, H, W, {levels, window_size, iters}, {alpha, beta, radius, strength}, flow_median,
                                out, count);
}

OFLK_API int oflk_denoise_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                      float alpha, float beta, int flow_median, int radius, float strength, unsigned char *out,
                                      unsigned char *count)
{
    return run_sequence_denoise(true, frames, T, H, W, {levels, window_size, iters}, {alpha, beta, radius, strength}, flow_median,
                                out, count);
}

// =============================================================================
// median filtering of flow planes (oflk_flowmedian.hpp): the device and the host form
// =============================================================================
namespace {
// what both forms refuse before any device call (every value OFLK_ERR_INVALID, then check_hw's with its codes)
int check_flow_median(const float *in, const float *out, int P, int H, int W, int size)
{
    if (!in || !out) return fail(OFLK_ERR_INVALID, "NULL array argument");
    if (P < 1) return fail(OFLK_ERR_INVALID, "P must be >= 1 (got %d)", P);
    if (int rc = check_flow_median_size(size)) return rc;
    if (int rc = check_hw(in, out, H, W)) return rc;
    const size_t bytes = (size_t)P * H * W * sizeof(float);
    if (ranges_overlap(out, bytes, in, bytes)) return fail(OFLK_ERR_INVALID, "the output overlaps the input: the filter is not in place");
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_flow_median_tile(int *tile_h, int *tile_w)
{
    if (!tile_h || !tile_w) return fail(OFLK_ERR_INVALID, "NULL output");
    *tile_h = kFlowMedianTileH;
    *tile_w = kFlowMedianTileW;
    return OFLK_OK;
}

OFLK_API int oflk_flow_median(const float *d_in, float *d_out, int P, int H, int W, int size, void *stream)
{
    if (int rc = check_flow_median(d_in, d_out, P, H, W, size)) return rc;
    return flow_median_launch(d_in, d_out, (size_t)P, H, W, size, (hipStream_t)stream);
}

// Host planes in chunks of sparse_chunk_pairs planes (~128 MB of float32, 64 planes at most) through one pair of device
// buffers, as the warps' frames go (warp_chunks).  Planes are independent, so the result does not depend on the cut.
OFLK_API int oflk_flow_median_host(const float *in, float *out, int P, int H, int W, int size)
{
    int rc = check_flow_median(in, out, P, H, W, size);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int C = sparse_chunk_pairs(P, H, W);
    const size_t plane = (size_t)H * W;
    float *d_in = nullptr, *d_out = nullptr;
    if ((rc = call.alloc(&d_in, (size_t)C * plane)) || (rc = call.alloc(&d_out, (size_t)C * plane))) return rc;
    for (int p0 = 0; p0 < P; p0 += C) {
        const size_t o = (size_t)p0 * plane, len = (size_t)std::min(C, P - p0) * plane;
        if ((rc = call.to_device(d_in, in + o, len)) ||
            (rc = flow_median_launch(d_in, d_out, (size_t)std::min(C, P - p0), H, W, size, nullptr)) ||
            (rc = call.to_host(out + o, d_out, len)) || (rc = call.sync()))
            return rc;
    }
    return OFLK_OK;
}

// =============================================================================
// video mosaics: the chain of step homographies, the canvas, accumulate and resolve (oflk_mosaic.hpp)
// =============================================================================
namespace {
size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

// the three planes of a canvas state in a buffer at `base` (NULL: only the size is wanted)
struct MosaicLayout {
    MosaicState st;
    size_t bytes;
};

MosaicLayout mosaic_state(void *base, int Hc, int Wc)
{
    const size_t Wp = ((size_t)Wc + kMosaicPx - 1) / kMosaicPx * kMosaicPx, n = (size_t)Hc * Wp;
    const size_t plane64 = round256(n * sizeof(double)), plane32 = round256(n * sizeof(int));
    char *b = static_cast<char *>(base);
    MosaicLayout l{};
    l.st.sum = reinterpret_cast<double *>(b);
    l.st.wsum = reinterpret_cast<double *>(b + plane64);
    l.st.count = reinterpret_cast<int *>(b + 2 * plane64);
    l.st.Wp = (int)Wp;
    l.bytes = 2 * plane64 + plane32;
    return l;
}

int check_mosaic_canvas(int Hc, int Wc)
{
    if (Hc < 1 || Wc < 1) return fail(OFLK_ERR_INVALID, "Hc and Wc must be >= 1 (got %d x %d)", Hc, Wc);
    if ((size_t)Hc * (size_t)Wc >= ((size_t)1 << 30)) return fail(OFLK_ERR_UNSUPPORTED, "a canvas of 2^30 pixels or more is not supported");
    return OFLK_OK;
}

int check_mosaic_blend(int blend)
{
    if (blend < OFLK_MOSAIC_MEAN || blend > OFLK_MOSAIC_LAST) return fail(OFLK_ERR_INVALID, "unknown blend %d", blend);
    return OFLK_OK;
}

int check_mosaic_frames(const void *frames, int F, int H, int W, const void *map, int Hc, int Wc, int blend)
{
    if (F < 1) return fail(OFLK_ERR_INVALID, "F must be >= 1 (got %d)", F);
    if (H < 2 || W < 2) return fail(OFLK_ERR_INVALID, "H and W must be >= 2 (got %d x %d)", H, W);
    int rc = check_mosaic_canvas(Hc, Wc);
    if (rc || (rc = check_mosaic_blend(blend))) return rc;
    if (!frames || !map) return fail(OFLK_ERR_INVALID, "NULL input argument");
    return check_hw(frames, frames, H, W);
}

int check_mosaic_chain(const void *model, int T, int anchor, int H, int W, double extent, const void *from_anchor, const void *to_anchor,
                       const void *box, const void *dropped)
{
    if (T < 1) return fail(OFLK_ERR_INVALID, "T must be >= 1 (got %d)", T);
    if (anchor < 0 || anchor >= T) return fail(OFLK_ERR_INVALID, "anchor must be in [0, %d] (got %d)", T - 1, anchor);
    if (H < 2 || W < 2) return fail(OFLK_ERR_INVALID, "H and W must be >= 2 (got %d x %d)", H, W);
    if (!(std::isfinite(extent) && extent > 0.0)) return fail(OFLK_ERR_INVALID, "extent must be finite and > 0 (got %g)", extent);
    if ((T > 1 && !model) || !from_anchor || !to_anchor || !box || !dropped) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    return OFLK_OK;
}

// the one launch of the chain on stream s; the arguments are checked
int mosaic_chain_launch(const float *d_model, const int *d_counts, int T, int anchor, int H, int W, double extent, double *d_from,
                        double *d_to, double *d_box, unsigned char *d_held, unsigned char *d_dropped, hipStream_t s)
{
    hipLaunchKernelGGL(k_mosaic_chain, dim3(1), dim3(kMosaicChainBlock), 0, s, d_model, d_counts, T, anchor, H, W, extent, d_from, d_to,
                       d_box, d_held, d_dropped);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the one launch that adds F frames to the state on stream s; the arguments are checked.  d_exposure: NULL, or the frames'
// (eg, eb) of the exposure-compensated form
template <class PIX>
int mosaic_accumulate_launch(const PIX *d_frames, int F, int H, int W, const double *d_map, const unsigned char *d_skip, int x0, int y0,
                             int Hc, int Wc, int blend, void *d_state, hipStream_t s, const double *d_exposure = nullptr)
{
    MosaicExposureArgs<PIX> a{};
    a.exposure = d_exposure;
    a.in = d_frames; a.map = d_map; a.skip = d_skip;
    a.st = mosaic_state(d_state, Hc, Wc).st;
    a.F = F; a.H = H; a.W = W;
    a.x0 = x0; a.y0 = y0; a.Hc = Hc; a.Wc = Wc;
    a.tiles_x = (Wc + kMosaicTileW - 1) / kMosaicTileW;
    const dim3 grid((unsigned)a.tiles_x * (unsigned)((Hc + kMosaicBlockH - 1) / kMosaicBlockH));
    const bool built = with_int<kMosaicMean, kMosaicFeather, kMosaicFirst, kMosaicLast>(blend, [&](auto BLEND) {
        if (d_exposure)
            hipLaunchKernelGGL((k_mosaic_accumulate<PIX, decltype(BLEND)::value, true, MosaicExposureArgs<PIX>>), grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((k_mosaic_accumulate<PIX, decltype(BLEND)::value>), grid, dim3(256), 0, s,
                               static_cast<const MosaicArgs<PIX> &>(a));
    });
    if (!built) return fail(OFLK_ERR_INVALID, "unknown blend %d", blend);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

template <class PIX>
int mosaic_resolve_launch(void *d_state, int Hc, int Wc, PIX *d_out, int *d_count, hipStream_t s)
{
    MosaicResolveArgs<PIX> a{};
    a.st = mosaic_state(d_state, Hc, Wc).st;
    a.out = d_out; a.count = d_count; a.Hc = Hc; a.Wc = Wc;
    const bool vec = Wc % kMosaicPx == 0 && aligned(d_out, (unsigned)(kMosaicPx * sizeof(PIX))) && (!d_count || aligned(d_count, 16));
    const size_t quads = (size_t)Hc * (size_t)(a.st.Wp / kMosaicPx);
    const dim3 grid((unsigned)((quads + 255) / 256));
    if (vec)
        hipLaunchKernelGGL((k_mosaic_resolve<PIX, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_mosaic_resolve<PIX, false>), grid, dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// F host frames added to an empty state in chunks through one device buffer, then resolved into the host arrays.  A pixel's
// samples are added in frame order whatever the cut, so the cut does not show.
template <class PIX>
int mosaic_composite_chunks(HostCall &call, const PIX *frames, int F, int H, int W, const double *d_map, const unsigned char *d_skip,
                            int x0, int y0, int Hc, int Wc, int blend, PIX *out, int *count, const double *d_exposure = nullptr)
{
    const int C = sparse_chunk_pairs(F, H, W);
    const size_t plane = (size_t)H * W, npix = (size_t)Hc * Wc;
    const size_t bytes = mosaic_state(nullptr, Hc, Wc).bytes;
    PIX *d_in = nullptr, *d_out = nullptr;
    char *d_state = nullptr;
    int *d_count = nullptr;
    int rc;
    if ((rc = call.alloc(&d_in, (size_t)C * plane)) || (rc = call.alloc(&d_state, bytes)) || (rc = call.alloc(&d_out, npix)) ||
        (rc = call.alloc(&d_count, npix, count != nullptr)))
        return rc;
    HIP_TRY(hipMemsetAsync(d_state, 0, bytes, nullptr));
    for (int f0 = 0; f0 < F; f0 += C) {
        const int n = std::min(C, F - f0);
        if ((rc = call.to_device(d_in, frames + (size_t)f0 * plane, (size_t)n * plane)) ||
            (rc = mosaic_accumulate_launch<PIX>(d_in, n, H, W, d_map + 9 * (size_t)f0, d_skip ? d_skip + f0 : nullptr, x0, y0, Hc, Wc,
                                                blend, d_state, nullptr, d_exposure ? d_exposure + 2 * (size_t)f0 : nullptr)) ||
            (rc = call.sync()))
            return rc;
    }
    if ((rc = mosaic_resolve_launch<PIX>(d_state, Hc, Wc, d_out, d_count, nullptr)) || (rc = call.to_host(out, d_out, npix)) ||
        (count && (rc = call.to_host(count, d_count, npix))))
        return rc;
    return call.sync();
}

template <class PIX>
int mosaic_composite_host(const PIX *frames, int F, int H, int W, const double *map, const unsigned char *skip, int x0, int y0, int Hc,
                          int Wc, int blend, PIX *out, int *count, bool compensated = false, const double *exposure = nullptr)
{
    int rc = check_mosaic_frames(frames, F, H, W, map, Hc, Wc, blend);
    if (rc) return rc;
    if (!out) return fail(OFLK_ERR_INVALID, "NULL output argument");
    if (compensated && !exposure) return fail(OFLK_ERR_INVALID, "NULL exposure");
    HostCall call;
    if ((rc = call.begin())) return rc;
    double *d_map = nullptr, *d_exposure = nullptr;
    unsigned char *d_skip = nullptr;
    if ((rc = call.upload(&d_map, map, 9 * (size_t)F)) || (skip && (rc = call.upload(&d_skip, skip, (size_t)F))) ||
        (compensated && (rc = call.upload(&d_exposure, exposure, 2 * (size_t)F))))
        return rc;
    return mosaic_composite_chunks<PIX>(call, frames, F, H, W, d_map, d_skip, x0, y0, Hc, Wc, blend, out, count, d_exposure);
}

// oflk_mosaic_sequence: pass 1 is the replenish call itself, as in stabilize_sequence; the rows go up again for the
// homography fit and the chain; the boxes and drop flags come down for the canvas; pass 2 adds the frames chunk by chunk
template <class PIX>
int mosaic_sequence(const PIX *frames, int T, int H, int W, const KltConfig &klt, const FitConfig &fit, int anchor, double extent,
                    int blend, PIX *out, size_t capacity, int *canvas, int *count, double *to_anchor, unsigned char *held,
                    unsigned char *dropped, float *model_out, int *counts_out)
{
    if (T < 2) return fail(OFLK_ERR_INVALID, "a sequence needs T >= 2 frames (got %d)", T);
    if (!canvas) return fail(OFLK_ERR_INVALID, "NULL canvas");
    const int K = klt.select.K;
    int rc = check_frames(FrameLayout::planar(sizeof(PIX) == 1), frames, T, H, W, out);
    if (rc || (rc = check_ransac(fit)) || (rc = check_mosaic_blend(blend)) ||
        (rc = check_mosaic_chain(frames, T, anchor, H, W, extent, frames, frames, frames, frames)) || (rc = check_klt(H, W, klt)) ||
        (rc = check_motion_shape(T - 1, K)))
        return rc;
    const size_t nT = (size_t)T, S = nT - 1;
    std::vector<unsigned char> h_dropped;
    std::vector<double> h_box;
    try {
        h_box.resize(4 * nT);
        h_dropped.resize(nT);
    } catch (const std::exception &) {
        return fail(OFLK_ERR_NOMEM, "no host memory for the rows of %d frames of %d slots", T, K);
    }
    SequenceFit steps;   // before `call`: the host rows outlive the device buffers
    HostCall call;
    if ((rc = steps.run(call, frames, sizeof(PIX) == 1, T, H, W, klt, fit))) return rc;   // fit.model: kMotionHomography
    float *const d_model = steps.d_model;
    int *const d_cnt = steps.d_counts;
    unsigned char *d_held, *d_drop;
    double *d_from, *d_to, *d_box;
    if ((rc = call.alloc(&d_from, 9 * nT)) || (rc = call.alloc(&d_to, 9 * nT)) || (rc = call.alloc(&d_box, 4 * nT)) ||
        (rc = call.alloc(&d_held, S)) || (rc = call.alloc(&d_drop, nT)) ||
        (rc = mosaic_chain_launch(d_model, d_cnt, T, anchor, H, W, extent, d_from, d_to, d_box, d_held, d_drop, nullptr)))
        return rc;
    if ((rc = call.to_host(h_box.data(), d_box, 4 * nT)) || (rc = call.to_host(h_dropped.data(), d_drop, nT)) ||
        (to_anchor && (rc = call.to_host(to_anchor, d_to, 9 * nT))) || (held && (rc = call.to_host(held, d_held, S))) ||
        (model_out && (rc = call.to_host(model_out, d_model, 9 * S))) || (counts_out && (rc = call.to_host(counts_out, d_cnt, 3 * S))) ||
        (rc = call.sync()))
        return rc;
    if (dropped) std::memcpy(dropped, h_dropped.data(), nT);
    if ((rc = oflk_mosaic_canvas(h_box.data(), h_dropped.data(), T, &canvas[0], &canvas[1], &canvas[2], &canvas[3]))) return rc;
    const int x0 = canvas[0], y0 = canvas[1], Wc = canvas[2], Hc = canvas[3];
    if ((rc = check_mosaic_canvas(Hc, Wc))) return rc;
    if ((size_t)Hc * (size_t)Wc > capacity)
        return fail(OFLK_ERR_UNSUPPORTED, "the canvas of %d x %d pixels at (%d, %d) exceeds the capacity of %zu pixels", Wc, Hc, x0, y0,
                    capacity);
    return mosaic_composite_chunks<PIX>(call, frames, T, H, W, d_from, d_drop, x0, y0, Hc, Wc, blend, out, count);
}

// the temporal median's refusals: check_mosaic_frames' without the blend, then the pointers the median reads and writes
int check_mosaic_median(const void *frames, bool u8, int F, int H, int W, const double *map, const double *exposure, int Hc, int Wc,
                        const void *out)
{
    if (int rc = check_mosaic_frames(frames, F, H, W, map, Hc, Wc, OFLK_MOSAIC_MEAN)) return rc;
    if (!out) return fail(OFLK_ERR_INVALID, "NULL output argument");
    if (!aligned(map, 8) || !aligned(exposure, 8)) return fail(OFLK_ERR_INVALID, "the map and the exposure must be 8-byte aligned");
    if (!u8 && (!aligned(frames, 4) || !aligned(out, 4))) return fail(OFLK_ERR_INVALID, "float32 frames and output must be 4-byte aligned");
    return OFLK_OK;
}

// the one launch of the median on stream s; the arguments are checked.  d_exposure: NULL, or the frames' (eg, eb)
template <class PIX>
int mosaic_median_launch(const PIX *d_frames, int F, int H, int W, const double *d_map, const unsigned char *d_skip,
                         const double *d_exposure, int x0, int y0, int Hc, int Wc, PIX *d_out, int *d_count, hipStream_t s)
{
    MosaicMedianArgs<PIX> a{};
    a.in = d_frames; a.map = d_map; a.skip = d_skip; a.exposure = d_exposure;
    a.out = d_out; a.count = d_count;
    a.F = F; a.H = H; a.W = W;
    a.x0 = x0; a.y0 = y0; a.Hc = Hc; a.Wc = Wc;
    a.tiles_x = (Wc + kMedianBlockW - 1) / kMedianBlockW;
    const dim3 grid((unsigned)a.tiles_x * (unsigned)((Hc + kMedianTileH - 1) / kMedianTileH));
    if (d_exposure)
        hipLaunchKernelGGL((k_mosaic_median<PIX, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_mosaic_median<PIX, false>), grid, dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// host arrays: every frame goes up before the one launch -- a median needs all samples of a pixel at once
template <class PIX>
int mosaic_median_host(const PIX *frames, int F, int H, int W, const double *map, const unsigned char *skip, const double *exposure,
                       int x0, int y0, int Hc, int Wc, PIX *out, int *count)
{
    int rc = check_mosaic_median(frames, sizeof(PIX) == 1, F, H, W, map, exposure, Hc, Wc, out);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t plane = (size_t)H * W, npix = (size_t)Hc * Wc;
    double *d_map = nullptr, *d_exposure = nullptr;
    unsigned char *d_skip = nullptr;
    PIX *d_in = nullptr, *d_out = nullptr;
    int *d_count = nullptr;
    if ((rc = call.upload(&d_map, map, 9 * (size_t)F)) || (skip && (rc = call.upload(&d_skip, skip, (size_t)F))) ||
        (exposure && (rc = call.upload(&d_exposure, exposure, 2 * (size_t)F))) || (rc = call.upload(&d_in, frames, (size_t)F * plane)) ||
        (rc = call.alloc(&d_out, npix)) || (rc = call.alloc(&d_count, npix, count != nullptr)) ||
        (rc = mosaic_median_launch<PIX>(d_in, F, H, W, d_map, d_skip, d_exposure, x0, y0, Hc, Wc, d_out, d_count, nullptr)) ||
        (rc = call.to_host(out, d_out, npix)) || (count && (rc = call.to_host(count, d_count, npix))))
        return rc;
    return call.sync();
}
}  // namespace

OFLK_API size_t oflk_mosaic_state_bytes(int Hc, int Wc)
{
    if (Hc < 1 || Wc < 1 || (size_t)Hc * (size_t)Wc >= ((size_t)1 << 30)) return 0;
    return mosaic_state(nullptr, Hc, Wc).bytes;
}

OFLK_API int oflk_mosaic_chain(const float *d_model, const int *d_counts, int T, int anchor, int H, int W, double extent,
                               double *d_from_anchor, double *d_to_anchor, double *d_box, unsigned char *d_held,
                               unsigned char *d_dropped, void *stream)
{
    if (int rc = check_mosaic_chain(d_model, T, anchor, H, W, extent, d_from_anchor, d_to_anchor, d_box, d_dropped)) return rc;
    if (!aligned(d_from_anchor, 8) || !aligned(d_to_anchor, 8) || !aligned(d_box, 8))
        return fail(OFLK_ERR_INVALID, "d_from_anchor, d_to_anchor and d_box must be 8-byte aligned");
    return mosaic_chain_launch(d_model, d_counts, T, anchor, H, W, extent, d_from_anchor, d_to_anchor, d_box, d_held, d_dropped,
                               (hipStream_t)stream);
}

OFLK_API int oflk_mosaic_chain_host(const float *model, const int *counts, int T, int anchor, int H, int W, double extent,
                                    double *from_anchor, double *to_anchor, double *box, unsigned char *held, unsigned char *dropped)
{
    int rc = check_mosaic_chain(model, T, anchor, H, W, extent, from_anchor, to_anchor, box, dropped);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t nT = (size_t)T, S = nT - 1;
    float *d_model = nullptr;
    int *d_cnt = nullptr;
    double *d_from, *d_to, *d_box;
    unsigned char *d_held, *d_drop;
    if ((S && (rc = call.upload(&d_model, model, 9 * S))) || (S && counts && (rc = call.upload(&d_cnt, counts, 3 * S))) ||
        (rc = call.alloc(&d_from, 9 * nT)) || (rc = call.alloc(&d_to, 9 * nT)) || (rc = call.alloc(&d_box, 4 * nT)) ||
        (rc = call.alloc(&d_held, S, held && S)) || (rc = call.alloc(&d_drop, nT)))
        return rc;
    if ((rc = mosaic_chain_launch(d_model, d_cnt, T, anchor, H, W, extent, d_from, d_to, d_box, d_held, d_drop, nullptr))) return rc;
    if ((rc = call.to_host(from_anchor, d_from, 9 * nT)) || (rc = call.to_host(to_anchor, d_to, 9 * nT)) ||
        (rc = call.to_host(box, d_box, 4 * nT)) || (d_held && (rc = call.to_host(held, d_held, S))) ||
        (rc = call.to_host(dropped, d_drop, nT)))
        return rc;
    return call.sync();
}

OFLK_API int oflk_mosaic_canvas(const double *box, const unsigned char *dropped, int T, int *x0, int *y0, int *Wc, int *Hc)
{
    if (T < 1) return fail(OFLK_ERR_INVALID, "T must be >= 1 (got %d)", T);
    if (!box || !dropped || !x0 || !y0 || !Wc || !Hc) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    bool any = false;
    for (int t = 0; t < T; t++) {
        if (dropped[t]) continue;
        const double *b = box + 4 * (size_t)t;
        for (int k = 0; k < 4; k++)
            if (!std::isfinite(b[k])) return fail(OFLK_ERR_INVALID, "box[%d] of a frame that is not dropped is not finite", t);
        any = true;
        for (int k = 0; k < 2; k++) {
            lo[k] = std::min(lo[k], b[k]);
            hi[k] = std::max(hi[k], b[2 + k]);
        }
    }
    if (!any) return fail(OFLK_ERR_INVALID, "every frame is dropped");
    const double lim = (double)(1 << 30);
    for (int k = 0; k < 2; k++) {
        lo[k] = std::floor(lo[k]);
        hi[k] = std::ceil(hi[k]);
        if (!(lo[k] > -lim && hi[k] < lim && hi[k] >= lo[k]))
            return fail(OFLK_ERR_UNSUPPORTED, "a canvas from %g to %g is not supported", lo[k], hi[k]);
    }
    *x0 = (int)lo[0];
    *y0 = (int)lo[1];
    *Wc = (int)(hi[0] - lo[0]) + 1;
    *Hc = (int)(hi[1] - lo[1]) + 1;
    return OFLK_OK;
}

OFLK_API int oflk_mosaic_accumulate(const void *d_frames, int u8, int F, int H, int W, const double *d_map, const unsigned char *d_skip,
                                    int x0, int y0, int Hc, int Wc, int blend, void *d_state, size_t state_bytes, void *stream)
{
    if (int rc = check_mosaic_frames(d_frames, F, H, W, d_map, Hc, Wc, blend)) return rc;
    if (!d_state) return fail(OFLK_ERR_INVALID, "NULL d_state");
    if (!aligned(d_map, 8)) return fail(OFLK_ERR_INVALID, "d_map must be 8-byte aligned");
    if (!u8 && !aligned(d_frames, 4)) return fail(OFLK_ERR_INVALID, "float32 frames must be 4-byte aligned");
    const size_t need = mosaic_state(nullptr, Hc, Wc).bytes;
    if (state_bytes < need) return fail(OFLK_ERR_INVALID, "state of %zu bytes, %zu needed (oflk_mosaic_state_bytes)", state_bytes, need);
    if (!aligned(d_state, 256)) return fail(OFLK_ERR_INVALID, "d_state must be 256-byte aligned");
    return u8 ? mosaic_accumulate_launch<unsigned char>((const unsigned char *)d_frames, F, H, W, d_map, d_skip, x0, y0, Hc, Wc, blend,
                                                        d_state, (hipStream_t)stream)
              : mosaic_accumulate_launch<float>((const float *)d_frames, F, H, W, d_map, d_skip, x0, y0, Hc, Wc, blend, d_state,
                                                (hipStream_t)stream);
}

OFLK_API int oflk_mosaic_accumulate_exposure(const void *d_frames, int u8, int F, int H, int W, const double *d_map,
                                             const unsigned char *d_skip, const double *d_exposure, int x0, int y0, int Hc, int Wc,
                                             int blend, void *d_state, size_t state_bytes, void *stream)
{
    if (int rc = check_mosaic_frames(d_frames, F, H, W, d_map, Hc, Wc, blend)) return rc;
    if (!d_state || !d_exposure) return fail(OFLK_ERR_INVALID, "NULL d_state or d_exposure");
    if (!aligned(d_map, 8) || !aligned(d_exposure, 8)) return fail(OFLK_ERR_INVALID, "d_map and d_exposure must be 8-byte aligned");
    if (!u8 && !aligned(d_frames, 4)) return fail(OFLK_ERR_INVALID, "float32 frames must be 4-byte aligned");
    const size_t need = mosaic_state(nullptr, Hc, Wc).bytes;
    if (state_bytes < need) return fail(OFLK_ERR_INVALID, "state of %zu bytes, %zu needed (oflk_mosaic_state_bytes)", state_bytes, need);
    if (!aligned(d_state, 256)) return fail(OFLK_ERR_INVALID, "d_state must be 256-byte aligned");
    return u8 ? mosaic_accumulate_launch<unsigned char>((const unsigned char *)d_frames, F, H, W, d_map, d_skip, x0, y0, Hc, Wc, blend,
                                                        d_state, (hipStream_t)stream, d_exposure)
              : mosaic_accumulate_launch<float>((const float *)d_frames, F, H, W, d_map, d_skip, x0, y0, Hc, Wc, blend, d_state,
                                                (hipStream_t)stream, d_exposure);
}

OFLK_API int oflk_exposure_chain_host(const float *photo, const int *status, int T, int anchor, double *exposure)
{
    if (T < 1) return fail(OFLK_ERR_INVALID, "T must be >= 1 (got %d)", T);
    if (anchor < 0 || anchor >= T) return fail(OFLK_ERR_INVALID, "anchor must be in [0, %d) (got %d)", T, anchor);
    if ((T > 1 && !photo) || !exposure) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    // step t's (g, b) widened, or (1, 0) when the step is held
    auto step = [&](int t, double &g, double &b) {
        g = (double)photo[2 * (size_t)t];
        b = (double)photo[2 * (size_t)t + 1];
        if ((status && status[t] == 0) || !std::isfinite(g) || !std::isfinite(b) || !(g > 0.0)) {
            g = 1.0;
            b = 0.0;
        }
    };
    double *e = exposure;
    e[2 * (size_t)anchor] = 1.0;
    e[2 * (size_t)anchor + 1] = 0.0;
    for (int t = anchor; t < T - 1; t++) {
        double g, b;
        step(t, g, b);
        const double eg = e[2 * (size_t)t] / g;
        const double p = eg * b;
        e[2 * (size_t)t + 2] = eg;
        e[2 * (size_t)t + 3] = e[2 * (size_t)t + 1] - p;
    }
    for (int t = anchor - 1; t >= 0; t--) {
        double g, b;
        step(t, g, b);
        const double eg = e[2 * (size_t)t + 2];
        const double p = eg * b;
        e[2 * (size_t)t] = eg * g;
        e[2 * (size_t)t + 1] = p + e[2 * (size_t)t + 3];
    }
    return OFLK_OK;
}

OFLK_API int oflk_mosaic_resolve(const void *d_state, int Hc, int Wc, int u8, void *d_out, int *d_count, void *stream)
{
    if (int rc = check_mosaic_canvas(Hc, Wc)) return rc;
    if (!d_state || !d_out) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    if (!aligned(d_state, 256)) return fail(OFLK_ERR_INVALID, "d_state must be 256-byte aligned");
    if ((!u8 && !aligned(d_out, 4)) || (d_count && !aligned(d_count, 4)))
        return fail(OFLK_ERR_INVALID, "float32 output and d_count must be 4-byte aligned");
    void *st = const_cast<void *>(d_state);   // read only
    return u8 ? mosaic_resolve_launch<unsigned char>(st, Hc, Wc, (unsigned char *)d_out, d_count, (hipStream_t)stream)
              : mosaic_resolve_launch<float>(st, Hc, Wc, (float *)d_out, d_count, (hipStream_t)stream);
}

OFLK_API int oflk_mosaic_composite_host(const float *frames, int F, int H, int W, const double *map, const unsigned char *skip, int x0,
                                        int y0, int Hc, int Wc, int blend, float *out, int *count)
{
    return mosaic_composite_host<float>(frames, F, H, W, map, skip, x0, y0, Hc, Wc, blend, out, count);
}

OFLK_API int oflk_mosaic_composite_host_u8(const unsigned char *frames, int F, int H, int W, const double *map,
                                           const unsigned char *skip, int x0, int y0, int Hc, int Wc, int blend, unsigned char *out,
                                           int *count)
{
    return mosaic_composite_host<unsigned char>(frames, F, H, W, map, skip, x0, y0, Hc, Wc, blend, out, count);
}

OFLK_API int oflk_mosaic_composite_exposure_host(const float *frames, int F, int H, int W, const double *map,
                                                 const unsigned char *skip, const double *exposure, int x0, int y0, int Hc, int Wc,
                                                 int blend, float *out, int *count)
{
    return mosaic_composite_host<float>(frames, F, H, W, map, skip, x0, y0, Hc, Wc, blend, out, count, true, exposure);
}

OFLK_API int oflk_mosaic_composite_exposure_host_u8(const unsigned char *frames, int F, int H, int W, const double *map,
                                                    const unsigned char *skip, const double *exposure, int x0, int y0, int Hc,
                                                    int Wc, int blend, unsigned char *out, int *count)
{
    return mosaic_composite_host<unsigned char>(frames, F, H, W, map, skip, x0, y0, Hc, Wc, blend, out, count, true, exposure);
}

OFLK_API int oflk_mosaic_median_capacity(void) { return kMedianCap; }

OFLK_API int oflk_mosaic_median(const void *d_frames, int u8, int F, int H, int W, const double *d_map, const unsigned char *d_skip,
                                const double *d_exposure, int x0, int y0, int Hc, int Wc, void *d_out, int *d_count, void *stream)
{
    if (int rc = check_mosaic_median(d_frames, u8 != 0, F, H, W, d_map, d_exposure, Hc, Wc, d_out)) return rc;
    return u8 ? mosaic_median_launch<unsigned char>((const unsigned char *)d_frames, F, H, W, d_map, d_skip, d_exposure, x0, y0, Hc, Wc,
                                                    (unsigned char *)d_out, d_count, (hipStream_t)stream)
              : mosaic_median_launch<float>((const float *)d_frames, F, H, W, d_map, d_skip, d_exposure, x0, y0, Hc, Wc, (float *)d_out,
                                            d_count, (hipStream_t)stream);
}

OFLK_API int oflk_mosaic_median_host(const float *frames, int F, int H, int W, const double *map, const unsigned char *skip,
                                     const double *exposure, int x0, int y0, int Hc, int Wc, float *out, int *count)
{
    return mosaic_median_host<float>(frames, F, H, W, map, skip, exposure, x0, y0, Hc, Wc, out, count);
}

OFLK_API int oflk_mosaic_median_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, const unsigned char *skip,
                                        const double *exposure, int x0, int y0, int Hc, int Wc, unsigned char *out, int *count)
{
    return mosaic_median_host<unsigned char>(frames, F, H, W, map, skip, exposure, x0, y0, Hc, Wc, out, count);
}

OFLK_API int oflk_mosaic_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                                  float beta, float max_residual, float quality_level, float min_distance, int max_corners,
                                  int detect_every, int hypotheses, float threshold, unsigned seed, int anchor, double extent,
                                  int blend, float *out, size_t capacity, int *canvas, int *count, double *to_anchor,
                                  unsigned char *held, unsigned char *dropped, float *model_out, int *counts_out)
{
    return mosaic_sequence<float>(
        frames, T, H, W, {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
        {kMotionHomography, hypotheses, threshold, seed}, anchor, extent, blend, out, capacity, canvas, count, to_anchor, held, dropped,
        model_out, counts_out);
}

OFLK_API int oflk_mosaic_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                     float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                     int max_corners, int detect_every, int hypotheses, float threshold, unsigned seed, int anchor,
                                     double extent, int blend, unsigned char *out, size_t capacity, int *canvas, int *count,
                                     double *to_anchor, unsigned char *held, unsigned char *dropped, float *model_out, int *counts_out)
{
    return mosaic_sequence<unsigned char>(
        frames, T, H, W, {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
        {kMotionHomography, hypotheses, threshold, seed}, anchor, extent, blend, out, capacity, canvas, count, to_anchor, held, dropped,
        model_out, counts_out);
}

// =============================================================================
// direct image alignment: step models refined on pixel intensities (oflk_align.hpp)
// =============================================================================
namespace {
int align_coefficients(int model) { return model == OFLK_ALIGN_HOMOGRAPHY ? 9 : 6; }
int align_nsums(int model, bool photo, bool robust)
{
    return align_sums(model == OFLK_ALIGN_HOMOGRAPHY ? 8 : 6, photo, robust);
}
int align_tiles(int h, int w) { return ((w + kAlignTileW - 1) / kAlignTileW) * ((h + kAlignTileH - 1) / kAlignTileH); }

// One alignment call as every layer takes it: the configuration with its form (photometric, robust; check_align leaves
// robust_delta 0 without `robust`) and the steps' buffers, device or host: [S][6 | 9], [S] (or NULL), the same two out, stats
// [S][4 | 8] and the photometric form's (g, b) [S][2] (check_align leaves it NULL without `photo`)
struct AlignConfig { int levels, iterations, model; float min_share; bool photo, robust; float robust_delta; };
struct AlignIo { const float *model_in; const int *status_in; float *model_out; int *status_out; double *stats; float *photo_out; };

// the robust forms' own refusal
int check_robust_delta(float robust_delta)
{
    if (!(std::isfinite(robust_delta) && robust_delta > 0.0f))
        return fail(OFLK_ERR_INVALID, "robust_delta must be finite and > 0 (got %g)", (double)robust_delta);
    return OFLK_OK;
}

// the refusals of the steps' shape and model, which the weight map shares
int check_align_shape(int S, int H, int W, int model)
{
    if (S < 1) return fail(OFLK_ERR_INVALID, "S must be >= 1 (got %d)", S);
    if (H < 1 || W < 1) return fail(OFLK_ERR_INVALID, "H and W must be >= 1 (got %d x %d)", H, W);
    if ((size_t)H * (size_t)W >= ((size_t)1 << 30)) return fail(OFLK_ERR_UNSUPPORTED, "frames of 2^30 pixels or more are not supported");
    if (H >= kMaxDim || W >= kMaxDim)
        return fail(OFLK_ERR_UNSUPPORTED, "frames of 2^23 rows or columns or more are not supported (got %d x %d)", H, W);
    if (model != OFLK_ALIGN_AFFINE && model != OFLK_ALIGN_HOMOGRAPHY) return fail(OFLK_ERR_INVALID, "unknown model %d", model);
    return OFLK_OK;
}

// The refusals of the configuration, before any device call; dims receives the level sizes.  What a form does not have is
// taken out of cfg and io: the layers below tell the form by them
int check_align(int S, int H, int W, AlignConfig &cfg, AlignIo &io, int *dims)
{
    if (int rc = check_align_shape(S, H, W, cfg.model)) return rc;
    if (cfg.iterations < 1) return fail(OFLK_ERR_INVALID, "iterations must be >= 1 (got %d)", cfg.iterations);
    const int levels = cfg.levels;
    if (!(cfg.min_share > 0.0f && cfg.min_share <= 1.0f)) return fail(OFLK_ERR_INVALID, "min_share must be in (0, 1] (got %g)", (double)cfg.min_share);
    if (levels < 1 || levels > OFLK_MAX_LEVELS) return fail(OFLK_ERR_INVALID, "levels must be in [1,%d] (got %d)", OFLK_MAX_LEVELS, levels);
    int h = H, w = W;
    for (int l = levels - 1; l >= 0; l--) {
        if (h < 8 || w < 8)
            return fail(OFLK_ERR_UNSUPPORTED, "pyramid level %d of %dx%d would be %dx%d: the alignment needs 8 x 8", l, W, H, w, h);
        dims[2 * l] = h;
        dims[2 * l + 1] = w;
        h = (int)((double)h * 0.5);
        w = (int)((double)w * 0.5);
    }
    if (!cfg.robust) cfg.robust_delta = 0.0f;
    if (!cfg.photo) io.photo_out = nullptr;
    return cfg.robust ? check_robust_delta(cfg.robust_delta) : OFLK_OK;
}

// The workspace, 256-byte aligned pieces: the steps' states [S], the tile sums [S][tiles of the frame][NS], and per level
// below the frame 2 S images (the pair form: S of A, then S of B; the sequence form: the first S + 1 hold its frames').  The
// photometric form has more sums per tile and, behind everything else, the steps' (g, b) [S][2].  The robust form has two
// more sums per tile and, last, the first pass's r r / count and sum(w) / count [S][2]
struct AlignWs {
    AlignState *state;
    double *partial;
    float *pyr[OFLK_MAX_LEVELS];
    double *photo;
    double *first;
    size_t pstride, bytes;
};

AlignWs align_ws(void *base, int S, const int *dims, const AlignConfig &cfg)
{
    const int levels = cfg.levels;
    char *b = static_cast<char *>(base);
    auto at = [&](size_t o) { return b ? b + o : nullptr; };   // NULL: only the size is wanted
    AlignWs ws{};
    size_t o = 0;
    ws.state = reinterpret_cast<AlignState *>(at(o));
    o += round256((size_t)S * sizeof(AlignState));
    ws.pstride = (size_t)align_tiles(dims[2 * (levels - 1)], dims[2 * (levels - 1) + 1]) * (size_t)align_nsums(cfg.model, cfg.photo, cfg.robust);
    ws.partial = reinterpret_cast<double *>(at(o));
    o += round256((size_t)S * ws.pstride * sizeof(double));
    for (int l = 0; l < levels - 1; l++) {
        ws.pyr[l] = reinterpret_cast<float *>(at(o));
        o += round256(2 * (size_t)S * (size_t)dims[2 * l] * (size_t)dims[2 * l + 1] * sizeof(float));
    }
    if (cfg.photo) {
        ws.photo = reinterpret_cast<double *>(at(o));
        o += round256(2 * (size_t)S * sizeof(double));
    }
    if (cfg.robust) {
        ws.first = reinterpret_cast<double *>(at(o));
        o += round256(2 * (size_t)S * sizeof(double));
    }
    ws.bytes = o;
    return ws;
}

int check_align_device(const void *d_a, const void *d_b, int u8, const void *d_model_in, const void *d_ws, size_t bytes, size_t need,
                       const void *d_model_out, const void *d_status_out, const void *d_stats)
{
    if (!d_a || !d_b || !d_model_in || !d_ws || !d_model_out || !d_status_out || !d_stats)
        return fail(OFLK_ERR_INVALID, "NULL input, workspace or output argument");
    if (bytes < need) return fail(OFLK_ERR_INVALID, "workspace of %zu bytes, %zu needed (oflk_align_workspace)", bytes, need);
    if (!aligned(d_ws, 256) || !aligned(d_stats, 8)) return fail(OFLK_ERR_INVALID, "d_workspace must be 256-byte aligned, d_stats 8-byte aligned");
    if (!u8 && (!aligned(d_a, 4) || !aligned(d_b, 4))) return fail(OFLK_ERR_INVALID, "float32 frames must be 4-byte aligned");
    return OFLK_OK;
}

// r.photo: NULL, or the steps' (g, b) of the photometric form.  r.delta > 0: the robust form
template <class PIX, int NP>
int align_reduce_launch(const AlignReduceArgs &r, int tiles, hipStream_t s)
{
    const dim3 grid((unsigned)tiles, (unsigned)std::min(r.S, 65535));
    with_bool(r.photo != nullptr, [&](auto PHOTO) {
        with_bool(r.delta > 0.0, [&](auto ROBUST) {
            constexpr bool photo = decltype(PHOTO)::value;
            hipLaunchKernelGGL((k_align_reduce<PIX, NP, photo, decltype(ROBUST)::value>), grid, dim3(64 * align_waves(NP, photo)), 0, s, r);
        });
    });
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// The whole chain of one call on stream s; the arguments are checked.  d_a, d_b: the S templates and images, `step` elements
// apart (the pair form: two arrays of S frames; the sequence form: d_b = d_a + one frame).  nimg > 0: the sequence form's
// nimg = S + 1 frames, whose pyramids are built once.  cfg and io are check_align's: io.photo_out is NULL or the
// photometric form's output, cfg.robust_delta > 0 in the robust form (io.stats [S][8]), and ws is that form's workspace
template <class PIX, int NP>
int align_launch(const PIX *d_a, const PIX *d_b, int nimg, int S, int H, int W, const int *dims, const AlignConfig &cfg,
                 const AlignIo &io, const AlignWs &ws, hipStream_t s)
{
    const int levels = cfg.levels, iterations = cfg.iterations;
    const double delta = (double)cfg.robust_delta;
    constexpr int NC = NP == 8 ? 9 : 6;
    const bool seq = nimg > 0;
    const int n = seq ? nimg : 2 * S;
    int rc;
    if (levels > 1) {
        GaussW gauss;
        if ((rc = make_gauss(2.0, &gauss)) || (rc = pyr_chain_fits(dims, levels, gauss))) return rc;
        PyrExtra first;
        first.u8 = sizeof(PIX) == 1;
        if (!seq) {
            first.in2 = reinterpret_cast<const float *>(d_b);
            first.nsplit = S;
        }
        if ((rc = pyr_chain(nullptr, gauss, s, reinterpret_cast<const float *>(d_a), ws.pyr, 0, nullptr, nullptr, n, dims, levels, first)))
            return rc;
    }
    hipLaunchKernelGGL(k_align_begin, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, io.model_in, io.status_in, S, NC, ws.state);
    HIP_TRY(hipGetLastError());
    const double *photo = io.photo_out ? ws.photo : nullptr;
    if (photo) {
        hipLaunchKernelGGL(k_align_photo_begin, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, S, ws.photo);
        HIP_TRY(hipGetLastError());
    }

    // the sums of level l under the steps' current models, then the update of the given mode
    auto pass = [&](int l, int mode, int last, int next) -> int {
        const int h = dims[2 * l], w = dims[2 * l + 1];
        AlignReduceArgs r{};
        r.stride = (size_t)h * (size_t)w;
        r.H = h; r.W = w; r.tiles_x = (w + kAlignTileW - 1) / kAlignTileW; r.S = S;
        r.skip_frozen = mode == kAlignIterate;
        r.state = ws.state; r.partial = ws.partial; r.pstride = ws.pstride;
        r.photo = photo; r.delta = delta;
        const int tiles = align_tiles(h, w);
        int rc2;
        if (l == levels - 1) {
            r.a = d_a;
            r.b = d_b;
            rc2 = align_reduce_launch<PIX, NP>(r, tiles, s);
        } else {
            r.a = ws.pyr[l];
            r.b = ws.pyr[l] + (seq ? 1 : (size_t)S) * r.stride;
            rc2 = align_reduce_launch<float, NP>(r, tiles, s);
        }
        if (rc2) return rc2;
        AlignUpdateArgs u{};
        u.state = ws.state; u.partial = ws.partial; u.pstride = ws.pstride;
        u.tiles = tiles; u.S = S; u.mode = mode;
        u.H = H; u.W = W; u.h = h; u.w = w;
        u.last = last;
        if (next >= 0) {
            u.nh = dims[2 * next];
            u.nw = dims[2 * next + 1];
        }
        u.min_count = (double)cfg.min_share * (double)((long long)w * (long long)h);
        u.model_in = io.model_in; u.model_out = io.model_out; u.status_out = io.status_out; u.stats = io.stats;
        u.photo = photo ? ws.photo : nullptr; u.photo_out = io.photo_out; u.first = ws.first;
        with_bool(photo != nullptr, [&](auto PHOTO) {
            with_bool(delta > 0.0, [&](auto ROBUST) {
                hipLaunchKernelGGL((k_align_update<NP, decltype(PHOTO)::value, decltype(ROBUST)::value>), dim3((unsigned)std::min(S, 65535)),
                                   dim3(64), 0, s, u);
            });
        });
        HIP_TRY(hipGetLastError());
        return OFLK_OK;
    };
    if ((rc = pass(levels - 1, kAlignFirst, 0, 0))) return rc;
    for (int l = 0; l < levels; l++)
        for (int k = 0; k < iterations; k++) {
            const bool last = k == iterations - 1;
            if ((rc = pass(l, kAlignIterate, last, last ? (l + 1 < levels ? l + 1 : -1) : -1))) return rc;
        }
    return pass(levels - 1, kAlignLast, 0, -1);
}

// the affine or the homography instantiation of align_launch, by cfg.model
template <class PIX>
int align_dispatch(const PIX *d_a, const PIX *d_b, int nimg, int S, int H, int W, const int *dims, const AlignConfig &cfg,
                   const AlignIo &io, const AlignWs &ws, hipStream_t s)
{
    int rc = OFLK_OK;
    with_int<6, 8>(cfg.model == OFLK_ALIGN_HOMOGRAPHY ? 8 : 6,
                   [&](auto NP) { rc = align_launch<PIX, decltype(NP)::value>(d_a, d_b, nimg, S, H, W, dims, cfg, io, ws, s); });
    return rc;
}

// The steps of a call: the n pairs of (a, b), or (seq) the n - 1 steps of the n frames at a.  The sequence forms' first
// refusal; with b, their second image set: the frames one plane on (a NULL, or a shape that is refused later, stays as it is)
int align_steps(bool seq, int n, const void *a, const void **b, size_t pix_bytes, int H, int W, int *S)
{
    if (seq && n < 2) return fail(OFLK_ERR_INVALID, "a sequence needs T >= 2 frames (got %d)", n);
    *S = seq ? n - 1 : n;
    if (seq && b) *b = a && H > 0 && W > 0 ? static_cast<const char *>(a) + (size_t)H * (size_t)W * pix_bytes : a;
    return OFLK_OK;
}

// Every device form.  n: the S pairs of d_a and d_b, or (seq) the T frames at d_a
int align_device(const void *d_a, const void *d_b, int u8, bool seq, int n, int H, int W, AlignConfig cfg, AlignIo io,
                 void *d_workspace, size_t bytes, void *stream)
{
    int dims[2 * OFLK_MAX_LEVELS], S;
    int rc = align_steps(seq, n, d_a, &d_b, u8 ? 1 : sizeof(float), H, W, &S);
    if (rc || (rc = check_align(S, H, W, cfg, io, dims))) return rc;
    const size_t need = align_ws(nullptr, S, dims, cfg).bytes;
    if ((rc = check_align_device(d_a, d_b, u8, io.model_in, d_workspace, bytes, need, io.model_out, io.status_out, io.stats))) return rc;
    if (cfg.photo && !io.photo_out) return fail(OFLK_ERR_INVALID, "NULL d_photo_out");
    if (cfg.photo && !aligned(io.photo_out, 4)) return fail(OFLK_ERR_INVALID, "d_photo_out must be 4-byte aligned");
    const AlignWs ws = align_ws(d_workspace, S, dims, cfg);
    with_pix(u8 != 0, [&](auto PIX) {
        using P = typename decltype(PIX)::type;
        rc = align_dispatch<P>(static_cast<const P *>(d_a), static_cast<const P *>(d_b), seq ? n : 0, S, H, W, dims, cfg, io, ws,
                               (hipStream_t)stream);
    });
    return rc;
}

// Every host form, n_in as align_device's n.  The S steps go in chunks through one set of device buffers: a chunk's frames go up,
// its steps are refined and the models, statuses and stats of all steps come down at the end.  Steps are independent and a frame's
// pyramid depends on the frame alone, so the cut does not show.  seq: a chunk of n steps takes its n + 1 frames (b is unused)
template <class PIX>
int align_host(const PIX *a, const PIX *b, bool seq, int n_in, int H, int W, AlignConfig cfg, AlignIo io)
{
    int dims[2 * OFLK_MAX_LEVELS], S;
    int rc = align_steps(seq, n_in, a, nullptr, sizeof(PIX), H, W, &S);
    if (rc || (rc = check_align(S, H, W, cfg, io, dims))) return rc;
    const bool photo = cfg.photo;
    const size_t ns = cfg.robust ? 8 : 4;   // a step's stats
    if (!a || (!seq && !b) || !io.model_in || !io.model_out || !io.status_out || !io.stats || (photo && !io.photo_out))
        return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int C = sparse_chunk_pairs(S, H, W), nc = align_coefficients(cfg.model);
    const size_t plane = (size_t)H * W, nS = (size_t)S;
    PIX *d_a = nullptr, *d_b = nullptr;
    float *d_min = nullptr, *d_mout = nullptr, *d_photo = nullptr;
    int *d_sin = nullptr, *d_sout = nullptr;
    double *d_stats = nullptr;
    char *d_ws = nullptr;
    const size_t bytes = align_ws(nullptr, C, dims, cfg).bytes;
    if ((rc = call.alloc(&d_a, (size_t)(C + (seq ? 1 : 0)) * plane)) || (rc = call.alloc(&d_b, (size_t)C * plane, !seq)) ||
        (rc = call.upload(&d_min, io.model_in, nc * nS)) || (io.status_in && (rc = call.upload(&d_sin, io.status_in, nS))) ||
        (rc = call.alloc(&d_mout, nc * nS)) || (rc = call.alloc(&d_sout, nS)) || (rc = call.alloc(&d_stats, ns * nS)) ||
        (rc = call.alloc(&d_ws, bytes)) || (rc = call.alloc(&d_photo, 2 * nS, photo)))
        return rc;
    for (int s0 = 0; s0 < S; s0 += C) {
        const int n = std::min(C, S - s0);
        const size_t o = (size_t)s0 * plane;
        if ((rc = call.to_device(d_a, a + o, (size_t)(n + (seq ? 1 : 0)) * plane)) ||
            (!seq && (rc = call.to_device(d_b, b + o, (size_t)n * plane))))
            return rc;
        const AlignIo d_io{d_min + (size_t)nc * s0, d_sin ? d_sin + s0 : nullptr, d_mout + (size_t)nc * s0,
                           d_sout + s0,             d_stats + ns * (size_t)s0,    photo ? d_photo + 2 * (size_t)s0 : nullptr};
        const AlignWs ws = align_ws(d_ws, n, dims, cfg);
        if ((rc = align_dispatch<PIX>(d_a, seq ? d_a + plane : d_b, seq ? n + 1 : 0, n, H, W, dims, cfg, d_io, ws, nullptr)) ||
            (rc = call.sync()))
            return rc;
    }
    if ((rc = call.to_host(io.model_out, d_mout, nc * nS)) || (rc = call.to_host(io.status_out, d_sout, nS)) ||
        (rc = call.to_host(io.stats, d_stats, ns * nS)) || (photo && (rc = call.to_host(io.photo_out, d_photo, 2 * nS))))
        return rc;
    return call.sync();
}

// the three workspace calls
int align_workspace(int S, int H, int W, int levels, int model, bool photo, bool robust, size_t *bytes)
{
    if (!bytes) return fail(OFLK_ERR_INVALID, "bytes is NULL");
    *bytes = 0;
    int dims[2 * OFLK_MAX_LEVELS];
    AlignConfig cfg{levels, 1, model, 1.0f, photo, robust, 1.0f};   // iterations, min_share, robust_delta: values that pass
    AlignIo none{};
    if (int rc = check_align(S, H, W, cfg, none, dims)) return rc;
    *bytes = align_ws(nullptr, S, dims, cfg).bytes;
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_align_workspace(int S, int H, int W, int levels, int model, size_t *bytes)
{
    return align_workspace(S, H, W, levels, model, false, false, bytes);
}

OFLK_API int oflk_align_refine(const void *d_a, const void *d_b, int u8, int S, int H, int W, int levels, int iterations, int model,
                               float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace,
                               size_t workspace_bytes, float *d_model_out, int *d_status_out, double *d_stats, void *stream)
{
    return align_device(d_a, d_b, u8, false, S, H, W, {levels, iterations, model, min_share, false, false, 0.0f},
                        {d_model_in, d_status_in, d_model_out, d_status_out, d_stats, nullptr}, d_workspace, workspace_bytes, stream);
}

OFLK_API int oflk_align_sequence(const void *d_frames, int u8, int T, int H, int W, int levels, int iterations, int model,
                                 float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace,
                                 size_t workspace_bytes, float *d_model_out, int *d_status_out, double *d_stats, void *stream)
{
    return align_device(d_frames, nullptr, u8, true, T, H, W, {levels, iterations, model, min_share, false, false, 0.0f},
                        {d_model_in, d_status_in, d_model_out, d_status_out, d_stats, nullptr}, d_workspace, workspace_bytes, stream);
}

OFLK_API int oflk_align_refine_host(const float *a, const float *b, int S, int H, int W, int levels, int iterations, int model,
                                    float min_share, const float *model_in, const int *status_in, float *model_out,
                                    int *status_out, double *stats)
{
    return align_host<float>(a, b, false, S, H, W, {levels, iterations, model, min_share, false, false, 0.0f},
                             {model_in, status_in, model_out, status_out, stats, nullptr});
}

OFLK_API int oflk_align_refine_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int levels,
                                       int iterations, int model, float min_share, const float *model_in, const int *status_in,
                                       float *model_out, int *status_out, double *stats)
{
    return align_host<unsigned char>(a, b, false, S, H, W, {levels, iterations, model, min_share, false, false, 0.0f},
                                     {model_in, status_in, model_out, status_out, stats, nullptr});
}

OFLK_API int oflk_align_sequence_host(const float *frames, int T, int H, int W, int levels, int iterations, int model,
                                      float min_share, const float *model_in, const int *status_in, float *model_out,
                                      int *status_out, double *stats)
{
    return align_host<float>(frames, nullptr, true, T, H, W, {levels, iterations, model, min_share, false, false, 0.0f},
                             {model_in, status_in, model_out, status_out, stats, nullptr});
}

OFLK_API int oflk_align_sequence_host_u8(const unsigned char *frames, int T, int H, int W, int levels, int iterations, int model,
                                         float min_share, const float *model_in, const int *status_in, float *model_out,
                                         int *status_out, double *stats)
{
    return align_host<unsigned char>(frames, nullptr, true, T, H, W, {levels, iterations, model, min_share, false, false, 0.0f},
                                     {model_in, status_in, model_out, status_out, stats, nullptr});
}

OFLK_API int oflk_align_photo_workspace(int S, int H, int W, int levels, int model, size_t *bytes)
{
    return align_workspace(S, H, W, levels, model, true, false, bytes);
}

OFLK_API int oflk_align_refine_photo(const void *d_a, const void *d_b, int u8, int S, int H, int W, int levels, int iterations,
                                     int model, float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace,
                                     size_t workspace_bytes, float *d_model_out, int *d_status_out, double *d_stats,
                                     float *d_photo_out, void *stream)
{
    return align_device(d_a, d_b, u8, false, S, H, W, {levels, iterations, model, min_share, true, false, 0.0f},
                        {d_model_in, d_status_in, d_model_out, d_status_out, d_stats, d_photo_out}, d_workspace, workspace_bytes, stream);
}

OFLK_API int oflk_align_sequence_photo(const void *d_frames, int u8, int T, int H, int W, int levels, int iterations, int model,
                                       float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace,
                                       size_t workspace_bytes, float *d_model_out, int *d_status_out, double *d_stats,
                                       float *d_photo_out, void *stream)
{
    return align_device(d_frames, nullptr, u8, true, T, H, W, {levels, iterations, model, min_share, true, false, 0.0f},
                        {d_model_in, d_status_in, d_model_out, d_status_out, d_stats, d_photo_out}, d_workspace, workspace_bytes, stream);
}

OFLK_API int oflk_align_refine_photo_host(const float *a, const float *b, int S, int H, int W, int levels, int iterations, int model,
                                          float min_share, const float *model_in, const int *status_in, float *model_out,
                                          int *status_out, double *stats, float *photo_out)
{
    return align_host<float>(a, b, false, S, H, W, {levels, iterations, model, min_share, true, false, 0.0f},
                             {model_in, status_in, model_out, status_out, stats, photo_out});
}

OFLK_API int oflk_align_refine_photo_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int levels,
                                             int iterations, int model, float min_share, const float *model_in, const int *status_in,
                                             float *model_out, int *status_out, double *stats, float *photo_out)
{
    return align_host<unsigned char>(a, b, false, S, H, W, {levels, iterations, model, min_share, true, false, 0.0f},
                                     {model_in, status_in, model_out, status_out, stats, photo_out});
}

OFLK_API int oflk_align_sequence_photo_host(const float *frames, int T, int H, int W, int levels, int iterations, int model,
                                            float min_share, const float *model_in, const int *status_in, float *model_out,
                                            int *status_out, double *stats, float *photo_out)
{
    return align_host<float>(frames, nullptr, true, T, H, W, {levels, iterations, model, min_share, true, false, 0.0f},
                             {model_in, status_in, model_out, status_out, stats, photo_out});
}

OFLK_API int oflk_align_sequence_photo_host_u8(const unsigned char *frames, int T, int H, int W, int levels, int iterations,
                                               int model, float min_share, const float *model_in, const int *status_in,
                                               float *model_out, int *status_out, double *stats, float *photo_out)
{
    return align_host<unsigned char>(frames, nullptr, true, T, H, W, {levels, iterations, model, min_share, true, false, 0.0f},
                                     {model_in, status_in, model_out, status_out, stats, photo_out});
}

// ---- the robust forms ----
OFLK_API int oflk_align_robust_workspace(int S, int H, int W, int levels, int model, int photometric, size_t *bytes)
{
    return align_workspace(S, H, W, levels, model, photometric != 0, true, bytes);
}

OFLK_API int oflk_align_refine_robust(const void *d_a, const void *d_b, int u8, int S, int H, int W, int levels, int iterations,
                                      int model, float min_share, float robust_delta, int photometric, const float *d_model_in,
                                      const int *d_status_in, void *d_workspace, size_t workspace_bytes, float *d_model_out,
                                      int *d_status_out, double *d_stats, float *d_photo_out, void *stream)
{
    return align_device(d_a, d_b, u8, false, S, H, W, {levels, iterations, model, min_share, photometric != 0, true, robust_delta},
                        {d_model_in, d_status_in, d_model_out, d_status_out, d_stats, d_photo_out}, d_workspace, workspace_bytes, stream);
}

OFLK_API int oflk_align_sequence_robust(const void *d_frames, int u8, int T, int H, int W, int levels, int iterations, int model,
                                        float min_share, float robust_delta, int photometric, const float *d_model_in,
                                        const int *d_status_in, void *d_workspace, size_t workspace_bytes, float *d_model_out,
                                        int *d_status_out, double *d_stats, float *d_photo_out, void *stream)
{
    return align_device(d_frames, nullptr, u8, true, T, H, W, {levels, iterations, model, min_share, photometric != 0, true, robust_delta},
                        {d_model_in, d_status_in, d_model_out, d_status_out, d_stats, d_photo_out}, d_workspace, workspace_bytes, stream);
}

OFLK_API int oflk_align_refine_robust_host(const float *a, const float *b, int S, int H, int W, int levels, int iterations, int model,
                                           float min_share, float robust_delta, int photometric, const float *model_in,
                                           const int *status_in, float *model_out, int *status_out, double *stats, float *photo_out)
{
    return align_host<float>(a, b, false, S, H, W, {levels, iterations, model, min_share, photometric != 0, true, robust_delta},
                             {model_in, status_in, model_out, status_out, stats, photo_out});
}

OFLK_API int oflk_align_refine_robust_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int levels,
                                              int iterations, int model, float min_share, float robust_delta, int photometric,
                                              const float *model_in, const int *status_in, float *model_out, int *status_out,
                                              double *stats, float *photo_out)
{
    return align_host<unsigned char>(a, b, false, S, H, W, {levels, iterations, model, min_share, photometric != 0, true, robust_delta},
                                     {model_in, status_in, model_out, status_out, stats, photo_out});
}

OFLK_API int oflk_align_sequence_robust_host(const float *frames, int T, int H, int W, int levels, int iterations, int model,
                                             float min_share, float robust_delta, int photometric, const float *model_in,
                                             const int *status_in, float *model_out, int *status_out, double *stats, float *photo_out)
{
    return align_host<float>(frames, nullptr, true, T, H, W, {levels, iterations, model, min_share, photometric != 0, true, robust_delta},
                             {model_in, status_in, model_out, status_out, stats, photo_out});
}

OFLK_API int oflk_align_sequence_robust_host_u8(const unsigned char *frames, int T, int H, int W, int levels, int iterations,
                                                int model, float min_share, float robust_delta, int photometric,
                                                const float *model_in, const int *status_in, float *model_out, int *status_out,
                                                double *stats, float *photo_out)
{
    return align_host<unsigned char>(frames, nullptr, true, T, H, W, {levels, iterations, model, min_share, photometric != 0, true, robust_delta},
                                     {model_in, status_in, model_out, status_out, stats, photo_out});
}

// ---- the weight map ----
namespace {
// the refusals of the weight map's configuration, before any device call
int check_align_weights(int S, int H, int W, int model, float robust_delta)
{
    if (int rc = check_align_shape(S, H, W, model)) return rc;
    return check_robust_delta(robust_delta);
}

template <class PIX, int NP>
int align_weights_launch(const AlignWeightsArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)(((size_t)a.H * (size_t)a.W + 255) / 256), (unsigned)std::min(a.S, 65535));
    if (a.photo)
        hipLaunchKernelGGL((k_align_weights<PIX, NP, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_align_weights<PIX, NP, false>), grid, dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the arguments are checked
int align_weights_dispatch(const void *d_a, const void *d_b, bool u8, int S, int H, int W, int model, float robust_delta,
                           const float *d_model, const float *d_photo, float *d_weights, hipStream_t s)
{
    AlignWeightsArgs a{};
    a.a = d_a; a.b = d_b;
    a.H = H; a.W = W; a.S = S;
    a.model = d_model; a.photo = d_photo;
    a.delta = (double)robust_delta;
    a.weights = d_weights;
    if (model == OFLK_ALIGN_HOMOGRAPHY) return u8 ? align_weights_launch<unsigned char, 8>(a, s) : align_weights_launch<float, 8>(a, s);
    return u8 ? align_weights_launch<unsigned char, 6>(a, s) : align_weights_launch<float, 6>(a, s);
}

template <class PIX>
int align_weights_host(const PIX *a, const PIX *b, int S, int H, int W, int model, float robust_delta, const float *model_in,
                       const float *photo, float *weights)
{
    int rc = check_align_weights(S, H, W, model, robust_delta);
    if (rc) return rc;
    if (!a || !b || !model_in || !weights) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    HostCall call;
    if ((rc = call.begin())) return rc;
    const int C = sparse_chunk_pairs(S, H, W), nc = align_coefficients(model);
    const size_t plane = (size_t)H * W, nS = (size_t)S;
    PIX *d_a = nullptr, *d_b = nullptr;
    float *d_model = nullptr, *d_photo = nullptr, *d_w = nullptr;
    if ((rc = call.alloc(&d_a, (size_t)C * plane)) || (rc = call.alloc(&d_b, (size_t)C * plane)) ||
        (rc = call.upload(&d_model, model_in, nc * nS)) || (photo && (rc = call.upload(&d_photo, photo, 2 * nS))) ||
        (rc = call.alloc(&d_w, (size_t)C * plane)))
        return rc;
    for (int s0 = 0; s0 < S; s0 += C) {
        const int n = std::min(C, S - s0);
        const size_t o = (size_t)s0 * plane;
        if ((rc = call.to_device(d_a, a + o, (size_t)n * plane)) || (rc = call.to_device(d_b, b + o, (size_t)n * plane)) ||
            (rc = align_weights_dispatch(d_a, d_b, sizeof(PIX) == 1, n, H, W, model, robust_delta, d_model + (size_t)nc * s0,
                                         d_photo ? d_photo + 2 * (size_t)s0 : nullptr, d_w, nullptr)) ||
            (rc = call.to_host(weights + o, d_w, (size_t)n * plane)) || (rc = call.sync()))
            return rc;
    }
    return call.sync();
}
}  // namespace

OFLK_API int oflk_align_weights(const void *d_a, const void *d_b, int u8, int S, int H, int W, int model, float robust_delta,
                                const float *d_model, const float *d_photo, float *d_weights, void *stream)
{
    if (int rc = check_align_weights(S, H, W, model, robust_delta)) return rc;
    if (!d_a || !d_b || !d_model || !d_weights) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    if (!aligned(d_model, 4) || !aligned(d_weights, 4) || (d_photo && !aligned(d_photo, 4)) || (!u8 && (!aligned(d_a, 4) || !aligned(d_b, 4))))
        return fail(OFLK_ERR_INVALID, "float32 arguments must be 4-byte aligned");
    return align_weights_dispatch(d_a, d_b, u8 != 0, S, H, W, model, robust_delta, d_model, d_photo, d_weights, (hipStream_t)stream);
}

OFLK_API int oflk_align_weights_host(const float *a, const float *b, int S, int H, int W, int model, float robust_delta,
                                     const float *model_in, const float *photo, float *weights)
{
    return align_weights_host<float>(a, b, S, H, W, model, robust_delta, model_in, photo, weights);
}

OFLK_API int oflk_align_weights_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int model,
                                        float robust_delta, const float *model_in, const float *photo, float *weights)
{
    return align_weights_host<unsigned char>(a, b, S, H, W, model, robust_delta, model_in, photo, weights);
}

// =============================================================================
// online sparse KLT tracker: one frame per push
// =============================================================================
// The state of a tracker.  Creation checks and records the configuration and makes no device call; the first push
// allocates everything (ensure_state), and no later push allocates.  Frame t lives in ring slot t & 1, and so do its
// pyramid levels and its row.
struct oflk_tracker {
    int device = 0, H = 0, W = 0;
    bool u8 = false;
    KltConfig klt{};   // the configuration, as oflk_tracker_create took it: klt.select.K slots; klt.select.every = 0: never detect
    int dims[2 * OFLK_MAX_LEVELS] = {0};
    GaussW gauss;
    long long t = -1;                 // index of the last pushed frame
    bool ready = false;               // the device state exists
    bool failed = false;              // a push failed part-way: pushes are refused until reset
    size_t ws_bytes = 0;
    void *ring = nullptr;             // [2][H][W], the input pixel type
    float *pyr[OFLK_MAX_LEVELS] = {nullptr};   // l < L-1: [2][h_l][w_l]
    float *xy = nullptr;              // [2][K][2]
    unsigned char *vis = nullptr;     // [2][K]
    int *qt = nullptr;                // [K]: birth
    float *qxy = nullptr, *pts = nullptr;   // [K][2] the detection's queries; the points of add_points
    unsigned char *born = nullptr;    // [K]
    float *residual = nullptr;        // [K]
    int *detected = nullptr;          // [1]
    char *feat = nullptr;             // the oflk_replenish_features workspace of one frame
    // the motion row (oflk_tracker_set_motion): off while fit.model < 0; the buffers come with the first push that needs them
    FitConfig fit{-1, 0, 0.0f, 0u};
    long long m_t = -2;              // the frame whose motion row the buffers hold
    float *m_out = nullptr;           // [6]
    unsigned char *m_inlier = nullptr;   // [K]
    int *m_counts = nullptr;          // [3]
    char *m_ws = nullptr;             // the fit's workspace of one step, for m_ws_hyps hypotheses
    int m_ws_hyps = 0;
    size_t m_ws_bytes = 0;

    size_t npix(int l) const { return (size_t)dims[2 * l] * (size_t)dims[2 * l + 1]; }
    size_t pix_bytes() const { return u8 ? 1 : sizeof(float); }
    int K() const { return klt.select.K; }
    float *row_xy(long long f) const { return xy + (size_t)(f & 1) * 2 * (size_t)K(); }
    unsigned char *row_vis(long long f) const { return vis + (size_t)(f & 1) * (size_t)K(); }
    char *frame(long long f) const { return static_cast<char *>(ring) + (size_t)(f & 1) * (size_t)H * W * pix_bytes(); }
};

namespace {
void tracker_free(oflk_tracker *tr)
{
    if (!tr) return;
    if (tr->ready || tr->ws_bytes) (void)hipSetDevice(tr->device);
    for (float *q : tr->pyr)
        if (q) (void)hipFree(q);
    for (void *q : {(void *)tr->ring, (void *)tr->xy, (void *)tr->vis, (void *)tr->qt, (void *)tr->qxy, (void *)tr->pts, (void *)tr->born,
                    (void *)tr->residual, (void *)tr->detected, (void *)tr->feat, (void *)tr->m_out, (void *)tr->m_inlier,
                    (void *)tr->m_counts, (void *)tr->m_ws})
        if (q) (void)hipFree(q);
    delete tr;
}

// the device state, on the first push
int tracker_ensure_state(oflk_tracker *tr)
{
    int rc = ensure_device(tr->device);
    if (rc || tr->ready) return rc;
    if (tr->ws_bytes) return fail(OFLK_ERR_NOMEM, "the tracker's state could not be allocated by an earlier push");
    const size_t plane = (size_t)tr->H * tr->W, row = (size_t)tr->K();
    unsigned char *ring = nullptr;
    if ((rc = dmalloc(&ring, 2 * plane * tr->pix_bytes(), &tr->ws_bytes))) return rc;
    tr->ring = ring;
    for (int l = 0; l < tr->klt.pyr.levels - 1; l++)
        if ((rc = dmalloc(&tr->pyr[l], 2 * tr->npix(l), &tr->ws_bytes))) return rc;
    if ((rc = dmalloc(&tr->xy, 2 * 2 * row, &tr->ws_bytes)) || (rc = dmalloc(&tr->vis, 2 * row, &tr->ws_bytes)) ||
        (rc = dmalloc(&tr->qt, row, &tr->ws_bytes)) || (rc = dmalloc(&tr->qxy, 2 * row, &tr->ws_bytes)) ||
        (rc = dmalloc(&tr->pts, 2 * row, &tr->ws_bytes)) || (rc = dmalloc(&tr->born, row, &tr->ws_bytes)) ||
        (rc = dmalloc(&tr->residual, row, &tr->ws_bytes)) || (rc = dmalloc(&tr->detected, 1, &tr->ws_bytes)) ||
        (rc = dmalloc(&tr->feat, feat_ws(nullptr, 1, tr->H, tr->W, tr->klt.select.md, tr->K()).bytes, &tr->ws_bytes)))
        return rc;
    tr->ready = true;
    return OFLK_OK;
}

// the motion row's buffers, before the first push that fits (and again when the hypotheses outgrow the workspace)
int tracker_ensure_motion(oflk_tracker *tr)
{
    int rc = OFLK_OK;
    if (!tr->m_out && ((rc = dmalloc(&tr->m_out, 6, &tr->ws_bytes)) || (rc = dmalloc(&tr->m_inlier, (size_t)tr->K(), &tr->ws_bytes)) ||
                       (rc = dmalloc(&tr->m_counts, 3, &tr->ws_bytes))))
        return rc;
    if (tr->m_ws_hyps >= tr->fit.hypotheses) return OFLK_OK;
    if (tr->m_ws) {
        HIP_TRY(hipFree(tr->m_ws));   // waits for the work that uses it
        tr->m_ws = nullptr;
        tr->ws_bytes -= tr->m_ws_bytes;
        tr->m_ws_hyps = 0;
    }
    const size_t before = tr->ws_bytes;
    if ((rc = dmalloc(&tr->m_ws, motion_ws(nullptr, 1, tr->K(), tr->fit.hypotheses).bytes, &tr->ws_bytes))) return rc;
    tr->m_ws_bytes = tr->ws_bytes - before;
    tr->m_ws_hyps = tr->fit.hypotheses;
    return OFLK_OK;
}

// the kernel arguments that describe the ring (sparse_pyramids' for a plan)
SparseArgs tracker_args(const oflk_tracker *tr)
{
    SparseArgs a{};
    a.frames = tr->ring;
    a.L = tr->klt.pyr.levels; a.K = tr->klt.pyr.iters; a.B = 1; a.H = tr->H; a.W = tr->W; a.N = tr->K();
    sparse_levels(&a, tr->klt.pyr.levels, tr->pyr, tr->dims);
    a.alpha = tr->klt.test.alpha; a.beta = tr->klt.test.beta; a.max_residual = tr->klt.test.max_residual;
    return a;
}

int tracker_newborn(const oflk_tracker *tr, long long t, const float *qxy, const int *free, const int *nfree, int n, hipStream_t s)
{
    NewbornArgs b{};
    b.row = reinterpret_cast<float2 *>(tr->row_xy(t));
    b.visible = tr->row_vis(t);
    b.born = tr->born; b.qt = tr->qt;
    b.qxy = reinterpret_cast<const float2 *>(qxy);
    b.free = free; b.nfree = nfree;
    b.n = n; b.K = tr->K(); b.t = (int)t;
    const int threads = free ? std::min(n, tr->K()) : tr->K();
    hipLaunchKernelGGL(k_tracker_newborn, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, b);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// One push: the frame (host or device memory) into the free ring slot, that one frame's pyramid into the same slot
// (launch_pyr_down on one image; the previous frame's is kept), the step of every alive slot (k_sparse_push) and, on a
// detection frame, detect_launch on the new row and the rows of the newborn.  All on stream s; nothing is synchronized.
// A push that fails leaves the frame index where it was, but the free ring slot, its pyramid and the other row may have
// been written: the previous row stays readable, and tracker_push refuses further pushes until the tracker is reset.
int tracker_enqueue(oflk_tracker *tr, const void *src, hipMemcpyKind kind, hipStream_t s)
{
    int rc = OFLK_OK;
    const long long t = tr->t + 1;
    const int c = (int)(t & 1);
    const size_t plane = (size_t)tr->H * tr->W;
    char *frame = tr->frame(t);
    HIP_TRY(hipMemcpyAsync(frame, src, plane * tr->pix_bytes(), kind, s));
    PyrExtra first;
    first.u8 = tr->u8;
    // every step is the fused kernel's (oflk_tracker_create), so no temporaries
    if ((rc = pyr_chain(nullptr, tr->gauss, s, reinterpret_cast<const float *>(frame), tr->pyr, (size_t)c, nullptr, nullptr, 1, tr->dims,
                        tr->klt.pyr.levels, first)))
        return rc;
    const SparseArgs a = tracker_args(tr);
    PushArgs r{};
    if (t > 0) {
        r.xy_in = tr->row_xy(t - 1);
        r.vis_in = tr->row_vis(t - 1);
    }
    r.xy_out = tr->row_xy(t); r.vis_out = tr->row_vis(t);
    r.residual = tr->residual; r.born = tr->born; r.detected = tr->detected;
    r.ib = c;
    const int hw = tr->klt.pyr.window_size / 2, K = tr->K();
    const bool built = with_half_window(hw, [&](auto HW) {
        with_pix(tr->u8, [&](auto PIX) {
            hipLaunchKernelGGL((k_sparse_push<decltype(HW)::value, typename decltype(PIX)::type>), dim3((unsigned)K), dim3(64), 0, s, a, r);
        });
    });
    if (!built) return fail(OFLK_ERR_UNSUPPORTED, "half window %d not built", hw);
    HIP_TRY(hipGetLastError());
    const Selection &sel = tr->klt.select;
    if (sel.every > 0 && t % sel.every == 0) {
        const SlotSide slots{tr->row_xy(t), tr->row_vis(t), tr->qt, tr->born, tr->detected, (int)t};
        if ((rc = detect_launch(frame, tr->u8, 1, tr->H, tr->W, tr->klt.pyr.window_size, sel.q, sel.md, K,
                                feat_ws(tr->feat, 1, tr->H, tr->W, sel.md, K), nullptr, tr->qxy, nullptr, &slots, s)) ||
            (rc = tracker_newborn(tr, t, tr->qxy, nullptr, nullptr, 0, s)))
            return rc;
    }
    if (tr->fit.model >= 0) {   // the motion row: step t-1 -> t on the two rows and this frame's born
        if (t == 0) {
            hipLaunchKernelGGL(k_motion_none, dim3((unsigned)((std::max(K, 6) + 255) / 256)), dim3(256), 0, s, tr->m_out, tr->m_inlier,
                               tr->m_counts, K);
            HIP_TRY(hipGetLastError());
        } else if ((rc = motion_launch({tr->row_xy(t - 1), tr->row_xy(t), tr->row_vis(t - 1), tr->row_vis(t), tr->born}, 1, K,
                                       (unsigned)(t - 1), tr->fit.model, tr->fit.hypotheses, tr->fit.threshold, tr->fit.seed,
                                       motion_ws(tr->m_ws, 1, K, tr->fit.hypotheses), tr->m_out, tr->m_inlier, tr->m_counts, s))) {
            return rc;
        }
        tr->m_t = t;
    }
    tr->t = t;   // only a push whose every launch was accepted counts
    return OFLK_OK;
}

int tracker_push(oflk_tracker *tr, const void *src, hipMemcpyKind kind, hipStream_t s)
{
    if (!tr || !src) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (tr->failed) return fail(OFLK_ERR_INVALID, "an earlier push failed part-way: reset the tracker before it is pushed again");
    if (tr->t >= (long long)INT_MAX - 1)
        return fail(OFLK_ERR_UNSUPPORTED, "frame index %lld is the last one a tracker takes (reset it)", tr->t);
    int rc = tracker_ensure_state(tr);   // a refusal here has written nothing
    if (rc || (tr->fit.model >= 0 && (rc = tracker_ensure_motion(tr)))) return rc;
    if ((rc = tracker_enqueue(tr, src, kind, s))) tr->failed = true;
    return rc;
}

// add_points' host side: the points inside [0, W-1] x [0, H-1] (float32 compares, as the kernels'; NaN: outside) in their
// order, at most one per slot
std::vector<float> tracker_filter_points(const oflk_tracker *tr, const float *pts, int n)
{
    std::vector<float> keep;
    const float xmax = (float)(tr->W - 1), ymax = (float)(tr->H - 1);
    for (int i = 0; i < n && keep.size() < 2 * (size_t)tr->K(); i++) {
        const float x = pts[2 * (size_t)i], y = pts[2 * (size_t)i + 1];
        if (x >= 0.0f && x <= xmax && y >= 0.0f && y <= ymax) {
            keep.push_back(x);
            keep.push_back(y);
        }
    }
    return keep;
}

int tracker_pushed(const oflk_tracker *tr)
{
    if (!tr) return fail(OFLK_ERR_INVALID, "NULL tracker");
    if (tr->t < 0) return fail(OFLK_ERR_INVALID, "no frame has been pushed yet");
    return OFLK_OK;
}
// oflk_tracker_create behind its flat list; the online stabiliser's creation makes its tracker here too
int tracker_create(oflk_tracker **out, int device, int H, int W, bool u8, const KltConfig &klt)
{
    if (!out) return fail(OFLK_ERR_INVALID, "tracker pointer is NULL");
    *out = nullptr;
    if (H < 1 || W < 1) return fail(OFLK_ERR_INVALID, "H and W must be >= 1 (got %d x %d)", H, W);
    int rc = check_frame_bounds(H, W);   // oflk_plan_create's, which the sequence call meets there
    if (rc || (rc = check_sparse_test(klt.test)) || (rc = check_sparse_config(H, W, klt.pyr)) || (rc = check_select(klt.select))) return rc;
    if (klt.select.every < 0) return fail(OFLK_ERR_INVALID, "detect_every must be >= 0 (0: never detect; got %d)", klt.select.every);
    if (device < 0 || device >= kMaxDevices) return fail(OFLK_ERR_INVALID, "device %d out of range", device);
    oflk_tracker *tr = new oflk_tracker();
    tr->device = device; tr->H = H; tr->W = W; tr->u8 = u8; tr->klt = klt;
    // At the pyramid's scale of 0.5 every step fits the fused kernel: a finer size is 2m or 2m + 1 for the coarser m, so a 32 x
    // 16 coarse tile spans at most 66 x 34 source elements.  The tracker therefore holds neither the unfused chain's
    // temporaries nor a float32 stage for uint8 frames, and pyr_chain_fits cannot refuse at that scale; it is here so that
    // pyr_chain is never handed NULL temporaries it would use
    if ((rc = level_dims(H, W, klt.pyr.levels, 0.5, tr->dims)) || (rc = make_gauss(2.0, &tr->gauss)) ||
        (rc = pyr_chain_fits(tr->dims, klt.pyr.levels, tr->gauss))) {
        delete tr;
        return rc;
    }
    *out = tr;
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_tracker_create(oflk_tracker **out, int device, int H, int W, int u8, int levels, int window_size, int iters,
                                 float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                 int max_corners, int detect_every)
{
    return tracker_create(out, device, H, W, u8 != 0,
                          {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}});
}

OFLK_API int oflk_tracker_destroy(oflk_tracker *tr)
{
    tracker_free(tr);
    return OFLK_OK;
}

OFLK_API int oflk_tracker_reset(oflk_tracker *tr, void *)
{
    if (!tr) return fail(OFLK_ERR_INVALID, "NULL tracker");
    tr->t = -1;   // frame 0's push reads no row: every slot is dead
    tr->m_t = -2;
    tr->failed = false;
    return OFLK_OK;
}

OFLK_API size_t oflk_tracker_workspace_bytes(const oflk_tracker *tr) { return tr ? tr->ws_bytes : 0; }

OFLK_API int oflk_tracker_frame_index(const oflk_tracker *tr) { return tr ? (int)tr->t : -1; }

OFLK_API int oflk_tracker_push_device(oflk_tracker *tr, const void *d_frame, void *stream)
{
    return tracker_push(tr, d_frame, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

OFLK_API int oflk_tracker_row_device(const oflk_tracker *tr, const float **d_xy, const unsigned char **d_visible,
                                     const unsigned char **d_born, const int **d_birth, const float **d_residual,
                                     const int **d_detected)
{
    if (int rc = tracker_pushed(tr)) return rc;
    if (d_xy) *d_xy = tr->row_xy(tr->t);
    if (d_visible) *d_visible = tr->row_vis(tr->t);
    if (d_born) *d_born = tr->born;
    if (d_birth) *d_birth = tr->qt;
    if (d_residual) *d_residual = tr->residual;
    if (d_detected) *d_detected = tr->detected;
    return OFLK_OK;
}

OFLK_API int oflk_tracker_read_row(oflk_tracker *tr, float *xy, unsigned char *visible, unsigned char *born, int *birth,
                                   float *residual, int *detected, void *stream)
{
    if (int rc = tracker_pushed(tr)) return rc;
    HIP_TRY(hipSetDevice(tr->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t row = (size_t)tr->K();
    if (xy) HIP_TRY(hipMemcpyAsync(xy, tr->row_xy(tr->t), 2 * row * sizeof(float), hipMemcpyDeviceToHost, s));
    if (visible) HIP_TRY(hipMemcpyAsync(visible, tr->row_vis(tr->t), row, hipMemcpyDeviceToHost, s));
    if (born) HIP_TRY(hipMemcpyAsync(born, tr->born, row, hipMemcpyDeviceToHost, s));
    if (birth) HIP_TRY(hipMemcpyAsync(birth, tr->qt, row * sizeof(int), hipMemcpyDeviceToHost, s));
    if (residual) HIP_TRY(hipMemcpyAsync(residual, tr->residual, row * sizeof(float), hipMemcpyDeviceToHost, s));
    if (detected) HIP_TRY(hipMemcpyAsync(detected, tr->detected, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return OFLK_OK;
}

OFLK_API int oflk_tracker_push(oflk_tracker *tr, const void *frame, float *xy, unsigned char *visible, unsigned char *born,
                               int *birth, float *residual, int *detected)
{
    int rc = tracker_push(tr, frame, hipMemcpyHostToDevice, nullptr);
    if (rc) {
        if (tr && tr->ready) (void)hipStreamSynchronize(nullptr);   // a copy from the caller's frame may be queued
        return rc;
    }
    return oflk_tracker_read_row(tr, xy, visible, born, birth, residual, detected, nullptr);
}

OFLK_API int oflk_tracker_add_points(oflk_tracker *tr, const float *pts, int n, void *stream)
{
    if (int rc = tracker_pushed(tr)) return rc;
    if (!pts) return fail(OFLK_ERR_INVALID, "NULL points");
    if (n < 1) return fail(OFLK_ERR_INVALID, "n must be >= 1 (got %d)", n);
    const std::vector<float> keep = tracker_filter_points(tr, pts, n);
    if (keep.empty()) return OFLK_OK;
    HIP_TRY(hipSetDevice(tr->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(tr->pts, keep.data(), keep.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // `keep` is this call's
    const FeatWs ws = feat_ws(tr->feat, 1, tr->H, tr->W, tr->klt.select.md, tr->K());
    hipLaunchKernelGGL(k_free_list, dim3(1), dim3(256), 0, s, (const unsigned char *)tr->row_vis(tr->t), tr->K(), ws.free, ws.nfree);
    HIP_TRY(hipGetLastError());
    return tracker_newborn(tr, tr->t, tr->pts, ws.free, ws.nfree, (int)(keep.size() / 2), s);
}

OFLK_API int oflk_tracker_set_motion(oflk_tracker *tr, int model, int hypotheses, float threshold, unsigned seed)
{
    if (!tr) return fail(OFLK_ERR_INVALID, "NULL tracker");
    if (model == -1) {
        tr->fit.model = -1;
        return OFLK_OK;
    }
    const FitConfig fit{model, hypotheses, threshold, seed};
    if (int rc = check_motion(fit)) return rc;
    tr->fit = fit;
    return OFLK_OK;
}

namespace {
int tracker_has_motion(const oflk_tracker *tr)
{
    if (int rc = tracker_pushed(tr)) return rc;
    if (tr->m_t != tr->t) return fail(OFLK_ERR_INVALID, "the last push had no motion model set (oflk_tracker_set_motion)");
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_tracker_motion_device(const oflk_tracker *tr, const float **d_model, const unsigned char **d_inlier,
                                        const int **d_counts)
{
    if (int rc = tracker_has_motion(tr)) return rc;
    if (d_model) *d_model = tr->m_out;
    if (d_inlier) *d_inlier = tr->m_inlier;
    if (d_counts) *d_counts = tr->m_counts;
    return OFLK_OK;
}

OFLK_API int oflk_tracker_read_motion(oflk_tracker *tr, float *model, unsigned char *inlier, int *counts, void *stream)
{
    if (int rc = tracker_has_motion(tr)) return rc;
    HIP_TRY(hipSetDevice(tr->device));
    hipStream_t s = (hipStream_t)stream;
    if (model) HIP_TRY(hipMemcpyAsync(model, tr->m_out, 6 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (inlier) HIP_TRY(hipMemcpyAsync(inlier, tr->m_inlier, (size_t)tr->K(), hipMemcpyDeviceToHost, s));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, tr->m_counts, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return OFLK_OK;
}

// =============================================================================
// online video stabilisation: a fixed-lag stabiliser on the tracker
// =============================================================================
// The state of a stabiliser: a tracker with its motion row on, and what the trajectory's window needs of the past -- the
// last r + 1 frames (frame t in delay slot t % (r + 1)) and the last cap = max(2 r, 1) step models (step s in ring slot
// s % cap).  The fit of the push of frame t writes step t-1 straight into its ring slot: the tracker's motion-row pointers
// are aimed there before the push (frame 0's failure row goes to the tracker's own buffers), so the inner tracker's
// motion_device / read_motion show the step as on a plain tracker.  Creation makes no device call; the first push
// allocates everything but the one-frame staging of the host forms, which comes with their first call.
struct oflk_stabilizer {
    oflk_tracker *tr = nullptr;
    int r = 0, cap = 1;
    StabWeights wt{};
    long long t = -1;                 // index of the last pushed frame
    bool ready = false;               // the device state exists
    bool failed = false;              // a push or flush failed part-way: refused until reset
    bool flushed = false;             // the stream has ended: pushes are refused until reset
    int rows = 0;                     // rows of corr / map the last emission wrote
    size_t ws_bytes = 0;
    char *delay = nullptr;            // [r + 1] frames of the layout
    float *ring_model = nullptr;      // [cap][6]
    int *ring_counts = nullptr;       // [cap][3]
    float *corr = nullptr;            // [max(r, 1)][6]
    double *map = nullptr;            // [max(r, 1)][6]
    float *own_model = nullptr;       // the tracker's own motion row, put back before it is freed
    int *own_counts = nullptr;
    char *stage_out = nullptr;        // a frame of the layout and [H][W] bytes: the host forms' staging
    unsigned char *stage_inside = nullptr;
    // The delay line and every frame in and out are the layout's.  Planar: the tracker is pushed the frame.  Packed: the
    // tracker (uint8) is pushed the luma of the frame, formed in `luma` by the push.  NV12: the tracker (uint8) is pushed the
    // frame's own first H W bytes, its Y plane: no luma launch and no luma plane
    FrameLayout layout = FrameLayout::planar(false);
    unsigned char *luma = nullptr;    // [H][W], packed only

    size_t plane_bytes() const { return layout.frame_bytes(tr->H, tr->W); }
    char *slot(long long f) const { return delay + (size_t)(f % (r + 1)) * plane_bytes(); }
};

namespace {
int check_trajectory_ring(const void *model, int cap, int f0, int n, int T, const double *weights, int radius, const void *correction,
                          const void *map)
{
    if (int rc = check_stab_window(weights, radius)) return rc;
    if (cap < std::max(2 * radius, 1))
        return fail(OFLK_ERR_INVALID, "cap must be >= max(2 radius, 1) = %d (got %d)", std::max(2 * radius, 1), cap);
    if (n < 1 || n > kStabOnlineBlock) return fail(OFLK_ERR_INVALID, "n must be in [1, %d] (got %d)", kStabOnlineBlock, n);
    if (f0 < 0) return fail(OFLK_ERR_INVALID, "f0 must be >= 0 (got %d)", f0);
    if (T < -1) return fail(OFLK_ERR_INVALID, "T must be >= 0, or -1 while the stream is open (got %d)", T);
    if (T >= 0 && (long long)f0 + n > (long long)T)
        return fail(OFLK_ERR_INVALID, "frames %d .. %lld of a stream of %d", f0, (long long)f0 + n - 1, T);
    if (T < 0 && n != 1) return fail(OFLK_ERR_INVALID, "an open stream has one final frame at a time (n = %d)", n);
    if (!model || !correction || !map) return fail(OFLK_ERR_INVALID, "NULL input or output argument");
    if (!aligned(map, 8)) return fail(OFLK_ERR_INVALID, "d_map must be 8-byte aligned");
    return OFLK_OK;
}

// the one launch of k_stab_online on stream s; the arguments are checked
int trajectory_ring_launch(const float *d_model, const int *d_counts, int cap, int f0, int n, int T, const StabWeights &wt, int radius,
                           float *d_correction, double *d_map, hipStream_t s)
{
    hipLaunchKernelGGL(k_stab_online, dim3((unsigned)n), dim3(kStabOnlineBlock), 0, s, d_model, d_counts, cap, f0, T, radius, wt,
                       d_correction, d_map);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

// the device state, on the first push
int stabilizer_ensure_state(oflk_stabilizer *st)
{
    oflk_tracker *tr = st->tr;
    int rc = tracker_ensure_state(tr);
    if (rc || st->ready) return rc;
    if (st->ws_bytes) return fail(OFLK_ERR_NOMEM, "the stabiliser's state could not be allocated by an earlier push");
    if ((rc = tracker_ensure_motion(tr))) return rc;
    const size_t rows = (size_t)std::max(st->r, 1);
    if ((rc = dmalloc(&st->delay, (size_t)(st->r + 1) * st->plane_bytes(), &st->ws_bytes)) ||
        (rc = dmalloc(&st->ring_model, 6 * (size_t)st->cap, &st->ws_bytes)) ||
        (rc = dmalloc(&st->ring_counts, 3 * (size_t)st->cap, &st->ws_bytes)) || (rc = dmalloc(&st->corr, 6 * rows, &st->ws_bytes)) ||
        (rc = dmalloc(&st->map, 6 * rows, &st->ws_bytes)) ||
        (st->layout.kind == FrameKind::Packed && (rc = dmalloc(&st->luma, (size_t)tr->H * tr->W, &st->ws_bytes))))
        return rc;
    st->own_model = tr->m_out;
    st->own_counts = tr->m_counts;
    st->ready = true;
    return OFLK_OK;
}

// the staging of the host forms, on their first call
int stabilizer_ensure_stage(oflk_stabilizer *st)
{
    if (st->stage_out) return OFLK_OK;
    int rc = dmalloc(&st->stage_out, st->plane_bytes(), &st->ws_bytes);
    if (!rc) rc = dmalloc(&st->stage_inside, (size_t)st->tr->H * st->tr->W, &st->ws_bytes);
    return rc;
}

// what every push and flush is refused for
int stabilizer_open(const oflk_stabilizer *st, const char *what)
{
    if (st->flushed) return fail(OFLK_ERR_INVALID, "the stabiliser has been flushed: reset it before %s", what);
    if (st->failed) return fail(OFLK_ERR_INVALID, "an earlier push or flush failed part-way: reset the stabiliser before %s", what);
    return OFLK_OK;
}

// One push on stream s: the frame (host or device memory) into its delay slot, the tracker's push of that slot with the fit
// aimed at the step's ring slot, and for t >= r the trajectory of frame t - r and its warp into d_out.  Nothing is
// synchronised.  The frame index moves only when every launch was accepted.
int stabilizer_enqueue(oflk_stabilizer *st, const void *src, hipMemcpyKind kind, void *d_out, unsigned char *d_inside, hipStream_t s)
{
    oflk_tracker *tr = st->tr;
    const long long t = st->t + 1;
    char *frame = st->slot(t);
    HIP_TRY(hipMemcpyAsync(frame, src, st->plane_bytes(), kind, s));
    const size_t k = t >= 1 ? (size_t)((t - 1) % st->cap) : 0;
    tr->m_out = t >= 1 ? st->ring_model + 6 * k : st->own_model;
    tr->m_counts = t >= 1 ? st->ring_counts + 3 * k : st->own_counts;
    // what the tracker is pushed: the frame, the packed frame's luma, or the NV12 frame's leading Y plane
    const FrameLayout &L = st->layout;
    const void *grey = frame;
    int rc = OFLK_OK;
    if (L.kind == FrameKind::Packed) {
        if ((rc = luma_launch((const unsigned char *)frame, 1, tr->H, tr->W, L.channels, L.order, st->luma, s))) return rc;
        grey = st->luma;
    }
    if ((rc = tracker_push(tr, grey, hipMemcpyDeviceToDevice, s))) return rc;
    if (t >= st->r) {
        const long long e = t - st->r;
        if ((rc = trajectory_ring_launch(st->ring_model, st->ring_counts, st->cap, (int)e, 1, -1, st->wt, st->r, st->corr, st->map, s)) ||
            (rc = warp_launch(L, false, st->slot(e), 1, tr->H, tr->W, st->map, d_out, d_inside, s)))
            return rc;
        st->rows = 1;
    }
    st->t = t;
    return OFLK_OK;
}

int stabilizer_push(oflk_stabilizer *st, const void *src, hipMemcpyKind kind, void *d_out, unsigned char *d_inside, int *emitted,
                    hipStream_t s)
{
    if (emitted) *emitted = -1;
    if (!st || !src || !d_out || !emitted) return fail(OFLK_ERR_INVALID, "NULL argument");
    int rc = stabilizer_open(st, "it is pushed again");
    if (rc || (rc = stabilizer_ensure_state(st))) return rc;   // a refusal here has written nothing
    if ((rc = stabilizer_enqueue(st, src, kind, d_out, d_inside, s))) {
        st->failed = true;
        return rc;
    }
    if (st->t >= st->r) *emitted = (int)(st->t - st->r);
    return OFLK_OK;
}

// A flush up to the trajectory: the refusals, the frames that are left (first, n) and their rows of corr / map on stream s
int stabilizer_flush_begin(oflk_stabilizer *st, const void *out, int *first, int *count, hipStream_t s)
{
    if (first) *first = 0;
    if (count) *count = 0;
    if (!st || !first || !count) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (st->failed) return fail(OFLK_ERR_INVALID, "an earlier push or flush failed part-way: reset the stabiliser");
    const long long T = st->t + 1;
    const int n = st->flushed ? 0 : (int)std::min<long long>(st->r, T);
    *first = (int)(T - n);
    if (n == 0) {
        st->flushed = true;
        return OFLK_OK;
    }
    if (!out) return fail(OFLK_ERR_INVALID, "NULL output for the %d frames that are left", n);
    HIP_TRY(hipSetDevice(st->tr->device));
    st->flushed = true;
    if (int rc = trajectory_ring_launch(st->ring_model, st->ring_counts, st->cap, *first, n, (int)T, st->wt, st->r, st->corr, st->map, s)) {
        st->failed = true;
        return rc;
    }
    st->rows = n;
    *count = n;
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_stabilize_trajectory_ring(const float *d_model_ring, const int *d_counts_ring, int cap, int f0, int n, int T,
                                            const double *weights, int radius, float *d_correction, double *d_map, void *stream)
{
    if (int rc = check_trajectory_ring(d_model_ring, cap, f0, n, T, weights, radius, d_correction, d_map)) return rc;
    StabWeights wt{};
    for (int i = 0; i <= radius; i++) wt.w[i] = weights[i];
    return trajectory_ring_launch(d_model_ring, d_counts_ring, cap, f0, n, T, wt, radius, d_correction, d_map, (hipStream_t)stream);
}

namespace {
// the creation of every layout: the layout's own refusals, the shape, the byte count of a packed frame, then the tracker's
int stabilizer_create(oflk_stabilizer **out, int device, int H, int W, const FrameLayout &L, const KltConfig &klt, const FitConfig &fit,
                      const TrajWindow &window)
{
    if (!out) return fail(OFLK_ERR_INVALID, "stabiliser pointer is NULL");
    *out = nullptr;
    int rc = check_layout(L, H, W);
    if (rc) return rc;
    if (H < 2 || W < 2) return fail(OFLK_ERR_INVALID, "H and W must be >= 2 (got %d x %d)", H, W);
    if (L.kind == FrameKind::Packed && L.frame_bytes(H, W) >= ((size_t)1 << 31))
        return fail(OFLK_ERR_UNSUPPORTED, "packed frames of 2^31 bytes or more are not supported");
    if ((rc = check_motion(fit)) || (rc = check_stab_window(window))) return rc;
    oflk_tracker *tr = nullptr;
    if ((rc = tracker_create(&tr, device, H, W, L.pix_bytes == 1, klt))) return rc;
    tr->fit = fit;   // checked above, as oflk_tracker_set_motion would
    oflk_stabilizer *st = new oflk_stabilizer();
    st->tr = tr;
    st->layout = L;
    st->r = window.radius;
    st->cap = std::max(2 * window.radius, 1);
    for (int i = 0; i <= window.radius; i++) st->wt.w[i] = window.weights[i];
    *out = st;
    return OFLK_OK;
}
}  // namespace

OFLK_API int oflk_stabilizer_create(oflk_stabilizer **out, int device, int H, int W, int u8, int levels, int window_size, int iters,
                                    float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                    int max_corners, int detect_every, int model, int hypotheses, float threshold, unsigned seed,
                                    const double *weights, int radius)
{
    return stabilizer_create(out, device, H, W, FrameLayout::planar(u8 != 0),
                             {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                             {model, hypotheses, threshold, seed}, {weights, radius});
}

OFLK_API int oflk_stabilizer_create_packed(oflk_stabilizer **out, int device, int H, int W, int channels, int order, int levels,
                                           int window_size, int iters, float alpha, float beta, float max_residual,
                                           float quality_level, float min_distance, int max_corners, int detect_every, int model,
                                           int hypotheses, float threshold, unsigned seed, const double *weights, int radius)
{
    return stabilizer_create(out, device, H, W, FrameLayout::packed(channels, order),
                             {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                             {model, hypotheses, threshold, seed}, {weights, radius});
}

OFLK_API int oflk_stabilizer_create_nv12(oflk_stabilizer **out, int device, int H, int W, int siting, int levels, int window_size,
                                         int iters, float alpha, float beta, float max_residual, float quality_level,
                                         float min_distance, int max_corners, int detect_every, int model, int hypotheses,
                                         float threshold, unsigned seed, const double *weights, int radius)
{
    return stabilizer_create(out, device, H, W, FrameLayout::nv12(siting),
                             {{levels, window_size, iters}, {alpha, beta, max_residual}, {quality_level, min_distance, max_corners, detect_every}},
                             {model, hypotheses, threshold, seed}, {weights, radius});
}

OFLK_API int oflk_stabilizer_destroy(oflk_stabilizer *st)
{
    if (!st) return OFLK_OK;
    if (st->ready) {   // the tracker frees its own motion row
        st->tr->m_out = st->own_model;
        st->tr->m_counts = st->own_counts;
    }
    if (st->ws_bytes) (void)hipSetDevice(st->tr->device);
    for (void *q : {(void *)st->delay, (void *)st->ring_model, (void *)st->ring_counts, (void *)st->corr, (void *)st->map,
                    (void *)st->stage_out, (void *)st->stage_inside, (void *)st->luma})
        if (q) (void)hipFree(q);
    tracker_free(st->tr);
    delete st;
    return OFLK_OK;
}

OFLK_API int oflk_stabilizer_reset(oflk_stabilizer *st, void *stream)
{
    if (!st) return fail(OFLK_ERR_INVALID, "NULL stabiliser");
    st->t = -1;
    st->rows = 0;
    st->failed = st->flushed = false;
    return oflk_tracker_reset(st->tr, stream);
}

OFLK_API size_t oflk_stabilizer_workspace_bytes(const oflk_stabilizer *st) { return st ? st->ws_bytes + st->tr->ws_bytes : 0; }

OFLK_API int oflk_stabilizer_lag(const oflk_stabilizer *st) { return st ? st->r : -1; }

OFLK_API int oflk_stabilizer_frame_index(const oflk_stabilizer *st) { return st ? (int)st->t : -1; }

OFLK_API oflk_tracker *oflk_stabilizer_tracker(oflk_stabilizer *st) { return st ? st->tr : nullptr; }

OFLK_API int oflk_stabilizer_push_device(oflk_stabilizer *st, const void *d_frame, void *d_out, unsigned char *d_inside, int *emitted,
                                         void *stream)
{
    if (st && !st->tr->u8 && (!aligned(d_frame, 4) || !aligned(d_out, 4))) {
        if (emitted) *emitted = -1;
        return fail(OFLK_ERR_INVALID, "float32 frames must be 4-byte aligned");
    }
    return stabilizer_push(st, d_frame, hipMemcpyDeviceToDevice, d_out, d_inside, emitted, (hipStream_t)stream);
}

OFLK_API int oflk_stabilizer_correction_device(const oflk_stabilizer *st, const float **d_correction, const double **d_map)
{
    if (!st) return fail(OFLK_ERR_INVALID, "NULL stabiliser");
    if (st->rows < 1) return fail(OFLK_ERR_INVALID, "no frame has been emitted yet");
    if (d_correction) *d_correction = st->corr;
    if (d_map) *d_map = st->map;
    return OFLK_OK;
}

OFLK_API int oflk_stabilizer_push(oflk_stabilizer *st, const void *frame, void *out, unsigned char *inside, float *correction,
                                  int *emitted)
{
    if (emitted) *emitted = -1;
    if (!st || !frame || !out || !emitted) return fail(OFLK_ERR_INVALID, "NULL argument");
    int rc = stabilizer_open(st, "it is pushed again");
    if (rc || (rc = stabilizer_ensure_state(st)) || (rc = stabilizer_ensure_stage(st))) return rc;
    if ((rc = stabilizer_push(st, frame, hipMemcpyHostToDevice, st->stage_out, inside ? st->stage_inside : nullptr, emitted, nullptr))) {
        if (st->ready) (void)hipStreamSynchronize(nullptr);   // a copy from the caller's frame may be queued
        return rc;
    }
    if (*emitted >= 0) {
        HIP_TRY(hipMemcpyAsync(out, st->stage_out, st->plane_bytes(), hipMemcpyDeviceToHost, nullptr));
        if (inside) HIP_TRY(hipMemcpyAsync(inside, st->stage_inside, (size_t)st->tr->H * st->tr->W, hipMemcpyDeviceToHost, nullptr));
        if (correction) HIP_TRY(hipMemcpyAsync(correction, st->corr, 6 * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return OFLK_OK;
}

OFLK_API int oflk_stabilizer_flush_device(oflk_stabilizer *st, void *d_out, unsigned char *d_inside, int *first, int *count, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    int rc = stabilizer_flush_begin(st, d_out, first, count, s);
    if (rc || *count == 0) return rc;
    // frames first .. first + n - 1 lie in consecutive delay slots that wrap at most once: two launches at the most
    const int n = *count, slots = st->r + 1, s0 = *first % slots, n0 = std::min(n, slots - s0);
    const int H = st->tr->H, W = st->tr->W;
    const size_t pb = st->plane_bytes(), plane = st->layout.inside_bytes(H, W);
    if ((rc = warp_launch(st->layout, false, st->delay + (size_t)s0 * pb, n0, H, W, st->map, d_out, d_inside, s)) ||
        (n > n0 && (rc = warp_launch(st->layout, false, st->delay, n - n0, H, W, st->map + 6 * (size_t)n0,
                                     static_cast<char *>(d_out) + (size_t)n0 * pb, d_inside ? d_inside + (size_t)n0 * plane : nullptr,
                                     s)))) {
        st->failed = true;
        *count = 0;
    }
    return rc;
}

OFLK_API int oflk_stabilizer_flush(oflk_stabilizer *st, void *out, unsigned char *inside, float *correction, int *first, int *count)
{
    int rc = stabilizer_flush_begin(st, out, first, count, nullptr);
    if (rc || *count == 0) return rc;
    const int n = *count;
    *count = 0;
    if ((rc = stabilizer_ensure_stage(st))) {
        st->failed = true;
        return rc;
    }
    // frame by frame through the one staged frame; the null stream orders a frame's copies ahead of the next warp
    const size_t pb = st->plane_bytes(), plane = (size_t)st->tr->H * st->tr->W;
    for (int i = 0; i < n; i++) {
        if ((rc = warp_launch(st->layout, false, st->slot((long long)*first + i), 1, st->tr->H, st->tr->W, st->map + 6 * (size_t)i,
                              st->stage_out, inside ? st->stage_inside : nullptr, nullptr))) {
            st->failed = true;
            (void)hipStreamSynchronize(nullptr);
            return rc;
        }
        HIP_TRY(hipMemcpyAsync(static_cast<char *>(out) + (size_t)i * pb, st->stage_out, pb, hipMemcpyDeviceToHost, nullptr));
        if (inside) HIP_TRY(hipMemcpyAsync(inside + (size_t)i * plane, st->stage_inside, plane, hipMemcpyDeviceToHost, nullptr));
    }
    if (correction) HIP_TRY(hipMemcpyAsync(correction, st->corr, 6 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    *count = n;
    return OFLK_OK;
}

OFLK_API int oflk_pyramidal_last_level_flow(int B, int H, int W, int levels, int window_size, int iters, int level,
                                            int pair, float *u, float *v)
{
    HostCall call;
    int rc = call.begin();
    if (rc) return rc;
    oflk_plan *p = nullptr;
    if ((rc = cached_plan(*call.c, B, H, W, levels, window_size, iters, &p))) return rc;
    return oflk_plan_read_level_flow(p, level, pair, u, v, nullptr);
}

OFLK_API int oflk_pyramidal_last_uncertain(int B, int H, int W, int levels, int window_size, int iters, int *uncertain)
{
    HostCall call;
    int rc = call.begin();
    if (rc) return rc;
    oflk_plan *p = nullptr;
    if ((rc = cached_plan(*call.c, B, H, W, levels, window_size, iters, &p))) return rc;
    return oflk_plan_read_uncertain(p, uncertain, nullptr);
}

OFLK_API void oflk_shard_range(int total, int shard, int n_shards, int *begin, int *end)
{
    int b = 0, e = 0;
    if (n_shards >= 1 && shard >= 0 && shard < n_shards && total >= 0) shard_range(total, shard, n_shards, &b, &e);
    if (begin) *begin = b;
    if (end) *end = e;
}

namespace {

// device flows -> metrics; `dev_true` holds u_true[B] then v_true[B]
int metrics_device(const float *d_u, const float *d_v, int B, int H, int W, const float *u_true, const float *v_true,
                   int y0, int y1, int x0, int x1, double *out, hipStream_t s)
{
    if (!d_u || !d_v || !u_true || !v_true || !out) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (B < 1 || H < 1 || W < 1) return fail(OFLK_ERR_INVALID, "B, H and W must be >= 1");
    // NumPy slice semantics for mask[y0:y1, x0:x1]: negative bounds count from the end, then clip
    auto norm = [](int i, int n) { return std::min(std::max(i < 0 ? i + n : i, 0), n); };
    y0 = norm(y0, H); y1 = norm(y1, H); x0 = norm(x0, W); x1 = norm(x1, W);
    const size_t count = (size_t)std::max(y1 - y0, 0) * (size_t)std::max(x1 - x0, 0);
    Arena ar;
    float *d_true = nullptr;
    double *d_part = nullptr;
    int rc = ar.get(&d_true, (size_t)2 * B);
    if (!rc) rc = ar.get(&d_part, (size_t)B * kMetricBlocks * kMetricTerms);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_true, u_true, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_true + B, v_true, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    MetricArgs a{};
    a.u = d_u; a.v = d_v;
    a.u_true = d_true; a.v_true = d_true + B;
    a.B = B; a.H = H; a.W = W;
    a.y0 = y0; a.y1 = y1; a.x0 = x0; a.x1 = x1;
    a.partial = d_part;
    // gridDim.y stops at 65 535: beyond it a block walks several pairs, each pair's partials laid out as before
    hipLaunchKernelGGL(k_flow_metrics, dim3(kMetricBlocks, (unsigned)std::min(B, kMetricMaxGridY)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    std::vector<double> part((size_t)B * kMetricBlocks * kMetricTerms);
    HIP_TRY(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        double t[kMetricTerms] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < kMetricBlocks; k++) {
            const double *q = &part[((size_t)b * kMetricBlocks + k) * kMetricTerms];
            for (int i = 0; i < kMetricTerms; i++) t[i] += q[i];
        }
        double *o = out + (size_t)b * 5;
        const double n = (double)count;   // an empty mask gives nan, as np.mean of an empty array does
        o[0] = (double)(float)(t[0] / n);
        o[1] = (double)(float)(t[1] / n);
        o[2] = (double)std::sqrt((float)(t[2] / n));   // np.sqrt of the fp32 mean (:69)
        o[3] = (double)(float)(t[3] / n);
        // "nothing moves and nothing was predicted" (:143-146): t[5] counts the region's pixels that are not below 1e-6,
        // NaN ones included; an empty region has none
        const double mt = std::sqrt((double)u_true[b] * u_true[b] + (double)v_true[b] * v_true[b]);
        o[4] = (mt < 1e-6 && t[5] == 0.0) ? 0.0 : (double)(float)(t[4] / n);
    }
    return OFLK_OK;
}

}  // namespace

OFLK_API int oflk_plan_metrics(oflk_plan *p, const float *d_u, const float *d_v, const float *u_true,
                               const float *v_true, int y0, int y1, int x0, int x1, double *out, void *stream)
{
    if (!p) return fail(OFLK_ERR_INVALID, "NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    return metrics_device(d_u, d_v, p->B, p->H, p->W, u_true, v_true, y0, y1, x0, x1, out, (hipStream_t)stream);
}

OFLK_API int oflk_flow_metrics(const float *u, const float *v, int B, int H, int W, const float *u_true,
                               const float *v_true, int y0, int y1, int x0, int x1, double *out)
{
    int rc = check_hw(u, v, H, W);
    if (rc) return rc;
    if (B < 1) return fail(OFLK_ERR_INVALID, "B must be >= 1");
    if (!u_true || !v_true || !out) return fail(OFLK_ERR_INVALID, "NULL argument");   // before anything is uploaded
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)B * H * W;
    float *d_u, *d_v;
    if ((rc = call.upload(&d_u, u, n)) || (rc = call.upload(&d_v, v, n))) return rc;
    return metrics_device(d_u, d_v, B, H, W, u_true, v_true, y0, y1, x0, x1, out, nullptr);
}

OFLK_API int oflk_u8_to_f32(const unsigned char *d_in, float *d_out, size_t n, void *stream)
{
    if (!d_in || !d_out) return fail(OFLK_ERR_INVALID, "NULL argument");
    if (n == 0) return OFLK_OK;
    dim3 grid((unsigned)((n + 4095) / 4096));
    hipLaunchKernelGGL(k_u8_to_f32, grid, dim3(256), 0, (hipStream_t)stream, d_in, d_out, n);
    HIP_TRY(hipGetLastError());
    return OFLK_OK;
}

OFLK_API int oflk_compute_gradients(const float *prev, const float *curr, int H, int W, float *Ix,
                                    float *Iy, float *It)
{
    int rc = check_hw(prev, curr, H, W);
    if (rc) return rc;
    if (!Ix || !Iy || !It) return fail(OFLK_ERR_INVALID, "NULL output");
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)H * W;
    float *d[5];
    if ((rc = call.upload(&d[0], prev, n)) || (rc = call.upload(&d[1], curr, n)) || (rc = call.alloc(&d[2], n)) ||
        (rc = call.alloc(&d[3], n)) || (rc = call.alloc(&d[4], n)))
        return rc;
    hipLaunchKernelGGL(k_gradients, grid2d(W, H, 1), dim3(256), 0, nullptr, (const float *)d[0],
                       (const float *)d[1], d[2], d[3], d[4], H, W);
    HIP_TRY(hipGetLastError());
    if ((rc = call.to_host(Ix, d[2], n)) || (rc = call.to_host(Iy, d[3], n)) || (rc = call.to_host(It, d[4], n))) return rc;
    return call.sync();
}

OFLK_API int oflk_from_gradients(const float *Ix, const float *Iy, const float *It, int H, int W,
                                 int window_size, float *u, float *v)
{
    int rc = check_hw(Ix, Iy, H, W);
    if (rc) return rc;
    if (!It || !u || !v) return fail(OFLK_ERR_INVALID, "NULL argument");
    int hw = 0;
    if ((rc = window_hw(window_size, &hw))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)H * W;
    float *d[5];
    if ((rc = call.upload(&d[0], Ix, n)) || (rc = call.upload(&d[1], Iy, n)) || (rc = call.upload(&d[2], It, n)) ||
        (rc = call.alloc(&d[3], n)) || (rc = call.alloc(&d[4], n)))
        return rc;
    LkArgs a{};
    a.prev = d[0]; a.curr = d[1]; a.aux = d[2];
    a.ou = d[3]; a.ov = d[4];
    a.H = H; a.W = W;
    rc = launch_lk<MODE_GRADS>(nullptr, nullptr, KC_LK_SINGLE, hw, a, 1);
    if (rc) return rc;
    if ((rc = call.to_host(u, d[3], n)) || (rc = call.to_host(v, d[4], n))) return rc;
    return call.sync();
}

namespace {
int build_pyramid_host(const float *image, int H, int W, int levels, double scale_factor, const GaussW *given, float *const *out_levels);
}

OFLK_API int oflk_build_pyramid(const float *image, int H, int W, int levels, double scale_factor,
                                float *const *out_levels)
{
    return build_pyramid_host(image, H, W, levels, scale_factor, nullptr, out_levels);
}

OFLK_API int oflk_build_pyramid_w(const float *image, int H, int W, int levels, double scale_factor, const double *weights,
                                  int radius, float *const *out_levels)
{
    if (!weights) return fail(OFLK_ERR_INVALID, "NULL weights");
    if (radius < 0 || radius > kMaxRadius) return fail(OFLK_ERR_UNSUPPORTED, "gaussian radius %d outside [0, %d]", radius, kMaxRadius);
    GaussW g;
    g.radius = radius;
    for (int k = 0; k <= radius; k++) g.w[k] = weights[k];
    return build_pyramid_host(image, H, W, levels, scale_factor, &g, out_levels);
}

namespace {
int build_pyramid_host(const float *image, int H, int W, int levels, double scale_factor, const GaussW *given, float *const *out_levels)
{
    int rc = check_hw(image, out_levels, H, W);
    if (rc) return rc;
    int dims[2 * OFLK_MAX_LEVELS];
    if ((rc = level_dims(H, W, levels, scale_factor, dims))) return rc;
    for (int l = 0; l < levels; l++)
        if (!out_levels[l]) return fail(OFLK_ERR_INVALID, "out_levels[%d] is NULL", l);
    HostCall call;
    if ((rc = call.begin())) return rc;
    GaussW gauss;
    if (given) gauss = *given;
    else if ((rc = make_gauss(1.0 / scale_factor, &gauss))) return rc;
    const size_t N = (size_t)H * W;
    float *cur, *nxt, *tA, *tB;
    if ((rc = call.upload(&cur, image, N)) || (rc = call.alloc(&nxt, N)) || (rc = call.alloc(&tA, N)) || (rc = call.alloc(&tB, N)))
        return rc;
    std::memcpy(out_levels[levels - 1], image, N * sizeof(float));  // image.copy(), :40
    for (int l = levels - 2; l >= 0; l--) {
        int h = dims[2 * (l + 1)], w = dims[2 * (l + 1) + 1];
        int ho = dims[2 * l], wo = dims[2 * l + 1];
        rc = launch_pyr_down(nullptr, gauss, nullptr, cur, nxt, tA, tB, 1, h, w, ho, wo);
        if (rc) return rc;
        if ((rc = call.to_host(out_levels[l], nxt, (size_t)ho * wo))) return rc;
        std::swap(cur, nxt);
    }
    return call.sync();
}
}  // namespace

OFLK_API int oflk_warp(const float *image, const float *flow_u, const float *flow_v, int H, int W,
                       float *out)
{
    int rc = check_hw(image, flow_u, H, W);
    if (rc) return rc;
    if (!flow_v || !out) return fail(OFLK_ERR_INVALID, "NULL argument");
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t n = (size_t)H * W;
    float *d[4];
    if ((rc = call.upload(&d[0], image, n)) || (rc = call.upload(&d[1], flow_u, n)) || (rc = call.upload(&d[2], flow_v, n)) ||
        (rc = call.alloc(&d[3], n)))
        return rc;
    hipLaunchKernelGGL(k_warp, grid2d(W, H, 1), dim3(256), 0, nullptr, (const float *)d[0],
                       (const float *)d[1], (const float *)d[2], d[3], H, W);
    HIP_TRY(hipGetLastError());
    if ((rc = call.to_host(out, d[3], n))) return rc;
    return call.sync();
}

OFLK_API int oflk_upsample_flow(const float *flow_u, const float *flow_v, int Hc, int Wc, int Ht,
                                int Wt, float *u_out, float *v_out)
{
    int rc = check_hw(flow_u, flow_v, Hc, Wc);
    if (rc) return rc;
    if ((rc = check_hw(u_out, v_out, Ht, Wt))) return rc;
    HostCall call;
    if ((rc = call.begin())) return rc;
    const size_t nc = (size_t)Hc * Wc, nt = (size_t)Ht * Wt;
    float *du, *dv, *ou, *ov;
    if ((rc = call.upload(&du, flow_u, nc)) || (rc = call.upload(&dv, flow_v, nc)) || (rc = call.alloc(&ou, nt)) ||
        (rc = call.alloc(&ov, nt)))
        return rc;
    ResampleArgs r = upsample_args(Hc, Wc, Ht, Wt);
    r.in[0] = du; r.in[1] = dv;
    r.out[0] = ou; r.out[1] = ov;
    if ((rc = launch_upsample(nullptr, nullptr, r, 1))) return rc;
    if ((rc = call.to_host(u_out, ou, nt)) || (rc = call.to_host(v_out, ov, nt))) return rc;
    return call.sync();
}
