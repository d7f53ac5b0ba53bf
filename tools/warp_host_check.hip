// Host-side check of the frame layouts' refusals for a sanitizer build (make -C optical-flow-fpga_amd/csrc warp-host-check):
// the six device and six host warps (affine and perspective; planar float32 / uint8, packed, NV12), oflk_luma_u8 and its
// host form, the four sequence stabilisers and the three oflk_stabilizer_create*.  Every call here is refused before any
// device call, and the check holds both the return code and the exact text of oflk_last_error().  Most cases break one
// argument; the ones marked "two" break two, and so pin which refusal comes first.  The texts were recorded from the
// library as it stood before the three layouts were given one host path; that path has to give them again.  It includes
// the library's translation unit and runs on a machine without a GPU.  Exit status 0: every expectation held (and the
// sanitizers found nothing).
#include "../optical-flow-fpga_amd/csrc/oflk.hip"

#include <cstdarg>
#include <cstdio>
#include <cstring>

static int g_failed = 0, g_cases = 0;

static void refused(int line, int rc, int want, const char *text)
{
    g_cases++;
    const char *got = oflk_last_error();
    if (rc == want && !std::strcmp(got, text)) return;
    std::printf("%s:%d: got %d \"%s\", expected %d \"%s\"\n", __FILE__, line, rc, got, want, text);
    g_failed++;
}
#define REFUSED(call, want, text) refused(__LINE__, (call), (want), (text))
#define INVALID(call, text) REFUSED(call, OFLK_ERR_INVALID, text)
#define UNSUPPORTED(call, text) REFUSED(call, OFLK_ERR_UNSUPPORTED, text)

// a formatted expectation; a few live at a time
static const char *fmt(const char *f, ...)
{
    static char buf[4][256];
    static int at = 0;
    char *b = buf[at++ & 3];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof(buf[0]), f, ap);
    va_end(ap);
    return b;
}

static const char *kNull = "NULL input or output argument";
static const char *k2_30 = "frames of 2^30 pixels or more are not supported";
static const char *k2_31 = "packed frames of 2^31 bytes or more are not supported";
static const char *kMap8 = "d_map must be 8-byte aligned";
static const char *kF32 = "float32 frames must be 4-byte aligned";
static const char *e_f(int F) { return fmt("F must be >= 1 (got %d)", F); }
static const char *e_hw(int H, int W) { return fmt("H and W must be >= 2 (got %d x %d)", H, W); }
static const char *e_dim(int H, int W) { return fmt("frames of 2^23 rows or columns or more are not supported (got %d x %d)", H, W); }
static const char *e_ch(int c) { return fmt("channels must be 3 or 4 (got %d)", c); }
static const char *e_order(int o) { return fmt("order must be OFLK_ORDER_RGB or OFLK_ORDER_BGR (got %d)", o); }
static const char *e_nv12(int H, int W) { return fmt("NV12 frames need even H and W >= 4 (got %d x %d)", H, W); }
static const char *e_siting(int s) { return fmt("siting must be OFLK_SITING_LEFT or OFLK_SITING_CENTER (got %d)", s); }
static const char *e_t(int T) { return fmt("a sequence needs T >= 2 frames (got %d)", T); }

static double g_w[OFLK_STABILIZE_MAX_RADIUS + 1];
alignas(16) static double g_map[9 * 2];
alignas(16) static unsigned char g_in[2 * 4 * 4 * 4 * 4], g_out[2 * 4 * 4 * 4 * 4];   // two 4 x 4 frames of any layout

// what a sequence call or a creation takes besides its frames
struct Cfg {
    int levels = 1, win = 5, iters = 3;
    float alpha = 0.01f, beta = 0.5f, res = 4.0f, q = 0.01f, md = 3.0f;
    int K = 8, every = 2, model = OFLK_MOTION_SIMILARITY, hyps = 16;
    float thr = 1.0f;
    const double *w = g_w;
    int radius = 3;
};

int main()
{
    for (double &v : g_w) v = 1.0;
    double *const map = g_map, *const map4 = reinterpret_cast<double *>(reinterpret_cast<char *>(g_map) + 4);
    unsigned char *const in = g_in, *const out = g_out;
    const int big = 32768, wide = 1 << 23;   // big x big pixels: 2^30; 30000 x 30000 x 3 bytes: past 2^31 below 2^30 pixels
    const int L = OFLK_SITING_LEFT, RGB = OFLK_ORDER_RGB;

    // ---- the planar warps: device (float32, uint8) and host, affine and perspective ----
    for (int persp = 0; persp < 2; persp++)
        for (int u8 = 0; u8 < 2; u8++) {
            auto dev = [&](const void *f, int F, int H, int W, const double *m, void *o) {
                return persp ? oflk_warp_perspective(f, u8, F, H, W, m, o, nullptr, nullptr)
                             : oflk_warp_affine(f, u8, F, H, W, m, o, nullptr, nullptr);
            };
            auto host = [&](const void *f, int F, int H, int W, const double *m, void *o) {
                if (u8)
                    return persp ? oflk_warp_perspective_host_u8((const unsigned char *)f, F, H, W, m, (unsigned char *)o, nullptr)
                                 : oflk_warp_affine_host_u8((const unsigned char *)f, F, H, W, m, (unsigned char *)o, nullptr);
                return persp ? oflk_warp_perspective_host((const float *)f, F, H, W, m, (float *)o, nullptr)
                             : oflk_warp_affine_host((const float *)f, F, H, W, m, (float *)o, nullptr);
            };
            for (int h = 0; h < 2; h++) {
                auto call = [&](const void *f, int F, int H, int W, const double *m, void *o) {
                    return h ? host(f, F, H, W, m, o) : dev(f, F, H, W, m, o);
                };
                INVALID(call(in, 0, 4, 4, map, out), e_f(0));
                INVALID(call(in, -3, 4, 4, map, out), e_f(-3));
                INVALID(call(in, 2, 1, 4, map, out), e_hw(1, 4));
                INVALID(call(in, 2, 4, 0, map, out), e_hw(4, 0));
                INVALID(call(nullptr, 2, 4, 4, map, out), kNull);
                INVALID(call(in, 2, 4, 4, nullptr, out), kNull);
                INVALID(call(in, 2, 4, 4, map, nullptr), kNull);
                UNSUPPORTED(call(in, 1, big, big, map, out), k2_30);
                UNSUPPORTED(call(in, 1, 2, wide, map, out), e_dim(2, wide));
                UNSUPPORTED(call(in, 1, wide, 2, map, out), e_dim(wide, 2));
                INVALID(call(in, 0, 1, 4, map, out), e_f(0));                  // two: F, then the shape
                INVALID(call(nullptr, 2, 1, 4, map, out), e_hw(1, 4));        // two: the shape, then NULL
                INVALID(call(in, 1, big, big, nullptr, out), kNull);           // two: a planar call's NULL map, then the size
                INVALID(call(in, 1, big, big, map, nullptr), kNull);           // two: NULL out, then the size
            }
            INVALID(dev(in, 2, 4, 4, map4, out), kMap8);
            INVALID(dev(in, 2, 4, 4, map4, nullptr), kNull);                   // two: NULL out, then the map's alignment
            INVALID(dev(in, 2, 4, 4, nullptr, out), kNull);                    // a NULL map is NULL, not misaligned
            UNSUPPORTED(dev(in, 1, big, big, map4, out), k2_30);               // two: the size, then the map's alignment
            if (!u8) {
                INVALID(dev(in + 1, 2, 4, 4, map, out), kF32);
                INVALID(dev(in, 2, 4, 4, map, out + 2), kF32);
                INVALID(dev(in + 1, 2, 4, 4, map4, out), kMap8);               // two: the map's alignment, then the frames'
                INVALID(dev(in + 1, 0, 4, 4, map, out), e_f(0));               // two: F, then the frames' alignment
            }
        }

    // ---- the packed warps ----
    for (int persp = 0; persp < 2; persp++)
        for (int h = 0; h < 2; h++) {
            auto call = [&](const unsigned char *f, int F, int H, int W, int C, const double *m, unsigned char *o) {
                if (h)
                    return persp ? oflk_warp_perspective_packed_host(f, F, H, W, C, m, o, nullptr)
                                 : oflk_warp_affine_packed_host(f, F, H, W, C, m, o, nullptr);
                return persp ? oflk_warp_perspective_packed(f, F, H, W, C, m, o, nullptr, nullptr)
                             : oflk_warp_affine_packed(f, F, H, W, C, m, o, nullptr, nullptr);
            };
            for (int C : {0, 1, 2, 5, -3}) INVALID(call(in, 2, 4, 4, C, map, out), e_ch(C));
            for (int C : {3, 4}) {
                INVALID(call(in, 0, 4, 4, C, map, out), e_f(0));
                INVALID(call(in, 2, 1, 4, C, map, out), e_hw(1, 4));
                INVALID(call(in, 2, 4, 1, C, map, out), e_hw(4, 1));
                INVALID(call(nullptr, 2, 4, 4, C, map, out), kNull);
                INVALID(call(in, 2, 4, 4, C, map, nullptr), kNull);
                INVALID(call(in, 2, 4, 4, C, nullptr, out), kNull);
                UNSUPPORTED(call(in, 1, big, big, C, map, out), k2_30);
                UNSUPPORTED(call(in, 1, 2, wide, C, map, out), e_dim(2, wide));
                UNSUPPORTED(call(in, 1, 30000, 30000, C, map, out), k2_31);
                UNSUPPORTED(call(in, 1, 30000, 30000, C, nullptr, out), k2_31);   // two: H W C >= 2^31, then the NULL map
                UNSUPPORTED(call(in, 1, big, big, C, nullptr, out), k2_30);        // two: the size, then the NULL map
                INVALID(call(in, 1, 30000, 30000, C, map, nullptr), kNull);        // two: NULL out, then the byte count
                INVALID(call(nullptr, 0, 4, 4, C, nullptr, out), e_f(0));          // three: F first
            }
            INVALID(call(in, 0, 4, 4, 2, map, out), e_ch(2));                      // two: channels, then F
            INVALID(call(in, 2, 1, 1, 7, nullptr, nullptr), e_ch(7));              // channels ahead of everything
            if (!h) {
                INVALID(call(in, 2, 4, 4, 3, map4, out), kMap8);
                INVALID(call(in, 2, 4, 4, 4, map4, nullptr), kNull);               // two: NULL out, then the map's alignment
                UNSUPPORTED(call(in, 1, 30000, 30000, 3, map4, out), k2_31);       // two: the byte count, then the alignment
            }
        }

    // ---- the NV12 warps ----
    for (int persp = 0; persp < 2; persp++)
        for (int h = 0; h < 2; h++) {
            auto call = [&](const unsigned char *f, int F, int H, int W, int siting, const double *m, unsigned char *o) {
                if (h)
                    return persp ? oflk_warp_perspective_nv12_host(f, F, H, W, siting, m, o, nullptr)
                                 : oflk_warp_affine_nv12_host(f, F, H, W, siting, m, o, nullptr);
                return persp ? oflk_warp_perspective_nv12(f, F, H, W, siting, m, o, nullptr, nullptr)
                             : oflk_warp_affine_nv12(f, F, H, W, siting, m, o, nullptr, nullptr);
            };
            INVALID(call(in, 2, 5, 4, L, map, out), e_nv12(5, 4));
            INVALID(call(in, 2, 4, 7, L, map, out), e_nv12(4, 7));
            INVALID(call(in, 2, 2, 4, L, map, out), e_nv12(2, 4));
            INVALID(call(in, 2, 4, 2, L, map, out), e_nv12(4, 2));
            INVALID(call(in, 2, 0, 0, L, map, out), e_nv12(0, 0));
            for (int siting : {-1, 2}) INVALID(call(in, 2, 4, 4, siting, map, out), e_siting(siting));
            for (int siting : {OFLK_SITING_LEFT, OFLK_SITING_CENTER}) {
                INVALID(call(in, 0, 4, 4, siting, map, out), e_f(0));
                INVALID(call(nullptr, 2, 4, 4, siting, map, out), kNull);
                INVALID(call(in, 2, 4, 4, siting, map, nullptr), kNull);
                INVALID(call(in, 2, 4, 4, siting, nullptr, out), kNull);
                UNSUPPORTED(call(in, 1, big, big, siting, map, out), k2_30);
                UNSUPPORTED(call(in, 1, 4, wide, siting, map, out), e_dim(4, wide));
                UNSUPPORTED(call(in, 1, big, big, siting, nullptr, out), k2_30);   // two: the size, then the NULL map
                INVALID(call(in, 1, big, big, siting, map, nullptr), kNull);       // two: NULL out, then the size
            }
            INVALID(call(in, 2, 5, 4, L, map, nullptr), e_nv12(5, 4));             // two: odd H, then NULL out
            INVALID(call(in, 2, 5, 4, 9, map, out), e_nv12(5, 4));                 // two: the shape, then the siting
            INVALID(call(in, 0, 4, 4, 9, map, out), e_siting(9));                  // two: the siting, then F
            INVALID(call(nullptr, 0, 4, 4, L, map, out), e_f(0));                  // two: F, then NULL
            if (!h) {
                INVALID(call(in, 2, 4, 4, L, map4, out), kMap8);
                INVALID(call(in, 2, 4, 4, L, map4, nullptr), kNull);               // two: NULL out, then the map's alignment
                INVALID(call(in, 2, 4, 6, 3, map4, out), e_siting(3));             // two: the siting, then the alignment
            }
        }

    // ---- luma ----
    for (int h = 0; h < 2; h++) {
        auto call = [&](const unsigned char *f, int F, int H, int W, int C, int order, unsigned char *o) {
            return h ? oflk_luma_u8_host(f, F, H, W, C, order, o) : oflk_luma_u8(f, F, H, W, C, order, o, nullptr);
        };
        for (int C : {0, 2, 5}) INVALID(call(in, 2, 4, 4, C, RGB, out), e_ch(C));
        for (int order : {-1, 2}) INVALID(call(in, 2, 4, 4, 3, order, out), e_order(order));
        INVALID(call(in, 0, 4, 4, 3, RGB, out), e_f(0));
        INVALID(call(in, 2, 4, 1, 4, OFLK_ORDER_BGR, out), e_hw(4, 1));
        INVALID(call(nullptr, 2, 4, 4, 3, RGB, out), kNull);
        INVALID(call(in, 2, 4, 4, 4, RGB, nullptr), kNull);
        UNSUPPORTED(call(in, 1, big, big, 3, RGB, out), k2_30);
        UNSUPPORTED(call(in, 1, 30000, 30000, 3, RGB, out), k2_31);
        INVALID(call(in, 2, 4, 4, 2, 7, out), e_ch(2));                            // two: channels, then the order
        INVALID(call(in, 2, 4, 4, 3, 7, nullptr), kNull);                          // two: NULL luma, then the order
        UNSUPPORTED(call(in, 1, 30000, 30000, 4, 7, out), k2_31);                  // two: the byte count, then the order
        INVALID(call(in, 0, 4, 4, 3, 7, out), e_f(0));                             // two: F, then the order
    }

    // ---- the sequence stabilisers ----
    // layout 0: float32, 1: uint8, 2: packed (a: channels, b: order), 3: NV12 (a: siting)
    auto seq = [&](int layout, const void *f, int T, int H, int W, int a, int b, const Cfg &c, void *o) {
        switch (layout) {
        case 0:
            return oflk_stabilize_sequence((const float *)f, T, H, W, c.levels, c.win, c.iters, c.alpha, c.beta, c.res, c.q, c.md, c.K,
                                           c.every, c.model, c.hyps, c.thr, 7u, c.w, c.radius, (float *)o, nullptr, nullptr, nullptr,
                                           nullptr);
        case 1:
            return oflk_stabilize_sequence_u8((const unsigned char *)f, T, H, W, c.levels, c.win, c.iters, c.alpha, c.beta, c.res, c.q,
                                              c.md, c.K, c.every, c.model, c.hyps, c.thr, 7u, c.w, c.radius, (unsigned char *)o, nullptr,
                                              nullptr, nullptr, nullptr);
        case 2:
            return oflk_stabilize_sequence_packed((const unsigned char *)f, T, H, W, a, b, c.levels, c.win, c.iters, c.alpha, c.beta,
                                                  c.res, c.q, c.md, c.K, c.every, c.model, c.hyps, c.thr, 7u, c.w, c.radius,
                                                  (unsigned char *)o, nullptr, nullptr, nullptr, nullptr);
        default:
            return oflk_stabilize_sequence_nv12((const unsigned char *)f, T, H, W, a, c.levels, c.win, c.iters, c.alpha, c.beta, c.res,
                                                c.q, c.md, c.K, c.every, c.model, c.hyps, c.thr, 7u, c.w, c.radius, (unsigned char *)o,
                                                nullptr, nullptr, nullptr, nullptr);
        }
    };
    const Cfg ok;
    Cfg bad_model, bad_hyps, bad_thr, no_w, bad_radius, bad_every, bad_q, bad_k, bad_alpha, bad_levels, bad_win, both;
    bad_model.model = 9;
    bad_hyps.hyps = 0;
    bad_thr.thr = 0.0f;
    no_w.w = nullptr;
    bad_radius.radius = -1;
    bad_every.every = 0;
    bad_q.q = 2.0f;
    bad_k.K = 0;
    bad_alpha.alpha = -1.0f;
    bad_levels.levels = 0;
    bad_win.win = 4;
    both.model = 9;
    both.every = 0;
    for (int layout = 0; layout < 4; layout++) {
        const int a = layout == 2 ? 3 : L, b = RGB;
        INVALID(seq(layout, in, 1, 4, 4, a, b, ok, out), e_t(1));
        INVALID(seq(layout, in, 0, 4, 4, a, b, ok, out), e_t(0));
        INVALID(seq(layout, nullptr, 2, 4, 4, a, b, ok, out), kNull);
        INVALID(seq(layout, in, 2, 4, 4, a, b, ok, nullptr), kNull);
        UNSUPPORTED(seq(layout, in, 2, big, big, a, b, ok, out), k2_30);
        UNSUPPORTED(seq(layout, in, 2, 4, wide, a, b, ok, out), e_dim(4, wide));
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_model, out), "unknown motion model 9");
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_hyps, out), fmt("hypotheses must be in [1, %d] (got 0)", OFLK_MOTION_MAX_HYPOTHESES));
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_thr, out), "threshold must be finite and > 0 (got 0)");
        INVALID(seq(layout, in, 2, 4, 4, a, b, no_w, out), "NULL weights");
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_radius, out), fmt("radius must be in [0, %d] (got -1)", OFLK_STABILIZE_MAX_RADIUS));
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_every, out), "detect_every must be >= 1 (got 0)");
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_q, out), "quality_level must be in [0,1] (got 2)");
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_k, out), "max_corners must be >= 1 (got 0)");
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_alpha, out), "alpha and beta must be finite and >= 0 (got -1, 0.5)");
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_levels, out), fmt("levels must be in [1,%d] (got 0)", OFLK_MAX_LEVELS));
        UNSUPPORTED(seq(layout, in, 2, 4, 4, a, b, bad_win, out), "the sparse tracker is built for the odd windows 3 ... 11 (got 4)");
        INVALID(seq(layout, nullptr, 1, 4, 4, a, b, ok, out), e_t(1));                       // two: T, then NULL
        INVALID(seq(layout, in, 2, 4, 4, a, b, bad_model, nullptr), kNull);                   // two: NULL out, then the model
        UNSUPPORTED(seq(layout, in, 2, big, big, a, b, bad_model, out), k2_30);               // two: the size, then the model
        INVALID(seq(layout, in, 2, 4, 4, a, b, both, out), "unknown motion model 9");         // two: the model, then detect_every
    }
    for (int layout = 0; layout < 2; layout++) {
        INVALID(seq(layout, in, 2, 1, 4, 0, 0, ok, out), e_hw(1, 4));
        INVALID(seq(layout, in, 1, 1, 4, 0, 0, ok, out), e_t(1));                             // two: T, then the shape
        INVALID(seq(layout, nullptr, 2, 4, 1, 0, 0, ok, out), e_hw(4, 1));                    // two: the shape, then NULL
    }
    INVALID(seq(2, in, 2, 4, 4, 2, RGB, ok, out), e_ch(2));
    INVALID(seq(2, in, 2, 4, 4, 3, 7, ok, out), e_order(7));
    INVALID(seq(2, in, 2, 1, 4, 3, RGB, ok, out), e_hw(1, 4));
    UNSUPPORTED(seq(2, in, 2, 30000, 30000, 3, RGB, ok, out), k2_31);
    INVALID(seq(2, in, 1, 4, 4, 5, RGB, ok, out), e_ch(5));                                   // two: channels, then T < 2
    INVALID(seq(2, in, 1, 4, 4, 4, 7, ok, out), e_order(7));                                  // two: the order, then T < 2
    INVALID(seq(2, in, 2, 4, 4, 5, 7, ok, out), e_ch(5));                                     // two: channels, then the order
    INVALID(seq(2, in, 1, 1, 4, 3, RGB, ok, out), e_t(1));                                    // two: T, then the shape
    UNSUPPORTED(seq(2, in, 2, 30000, 30000, 4, RGB, bad_model, out), k2_31);                  // two: the byte count, then the model
    INVALID(seq(2, in, 2, 30000, 30000, 4, RGB, ok, nullptr), kNull);                         // two: NULL out, then the byte count
    INVALID(seq(3, in, 2, 5, 4, L, 0, ok, out), e_nv12(5, 4));
    INVALID(seq(3, in, 2, 4, 2, L, 0, ok, out), e_nv12(4, 2));
    INVALID(seq(3, in, 2, 4, 4, 7, 0, ok, out), e_siting(7));
    INVALID(seq(3, in, 2, 5, 4, L, 0, ok, nullptr), e_nv12(5, 4));                            // two: odd H, then NULL out
    INVALID(seq(3, in, 1, 4, 6, 7, 0, ok, out), e_siting(7));                                 // two: the siting, then T < 2
    INVALID(seq(3, in, 1, 3, 4, L, 0, ok, out), e_nv12(3, 4));                                // two: the shape, then T < 2

    // ---- the three creations ----
    oflk_stabilizer *st = nullptr;
    auto create = [&](int layout, oflk_stabilizer **s, int H, int W, int a, int b, const Cfg &c) {
        switch (layout) {
        case 0:
        case 1:
            return oflk_stabilizer_create(s, 0, H, W, layout, c.levels, c.win, c.iters, c.alpha, c.beta, c.res, c.q, c.md, c.K, c.every,
                                          c.model, c.hyps, c.thr, 7u, c.w, c.radius);
        case 2:
            return oflk_stabilizer_create_packed(s, 0, H, W, a, b, c.levels, c.win, c.iters, c.alpha, c.beta, c.res, c.q, c.md, c.K,
                                                 c.every, c.model, c.hyps, c.thr, 7u, c.w, c.radius);
        default:
            return oflk_stabilizer_create_nv12(s, 0, H, W, a, c.levels, c.win, c.iters, c.alpha, c.beta, c.res, c.q, c.md, c.K, c.every,
                                               c.model, c.hyps, c.thr, 7u, c.w, c.radius);
        }
    };
    Cfg neg_every;
    neg_every.every = -1;
    for (int layout = 0; layout < 4; layout++) {
        const int a = layout == 2 ? 4 : L, b = OFLK_ORDER_BGR;
        INVALID(create(layout, nullptr, 24, 32, a, b, ok), "stabiliser pointer is NULL");
        INVALID(create(layout, &st, 24, 32, a, b, bad_model), "unknown motion model 9");
        INVALID(create(layout, &st, 24, 32, a, b, bad_hyps), fmt("hypotheses must be in [1, %d] (got 0)", OFLK_MOTION_MAX_HYPOTHESES));
        INVALID(create(layout, &st, 24, 32, a, b, no_w), "NULL weights");
        INVALID(create(layout, &st, 24, 32, a, b, bad_radius), fmt("radius must be in [0, %d] (got -1)", OFLK_STABILIZE_MAX_RADIUS));
        INVALID(create(layout, &st, 24, 32, a, b, bad_alpha), "alpha and beta must be finite and >= 0 (got -1, 0.5)");
        INVALID(create(layout, &st, 24, 32, a, b, bad_levels), fmt("levels must be in [1,%d] (got 0)", OFLK_MAX_LEVELS));
        UNSUPPORTED(create(layout, &st, 24, 32, a, b, bad_win), "the sparse tracker is built for the odd windows 3 ... 11 (got 4)");
        INVALID(create(layout, &st, 24, 32, a, b, bad_k), "max_corners must be >= 1 (got 0)");
        INVALID(create(layout, &st, 24, 32, a, b, neg_every), "detect_every must be >= 0 (0: never detect; got -1)");
        INVALID(create(layout, nullptr, 24, 32, a, b, bad_model), "stabiliser pointer is NULL");   // two: the pointer, then the model
        INVALID(create(layout, &st, 24, 32, a, b, both), "unknown motion model 9");
        REFUSED(create(layout, &st, big, big, a, b, bad_model), layout == 2 ? OFLK_ERR_UNSUPPORTED : OFLK_ERR_INVALID,
                layout == 2 ? k2_31 : "unknown motion model 9");                                   // two: only packed counts bytes first
        if (st) std::printf("%s:%d: a refused creation left a stabiliser\n", __FILE__, __LINE__), g_failed++;
    }
    for (int layout = 0; layout < 3; layout++) {
        const int a = layout == 2 ? 3 : 0;
        INVALID(create(layout, &st, 1, 32, a, RGB, ok), e_hw(1, 32));
        INVALID(create(layout, &st, 24, 1, a, RGB, bad_model), e_hw(24, 1));                       // two: the shape, then the model
    }
    INVALID(create(2, &st, 24, 32, 2, RGB, ok), e_ch(2));
    INVALID(create(2, &st, 24, 32, 3, 7, ok), e_order(7));
    UNSUPPORTED(create(2, &st, 30000, 30000, 3, RGB, ok), k2_31);
    INVALID(create(2, nullptr, 24, 32, 2, RGB, ok), "stabiliser pointer is NULL");                 // two: the pointer, then channels
    INVALID(create(2, &st, 24, 32, 2, 7, ok), e_ch(2));                                            // two: channels, then the order
    INVALID(create(2, &st, 1, 32, 5, RGB, ok), e_ch(5));                                           // two: channels, then the shape
    INVALID(create(2, &st, 1, wide, 4, RGB, ok), e_hw(1, wide));                                   // two: a shape too small is no byte count
    INVALID(create(3, &st, 23, 32, L, 0, ok), e_nv12(23, 32));
    INVALID(create(3, &st, 24, 2, L, 0, ok), e_nv12(24, 2));
    INVALID(create(3, &st, 24, 32, 5, 0, ok), e_siting(5));
    INVALID(create(3, &st, 23, 32, L, 0, bad_model), e_nv12(23, 32));                              // two: odd H, then the model
    INVALID(create(3, &st, 23, 32, 5, 0, ok), e_nv12(23, 32));                                     // two: the shape, then the siting
    INVALID(create(3, nullptr, 23, 32, L, 0, ok), "stabiliser pointer is NULL");                   // two: the pointer, then the shape
    if (st) std::printf("%s:%d: a refused creation left a stabiliser\n", __FILE__, __LINE__), g_failed++;
    // what is created holds its layout's frame size
    for (int layout = 0; layout < 4; layout++) {
        const int a = layout == 2 ? 3 : OFLK_SITING_CENTER;
        REFUSED(create(layout, &st, 24, 32, a, OFLK_ORDER_BGR, ok), OFLK_OK, oflk_last_error());
        if (!st) continue;
        const size_t want[4] = {24 * 32 * 4, 24 * 32, 24 * 32 * 3, 24 * 32 * 3 / 2};
        if (st->plane_bytes() != want[layout]) std::printf("%s:%d: layout %d: %zu bytes a frame\n", __FILE__, __LINE__, layout, st->plane_bytes()), g_failed++;
        oflk_stabilizer_destroy(st);
        st = nullptr;
    }
    if (g_failed)
        std::printf("warp host check: %d of %d expectation(s) failed\n", g_failed, g_cases);
    else
        std::printf("warp host check: ok (%d cases)\n", g_cases);
    return g_failed ? 1 : 0;
}
