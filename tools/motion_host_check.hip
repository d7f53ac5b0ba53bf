// Host-side check of the global motion fit for a sanitizer build (make -C optical-flow-fpga_amd/csrc motion-host-check):
// the workspace layout, every refusal of oflk_motion_workspace / oflk_estimate_motion / oflk_tracks_motion /
// oflk_estimate_motion_host and the tracker's motion settings, none of which needs a device.  It includes the library's
// translation unit so that the workspace's pieces can be checked against its size.  Exit status 0: every expectation held
// (and the sanitizers found nothing).
#include "../optical-flow-fpga_amd/csrc/oflk.hip"

#include <cstdio>
#include <limits>

static int g_failed = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            g_failed++;                                                     \
        }                                                                   \
    } while (0)

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the workspace: pieces in order, 256-byte aligned, inside the size the ABI reports
    for (int S : {1, 3, 70000})
        for (int N : {1, 65, 10000})
            for (int Hn : {1, 257, OFLK_MOTION_MAX_HYPOTHESES}) {
                size_t bytes = 0;
                EXPECT(oflk_motion_workspace(S, N, Hn, &bytes) == OFLK_OK);
                char *base = reinterpret_cast<char *>(uintptr_t(1) << 20);   // an address, never read
                const MotionWs w = motion_ws(base, S, N, Hn);
                EXPECT(w.bytes == bytes && bytes % 256 == 0);
                EXPECT((char *)w.M == base && (char *)(w.M + S) <= (char *)w.pts);
                EXPECT((char *)(w.pts + (size_t)S * N) <= (char *)w.score && (char *)(w.score + (size_t)S * Hn) <= (char *)w.hmodel);
                EXPECT((char *)(w.hmodel + (size_t)S * Hn * 6) <= base + bytes);
                for (const void *p : {(const void *)w.pts, (const void *)w.score, (const void *)w.hmodel}) EXPECT(aligned(p, 256));
            }
    size_t bytes = 0;
    EXPECT(oflk_motion_workspace(2, 10, 16, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_motion_workspace(0, 10, 16, &bytes) == OFLK_ERR_INVALID && oflk_motion_workspace(2, 0, 16, &bytes) == OFLK_ERR_INVALID);
    EXPECT(oflk_motion_workspace(2, 10, 0, &bytes) == OFLK_ERR_INVALID);
    EXPECT(oflk_motion_workspace(2, 10, OFLK_MOTION_MAX_HYPOTHESES + 1, &bytes) == OFLK_ERR_INVALID);
    EXPECT(oflk_motion_workspace(2, 10, 16, &bytes) == OFLK_OK && bytes > 0);

    // the device forms: addresses that are never read, since every refusal comes before a device call
    float *p = reinterpret_cast<float *>(uintptr_t(1) << 20);
    unsigned char *b = reinterpret_cast<unsigned char *>(uintptr_t(2) << 20);
    int *c = reinterpret_cast<int *>(uintptr_t(3) << 20);
    void *ws = reinterpret_cast<void *>(uintptr_t(4) << 20);
    auto est = [&](const float *src, const float *dst, int S, int N, int model, int Hn, float thr, void *w, size_t wb, float *om,
                   unsigned char *oi, int *oc) {
        return oflk_estimate_motion(src, dst, nullptr, S, N, 0, model, Hn, thr, 0, w, wb, om, oi, oc, nullptr);
    };
    EXPECT(est(p, p, 2, 10, 3, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, -1, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 0, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, OFLK_MOTION_MAX_HYPOTHESES + 1, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    for (float thr : {0.0f, -1.0f, nan, inf, -inf}) EXPECT(est(p, p, 2, 10, 1, 16, thr, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 0, 10, 1, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, -3, 1, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(nullptr, p, 2, 10, 1, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, nullptr, 2, 10, 1, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p + 1, p, 2, 10, 1, 16, 1.0f, ws, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 16, 1.0f, nullptr, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 16, 1.0f, ws, bytes - 1, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 16, 1.0f, (char *)ws + 128, bytes, p, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 16, 1.0f, ws, bytes, nullptr, b, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 16, 1.0f, ws, bytes, p, nullptr, c) == OFLK_ERR_INVALID);
    EXPECT(est(p, p, 2, 10, 1, 16, 1.0f, ws, bytes, p, b, nullptr) == OFLK_ERR_INVALID);
    auto trk = [&](const float *rows, const unsigned char *vis, int T, int K, int model, size_t wb) {
        return oflk_tracks_motion(rows, vis, nullptr, T, K, 0, model, 16, 1.0f, 0, ws, wb, p, b, c, nullptr);
    };
    EXPECT(trk(p, b, 1, 10, 1, bytes) == OFLK_ERR_INVALID && trk(p, b, 3, 0, 1, bytes) == OFLK_ERR_INVALID);
    EXPECT(trk(nullptr, b, 3, 10, 1, bytes) == OFLK_ERR_INVALID && trk(p, nullptr, 3, 10, 1, bytes) == OFLK_ERR_INVALID);
    EXPECT(trk(p + 1, b, 3, 10, 1, bytes) == OFLK_ERR_INVALID && trk(p, b, 3, 10, 5, bytes) == OFLK_ERR_INVALID);
    EXPECT(trk(p, b, 3, 10, 1, bytes - 1) == OFLK_ERR_INVALID);   // T = 3 is S = 2: the same workspace
    // the host form refuses the same before it touches a device
    float h[40] = {0}, om[12];
    unsigned char oi[20];
    int oc[6];
    EXPECT(oflk_estimate_motion_host(nullptr, h, nullptr, 2, 10, 0, 1, 16, 1.0f, 0, om, oi, oc) == OFLK_ERR_INVALID);
    EXPECT(oflk_estimate_motion_host(h, h, nullptr, 2, 10, 0, 1, 16, 1.0f, 0, nullptr, oi, oc) == OFLK_ERR_INVALID);
    EXPECT(oflk_estimate_motion_host(h, h, nullptr, 0, 10, 0, 1, 16, 1.0f, 0, om, oi, oc) == OFLK_ERR_INVALID);
    EXPECT(oflk_estimate_motion_host(h, h, nullptr, 2, 10, 0, 9, 16, 1.0f, 0, om, oi, oc) == OFLK_ERR_INVALID);
    EXPECT(oflk_estimate_motion_host(h, h, nullptr, 2, 10, 0, 1, 16, nan, 0, om, oi, oc) == OFLK_ERR_INVALID);

    // the tracker's settings
    oflk_tracker *tr = nullptr;
    EXPECT(oflk_tracker_create(&tr, 0, 24, 32, 1, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_OK && tr);
    if (tr) {
        EXPECT(oflk_tracker_set_motion(tr, OFLK_MOTION_AFFINE, 64, 1.5f, 7u) == OFLK_OK && tr->fit.model == 2 && tr->fit.hypotheses == 64);
        EXPECT(oflk_tracker_set_motion(tr, 3, 64, 1.0f, 0) == OFLK_ERR_INVALID && tr->fit.model == 2);
        EXPECT(oflk_tracker_set_motion(tr, -2, 64, 1.0f, 0) == OFLK_ERR_INVALID);
        EXPECT(oflk_tracker_set_motion(tr, 1, 0, 1.0f, 0) == OFLK_ERR_INVALID && oflk_tracker_set_motion(tr, 1, 64, 0.0f, 0) == OFLK_ERR_INVALID);
        EXPECT(oflk_tracker_set_motion(tr, -1, 0, nan, 0) == OFLK_OK && tr->fit.model == -1);   // off: the rest is ignored
        const float *m = nullptr;
        EXPECT(oflk_tracker_motion_device(tr, &m, nullptr, nullptr) == OFLK_ERR_INVALID && !m);
        EXPECT(oflk_tracker_read_motion(tr, om, oi, oc, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_tracker_workspace_bytes(tr) == 0);
        EXPECT(oflk_tracker_destroy(tr) == OFLK_OK);
    }
    EXPECT(oflk_tracker_set_motion(nullptr, 1, 64, 1.0f, 0) == OFLK_ERR_INVALID);
    std::printf(g_failed ? "motion host check: %d expectation(s) failed\n" : "motion host check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
