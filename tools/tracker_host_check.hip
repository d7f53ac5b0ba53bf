// Host-side check of the online tracker for a sanitizer build (make -C optical-flow-fpga_amd/csrc tracker-host-check):
// create, every refusal that needs no device, destroy, and the host-side point filter of oflk_tracker_add_points.  It
// includes the library's translation unit so that the filter, which the ABI reaches only after a pushed frame, can be
// called on a machine without a GPU.  Exit status 0: every expectation held (and the sanitizers found nothing).
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

static int create(oflk_tracker **tr, int H, int W, int u8, int L, int w, int it, float alpha, float beta, float mr, float q, float md,
                  int K, int D)
{
    return oflk_tracker_create(tr, 0, H, W, u8, L, w, it, alpha, beta, mr, q, md, K, D);
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    oflk_tracker *tr = nullptr;
    // refusals of creation
    EXPECT(oflk_tracker_create(nullptr, 0, 24, 32, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID);
    EXPECT(create(&tr, 24, 32, 0, 3, 4, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_UNSUPPORTED && !tr);
    EXPECT(create(&tr, 24, 32, 1, 3, 13, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_UNSUPPORTED && !tr);
    EXPECT(create(&tr, 7, 9, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_UNSUPPORTED && !tr);
    EXPECT(create(&tr, 0, 32, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 0, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, OFLK_MAX_LEVELS + 1, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 0, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, -1.0f, 0.5f, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, 0.01f, nan, 4.0f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, 0.01f, 0.5f, -0.5f, 0.01f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 2.0f, 3.0f, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, inf, 8, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 0, 2) == OFLK_ERR_INVALID && !tr);
    EXPECT(create(&tr, 24, 32, 0, 3, 5, 3, 0.01f, 0.5f, 4.0f, 0.01f, 3.0f, 8, -1) == OFLK_ERR_INVALID && !tr);
    // a tracker, and what it refuses before the first push
    for (int u8 = 0; u8 < 2; u8++)
        for (int D : {0, 1, INT_MAX}) {
            EXPECT(create(&tr, 24, 32, u8, 3, 5, 3, 0.01f, 0.5f, inf, 0.0f, 0.0f, 5, D) == OFLK_OK && tr);
            if (!tr) continue;
            EXPECT(oflk_tracker_frame_index(tr) == -1 && oflk_tracker_workspace_bytes(tr) == 0);
            const float *xy = nullptr;
            EXPECT(oflk_tracker_row_device(tr, &xy, nullptr, nullptr, nullptr, nullptr, nullptr) == OFLK_ERR_INVALID && !xy);
            EXPECT(oflk_tracker_read_row(tr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == OFLK_ERR_INVALID);
            const float one[2] = {3.0f, 4.0f};
            EXPECT(oflk_tracker_add_points(tr, one, 1, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_tracker_push_device(tr, nullptr, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_tracker_push(tr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_tracker_reset(tr, nullptr) == OFLK_OK && oflk_tracker_frame_index(tr) == -1);
            // the filter: 32 x 24 frames, 5 slots
            const float pts[] = {nan, 3, 5, 6, -0.5f, 3, 31, 23, 31.5f, 3, 3, 23.25f, inf, 1, -0.0f, 0, 1, nan, 7, 7, 8, 8, 9, 9, 10, 10};
            std::vector<float> keep = tracker_filter_points(tr, pts, 13);
            const float want[] = {5, 6, 31, 23, -0.0f, 0, 7, 7, 8, 8};   // five slots: (9, 9) and (10, 10) are not read
            EXPECT(keep.size() == 10 && std::memcmp(keep.data(), want, sizeof(want)) == 0);
            EXPECT(tracker_filter_points(tr, pts, 1).empty());
            EXPECT(tracker_filter_points(tr, pts + 2, 1).size() == 2);
            EXPECT(oflk_tracker_destroy(tr) == OFLK_OK);
            tr = nullptr;
        }
    EXPECT(oflk_tracker_destroy(nullptr) == OFLK_OK);
    EXPECT(oflk_tracker_reset(nullptr, nullptr) == OFLK_ERR_INVALID);
    std::printf(g_failed ? "tracker host check: %d expectation(s) failed\n" : "tracker host check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
