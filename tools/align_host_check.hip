// Host-side check of direct image alignment for a sanitizer build (make -C optical-flow-fpga_amd/csrc align-host-check): the
// workspace sizing and layout and every refusal that needs no device, of the device forms and of the host forms.  It includes
// the library's translation unit and runs on a machine without a GPU.  Exit status 0: every expectation held (and the
// sanitizers found nothing).
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

alignas(256) static unsigned char g_buf[1024];   // stands for device memory: every call below is refused before it is touched

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const int A = OFLK_ALIGN_AFFINE, P = OFLK_ALIGN_HOMOGRAPHY;
    size_t n = 7;
    // the workspace: refusals and sizes
    EXPECT(oflk_align_workspace(1, 32, 32, 1, P, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_workspace(0, 32, 32, 1, P, &n) == OFLK_ERR_INVALID && n == 0);
    EXPECT(oflk_align_workspace(1, 0, 32, 1, P, &n) == OFLK_ERR_INVALID && n == 0);
    EXPECT(oflk_align_workspace(1, 32, 32, 0, P, &n) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_workspace(1, 32, 32, OFLK_MAX_LEVELS + 1, P, &n) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_workspace(1, 32, 32, 1, 2, &n) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_workspace(1, 32, 32, 1, -1, &n) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_workspace(1, 7, 32, 1, P, &n) == OFLK_ERR_UNSUPPORTED);        // the frame itself under 8 x 8
    EXPECT(oflk_align_workspace(1, 32, 31, 3, P, &n) == OFLK_ERR_UNSUPPORTED);       // 31 -> 15 -> 7
    EXPECT(oflk_align_workspace(1, 32, 32, 3, P, &n) == OFLK_OK && n > 0);           // 32 -> 16 -> 8
    EXPECT(oflk_align_workspace(1, 1 << 15, 1 << 15, 1, P, &n) == OFLK_ERR_UNSUPPORTED && n == 0);
    EXPECT(std::string(oflk_last_error()).find("2^30") != std::string::npos);
    for (int model : {A, P})
        for (int L : {1, 3})
            for (int S : {1, 5}) {
                int dims[2 * OFLK_MAX_LEVELS];
                AlignConfig cfg{L, 1, model, 0.25f, false, false, 0.0f};
                AlignIo io{};
                EXPECT(check_align(S, 70, 257, cfg, io, dims) == OFLK_OK);
                EXPECT(dims[2 * (L - 1)] == 70 && dims[2 * (L - 1) + 1] == 257);
                const AlignWs ws = align_ws(g_buf, S, dims, cfg);
                EXPECT(oflk_align_workspace(S, 70, 257, L, model, &n) == OFLK_OK && n == ws.bytes);
                // the pieces follow each other on 256-byte boundaries and end inside the size
                const size_t ns = model == P ? 46 : 29, tiles = 5 * 3;
                EXPECT(ws.pstride == tiles * ns && align_nsums(model, false, false) == (int)ns && align_tiles(70, 257) == (int)tiles);
                const char *b = reinterpret_cast<const char *>(g_buf);
                EXPECT(reinterpret_cast<const char *>(ws.state) == b);
                EXPECT(reinterpret_cast<const char *>(ws.partial) >= b + S * sizeof(AlignState) && aligned(ws.partial, 256));
                const char *end = reinterpret_cast<const char *>(ws.partial) + S * ws.pstride * sizeof(double);
                for (int l = 0; l < L - 1; l++) {
                    EXPECT(reinterpret_cast<const char *>(ws.pyr[l]) >= end && aligned(ws.pyr[l], 256));
                    end = reinterpret_cast<const char *>(ws.pyr[l]) + 2 * (size_t)S * dims[2 * l] * dims[2 * l + 1] * sizeof(float);
                }
                EXPECT(end <= b + ws.bytes && ws.bytes % 256 == 0);
            }
    // the device forms: every refusal comes before the pointers are used
    EXPECT(oflk_align_workspace(2, 32, 40, 2, P, &n) == OFLK_OK);
    void *d = g_buf;
    float *fm = reinterpret_cast<float *>(g_buf);
    int *im = reinterpret_cast<int *>(g_buf);
    double *dm = reinterpret_cast<double *>(g_buf);
    auto refine = [&](const void *a, const void *b, int u8, int S, int H, int W, int L, int it, int model, float share, const float *mi,
                      void *ws, size_t bytes, float *mo, int *so, double *st) {
        return oflk_align_refine(a, b, u8, S, H, W, L, it, model, share, mi, nullptr, ws, bytes, mo, so, st, nullptr);
    };
    EXPECT(refine(d, d, 0, 0, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 0, P, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(std::string(oflk_last_error()).find("iterations") != std::string::npos);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, 5, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(std::string(oflk_last_error()).find("model") != std::string::npos);
    for (float share : {0.0f, -0.5f, 1.5f, nan}) {
        EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, share, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);
        EXPECT(std::string(oflk_last_error()).find("min_share") != std::string::npos);
    }
    EXPECT(refine(d, d, 0, 2, 31, 40, 3, 1, P, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_UNSUPPORTED);   // 31 -> 15 -> 7 rows
    EXPECT(refine(nullptr, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, nullptr, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, nullptr, d, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, nullptr, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, nullptr, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, nullptr, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, im, nullptr) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n - 1, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(std::string(oflk_last_error()).find("oflk_align_workspace") != std::string::npos);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, g_buf + 128, n, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(refine(d, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, im, reinterpret_cast<double *>(g_buf + 4)) == OFLK_ERR_INVALID);
    EXPECT(refine(g_buf + 1, d, 0, 2, 32, 40, 2, 1, P, 0.25f, fm, d, n, fm, im, dm) == OFLK_ERR_INVALID);   // float32 frames off a 4-byte boundary
    auto sequence = [&](const void *f, int T, int L, int it, int model) {
        return oflk_align_sequence(f, 1, T, 32, 40, L, it, model, 0.25f, fm, nullptr, d, n, fm, im, dm, nullptr);
    };
    EXPECT(sequence(d, 1, 2, 1, P) == OFLK_ERR_INVALID);
    EXPECT(sequence(nullptr, 3, 2, 1, P) == OFLK_ERR_INVALID);
    EXPECT(sequence(d, 3, 2, 0, A) == OFLK_ERR_INVALID);
    EXPECT(sequence(d, 3, 2, 1, 9) == OFLK_ERR_INVALID);
    EXPECT(sequence(d, 3, 4, 1, A) == OFLK_ERR_UNSUPPORTED);
    // the host forms refuse the same before they look for a device
    const unsigned char *u = g_buf;
    EXPECT(oflk_align_refine_host(fm, fm, 0, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host(fm, fm, 1, 32, 40, 2, 0, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host(fm, fm, 1, 32, 40, 2, 1, P, 2.0f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host(fm, fm, 1, 32, 40, 4, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_UNSUPPORTED);
    EXPECT(oflk_align_refine_host(nullptr, fm, 1, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host(fm, nullptr, 1, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host_u8(u, u, 1, 32, 40, 2, 1, 3, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host_u8(u, u, 1, 32, 40, 2, 1, A, 0.25f, nullptr, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host_u8(u, u, 1, 32, 40, 2, 1, A, 0.25f, fm, nullptr, nullptr, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host_u8(u, u, 1, 32, 40, 2, 1, A, 0.25f, fm, nullptr, fm, nullptr, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_host_u8(u, u, 1, 32, 40, 2, 1, A, 0.25f, fm, nullptr, fm, im, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_host(fm, 1, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_host(nullptr, 2, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_host_u8(u, 2, 32, 40, 2, -3, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_host_u8(u, 2, 6, 40, 1, 1, P, 0.25f, fm, nullptr, fm, im, dm) == OFLK_ERR_UNSUPPORTED);
    // the photometric forms: a larger workspace with the steps' (g, b) behind everything else, the plain refusals, and a NULL
    // or misaligned photo output
    for (int model : {A, P}) {
        size_t plain = 0, photo = 0;
        EXPECT(oflk_align_workspace(3, 70, 257, 3, model, &plain) == OFLK_OK);
        EXPECT(oflk_align_photo_workspace(3, 70, 257, 3, model, &photo) == OFLK_OK && photo > plain && photo % 256 == 0);
        int dims[2 * OFLK_MAX_LEVELS];
        AlignConfig cfg{3, 1, model, 0.25f, true, false, 0.0f};
        AlignIo io{};
        EXPECT(check_align(3, 70, 257, cfg, io, dims) == OFLK_OK);
        char *b = reinterpret_cast<char *>(g_buf);
        const AlignWs ws = align_ws(b, 3, dims, cfg);
        EXPECT(ws.bytes == photo && ws.pstride == 3u * 5u * (size_t)align_sums(model == P ? 10 : 8));
        EXPECT(reinterpret_cast<const char *>(ws.photo) >= reinterpret_cast<const char *>(ws.pyr[1]) && aligned(ws.photo, 256));
        EXPECT(reinterpret_cast<const char *>(ws.photo) + 2 * 3 * sizeof(double) <= b + ws.bytes);
        cfg.photo = false;
        EXPECT(align_ws(b, 3, dims, cfg).photo == nullptr);
    }
    EXPECT(oflk_align_photo_workspace(2, 32, 40, 2, P, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_photo_workspace(2, 32, 40, 2, P, &n) == OFLK_OK);
    auto photo = [&](const void *a, int S, int it, void *ws, size_t bytes, float *mo, float *po) {
        return oflk_align_refine_photo(a, d, 0, S, 32, 40, 2, it, P, 0.25f, fm, nullptr, ws, bytes, mo, im, dm, po, nullptr);
    };
    EXPECT(photo(d, 0, 1, d, n, fm, fm) == OFLK_ERR_INVALID);
    EXPECT(photo(d, 2, 0, d, n, fm, fm) == OFLK_ERR_INVALID);
    EXPECT(photo(nullptr, 2, 1, d, n, fm, fm) == OFLK_ERR_INVALID);
    EXPECT(photo(d, 2, 1, d, n, nullptr, fm) == OFLK_ERR_INVALID);
    EXPECT(photo(d, 2, 1, d, n - 1, fm, fm) == OFLK_ERR_INVALID);
    EXPECT(photo(d, 2, 1, d, n, fm, nullptr) == OFLK_ERR_INVALID);
    EXPECT(std::string(oflk_last_error()).find("d_photo_out") != std::string::npos);
    EXPECT(photo(d, 2, 1, d, n, fm, reinterpret_cast<float *>(g_buf + 2)) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_photo(d, 1, 1, 32, 40, 2, 1, P, 0.25f, fm, nullptr, d, n, fm, im, dm, fm, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_photo(d, 1, 3, 32, 40, 2, 1, P, 0.25f, fm, nullptr, d, n, fm, im, dm, nullptr, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_photo_host(fm, fm, 1, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_refine_photo_host_u8(u, u, 1, 32, 40, 2, 0, A, 0.25f, fm, nullptr, fm, im, dm, fm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_photo_host(fm, 1, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm, fm) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_sequence_photo_host_u8(u, 2, 32, 40, 2, 1, P, 0.25f, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
    // the robust forms: two more sums per tile and the first pass's two values behind everything else, the base forms' refusals,
    // a delta that is not finite and positive, photometric without its output; the weight map's refusals
    for (int model : {A, P})
        for (int ph : {0, 1}) {
            size_t base = 0, robust = 0;
            EXPECT((ph ? oflk_align_photo_workspace(3, 70, 257, 3, model, &base) : oflk_align_workspace(3, 70, 257, 3, model, &base)) == OFLK_OK);
            EXPECT(oflk_align_robust_workspace(3, 70, 257, 3, model, ph, &robust) == OFLK_OK && robust > base && robust % 256 == 0);
            int dims[2 * OFLK_MAX_LEVELS];
            AlignConfig cfg{3, 1, model, 0.25f, ph != 0, true, 4.0f};
            AlignIo io{};
            EXPECT(check_align(3, 70, 257, cfg, io, dims) == OFLK_OK);
            char *b = reinterpret_cast<char *>(g_buf);
            const AlignWs ws = align_ws(b, 3, dims, cfg);
            const size_t ns = (size_t)align_sums((model == P ? 8 : 6) + (ph ? 2 : 0)) + 2;
            EXPECT(ws.bytes == robust && ws.pstride == 3u * 5u * ns && align_nsums(model, ph != 0, true) == (int)ns);
            EXPECT(ns == (size_t)(model == P ? (ph ? 69 : 48) : (ph ? 48 : 31)));
            EXPECT((ws.photo != nullptr) == (ph != 0));
            EXPECT(reinterpret_cast<const char *>(ws.first) >= reinterpret_cast<const char *>(ws.pyr[1]) && aligned(ws.first, 256));
            EXPECT(!ph || reinterpret_cast<const char *>(ws.first) >= reinterpret_cast<const char *>(ws.photo) + 2 * 3 * sizeof(double));
            EXPECT(reinterpret_cast<const char *>(ws.first) + 2 * 3 * sizeof(double) <= b + ws.bytes);
            cfg.robust = false;
            EXPECT(align_ws(b, 3, dims, cfg).first == nullptr);
        }
    EXPECT(oflk_align_robust_workspace(2, 32, 40, 2, P, 0, nullptr) == OFLK_ERR_INVALID);
    EXPECT(oflk_align_robust_workspace(0, 32, 40, 2, P, 0, &n) == OFLK_ERR_INVALID && n == 0);
    EXPECT(oflk_align_robust_workspace(2, 32, 40, 4, P, 1, &n) == OFLK_ERR_UNSUPPORTED);
    {
        const float inf = std::numeric_limits<float>::infinity();
        size_t np = 0;
        EXPECT(oflk_align_robust_workspace(2, 32, 40, 2, P, 0, &n) == OFLK_OK && oflk_align_robust_workspace(2, 32, 40, 2, P, 1, &np) == OFLK_OK);
        auto robust = [&](const void *a, int S, int it, float delta, int ph, void *ws, size_t bytes, float *mo, float *po) {
            return oflk_align_refine_robust(a, d, 0, S, 32, 40, 2, it, P, 0.25f, delta, ph, fm, nullptr, ws, bytes, mo, im, dm, po, nullptr);
        };
        for (float delta : {0.0f, -4.0f, nan, inf, -inf}) {
            EXPECT(robust(d, 2, 1, delta, 0, d, n, fm, nullptr) == OFLK_ERR_INVALID);
            EXPECT(std::string(oflk_last_error()).find("robust_delta") != std::string::npos);
            EXPECT(robust(d, 2, 1, delta, 1, d, np, fm, fm) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_sequence_robust(d, 1, 3, 32, 40, 2, 1, P, 0.25f, delta, 0, fm, nullptr, d, n, fm, im, dm, nullptr, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_refine_robust_host(fm, fm, 1, 32, 40, 2, 1, P, 0.25f, delta, 0, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_refine_robust_host_u8(u, u, 1, 32, 40, 2, 1, A, 0.25f, delta, 1, fm, nullptr, fm, im, dm, fm) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_sequence_robust_host(fm, 2, 32, 40, 2, 1, P, 0.25f, delta, 0, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_sequence_robust_host_u8(u, 2, 32, 40, 2, 1, P, 0.25f, delta, 0, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_weights(d, d, 0, 2, 32, 40, P, delta, fm, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_weights_host(fm, fm, 2, 32, 40, P, delta, fm, nullptr, fm) == OFLK_ERR_INVALID);
            EXPECT(oflk_align_weights_host_u8(u, u, 2, 32, 40, A, delta, fm, fm, fm) == OFLK_ERR_INVALID);
        }
        EXPECT(robust(d, 0, 1, 4.0f, 0, d, n, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(robust(d, 2, 0, 4.0f, 0, d, n, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(robust(nullptr, 2, 1, 4.0f, 0, d, n, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(robust(d, 2, 1, 4.0f, 0, d, n, nullptr, nullptr) == OFLK_ERR_INVALID);
        EXPECT(robust(d, 2, 1, 4.0f, 0, d, n - 1, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(robust(d, 2, 1, 4.0f, 1, d, np - 1, fm, fm) == OFLK_ERR_INVALID);
        EXPECT(robust(d, 2, 1, 4.0f, 1, d, np, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(std::string(oflk_last_error()).find("d_photo_out") != std::string::npos);
        EXPECT(robust(d, 2, 1, 4.0f, 1, d, np, fm, reinterpret_cast<float *>(g_buf + 2)) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_sequence_robust(d, 1, 1, 32, 40, 2, 1, P, 0.25f, 4.0f, 0, fm, nullptr, d, n, fm, im, dm, nullptr, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_sequence_robust(d, 1, 3, 32, 40, 2, 1, P, 0.25f, 4.0f, 1, fm, nullptr, d, np, fm, im, dm, nullptr, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_refine_robust_host(fm, fm, 1, 32, 40, 2, 1, P, 0.25f, 4.0f, 1, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_refine_robust_host(fm, fm, 0, 32, 40, 2, 1, P, 0.25f, 4.0f, 0, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_sequence_robust_host_u8(u, 1, 32, 40, 2, 1, P, 0.25f, 4.0f, 0, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_sequence_robust_host(fm, 2, 32, 40, 4, 1, P, 0.25f, 4.0f, 0, fm, nullptr, fm, im, dm, nullptr) == OFLK_ERR_UNSUPPORTED);
        EXPECT(oflk_align_weights(d, d, 0, 0, 32, 40, P, 4.0f, fm, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(d, d, 0, 2, 0, 40, P, 4.0f, fm, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(d, d, 0, 2, 32, 40, 2, 4.0f, fm, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(nullptr, d, 0, 2, 32, 40, P, 4.0f, fm, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(d, d, 0, 2, 32, 40, P, 4.0f, nullptr, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(d, d, 0, 2, 32, 40, P, 4.0f, fm, nullptr, nullptr, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(g_buf + 1, d, 0, 2, 32, 40, P, 4.0f, fm, nullptr, fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(d, d, 1, 2, 32, 40, P, 4.0f, fm, reinterpret_cast<float *>(g_buf + 2), fm, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights(d, d, 0, 2, 1 << 15, 1 << 15, P, 4.0f, fm, nullptr, fm, nullptr) == OFLK_ERR_UNSUPPORTED);
        EXPECT(oflk_align_weights_host(nullptr, fm, 2, 32, 40, P, 4.0f, fm, nullptr, fm) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights_host(fm, fm, 2, 32, 40, P, 4.0f, fm, nullptr, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_align_weights_host_u8(u, u, 0, 32, 40, P, 4.0f, fm, nullptr, fm) == OFLK_ERR_INVALID);
    }
    // the exposure chain is host code: its refusals, a held step, and forwards against backwards
    {
        const float ph[3][2] = {{2.0f, 4.0f}, {-1.0f, 7.0f}, {0.5f, -1.0f}};
        const int st[3] = {1, 1, 1};
        double e[4][2];
        EXPECT(oflk_exposure_chain_host(&ph[0][0], st, 0, 0, &e[0][0]) == OFLK_ERR_INVALID);
        EXPECT(oflk_exposure_chain_host(&ph[0][0], st, 4, 4, &e[0][0]) == OFLK_ERR_INVALID);
        EXPECT(oflk_exposure_chain_host(nullptr, st, 4, 0, &e[0][0]) == OFLK_ERR_INVALID);
        EXPECT(oflk_exposure_chain_host(&ph[0][0], st, 4, 0, nullptr) == OFLK_ERR_INVALID);
        EXPECT(oflk_exposure_chain_host(nullptr, nullptr, 1, 0, &e[0][0]) == OFLK_OK && e[0][0] == 1.0 && e[0][1] == 0.0);
        EXPECT(oflk_exposure_chain_host(&ph[0][0], nullptr, 4, 0, &e[0][0]) == OFLK_OK);
        EXPECT(e[0][0] == 1.0 && e[0][1] == 0.0 && e[1][0] == 0.5 && e[1][1] == -2.0);
        EXPECT(e[2][0] == 0.5 && e[2][1] == -2.0);   // the step with a negative gain is held
        EXPECT(e[3][0] == 1.0 && e[3][1] == -1.0);
        EXPECT(oflk_exposure_chain_host(&ph[0][0], nullptr, 4, 3, &e[0][0]) == OFLK_OK);
        EXPECT(e[3][0] == 1.0 && e[3][1] == 0.0 && e[2][0] == 0.5 && e[2][1] == -1.0 && e[1][0] == 0.5 && e[0][0] == 1.0 && e[0][1] == 1.0);
    }
    std::printf(g_failed ? "align host check: %d expectation(s) failed\n" : "align host check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
