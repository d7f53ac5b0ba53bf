/*
 * oflk.h -- C ABI of liboflk.so: dense Lucas-Kanade optical flow on MI355X (gfx950).
 *
 * This is the drop-in boundary for the hot path of rothej/optical-flow-fpga's
 * Python golden model.  The reference has no FFI of its own: its "interface" is
 * a set of plain Python functions in python/lucas_kanade_core.py and
 * python/lucas_kanade_pyramidal.py, imported by name by the verifier
 * (python/optical_flow_verifier.py:19-20) and the demo CLIs.  Each entry point
 * below cites the reference function it replaces; the Python shims in
 * optical-flow-fpga_amd/python/ (same module and function names as the
 * reference) bind them with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.
 *   - Images and flow fields are C-contiguous row-major float32 [H][W]
 *     (batched: [B][H][W]).
 *   - Every function returns OFLK_OK (0) or a negative OFLK_ERR_* code;
 *     oflk_last_error() returns a human-readable message for the calling thread.
 *   - There is NO CPU fallback: every compute entry point runs hand-written HIP
 *     kernels and fails with OFLK_ERR_NO_DEVICE when no gfx950 GPU is usable.
 *   - Frames are at most 2^23 - 1 (8 388 607) rows and columns and fewer than 2^30 pixels (plans: 2^29): the kernels form
 *     row offsets with the signed 24-bit multiply and byte offsets in 32 bits.  Anything larger is refused with
 *     OFLK_ERR_UNSUPPORTED before any device call.
 *   - "host" entry points take host pointers and are synchronous (H2D, kernels,
 *     D2H inside the call).  "plan" entry points take device pointers, enqueue
 *     on a caller-supplied hipStream_t and return without synchronising.
 */
#ifndef OFLK_H
#define OFLK_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFLK_OK 0
#define OFLK_ERR_INVALID (-1)     /* bad argument (null pointer, non-positive size, ...) */
#define OFLK_ERR_NO_DEVICE (-2)   /* no usable HIP device / HIP runtime error at init */
#define OFLK_ERR_HIP (-3)         /* a HIP runtime call failed (message has details) */
#define OFLK_ERR_UNSUPPORTED (-4) /* parameter outside what the kernels are built for */
#define OFLK_ERR_NOMEM (-5)       /* device or host allocation failed */

#define OFLK_MAX_LEVELS 16
#define OFLK_MAX_WINDOW 45 /* largest window_size (45 x 45 = 2025 products; even sizes round down like the reference) */
#define OFLK_MAX_TILED_WINDOW 11 /* 3x3 ... 11x11 run the tiled kernels; every other size the generic one-thread-per-pixel kernel */

/* ---- library ------------------------------------------------------------ */
const char *oflk_version(void);
/* number of visible HIP devices; 0 when there is none (never fails) */
int oflk_device_count(void);
/* message of the last error raised on the calling thread ("" if none) */
const char *oflk_last_error(void);
/* device used by the host entry points (default 0).  Each device has its own plan cache and
 * staging buffers; calls on different devices (from different host threads) run concurrently. */
int oflk_set_device(int device);

/* ---- host-pointer entry points: one per reference function ---------------- */

/* compute_gradients(frame_prev, frame_curr) -> (Ix, Iy, It)
 * replaces python/lucas_kanade_core.py:15-45 */
int oflk_compute_gradients(const float *prev, const float *curr, int H, int W, float *Ix,
                           float *Iy, float *It);

/* lucas_kanade_from_gradients(Ix, Iy, It, window_size) -> (u, v)
 * replaces python/lucas_kanade_core.py:73-135 */
int oflk_from_gradients(const float *Ix, const float *Iy, const float *It, int H, int W,
                        int window_size, float *u, float *v);

/* lucas_kanade_single_scale(frame_prev, frame_curr, window_size) -> (u, v)
 * replaces python/lucas_kanade_core.py:48-70 (one fused kernel) */
int oflk_single_scale(const float *prev, const float *curr, int H, int W, int window_size,
                      float *u, float *v);

/* level sizes of build_gaussian_pyramid: dims_out[2*l] = H_l, dims_out[2*l+1] = W_l,
 * l = 0 is the coarsest level (python/lucas_kanade_pyramidal.py:51-52, :61) */
int oflk_pyramid_level_dims(int H, int W, int levels, double scale_factor, int *dims_out);

/* build_gaussian_pyramid(image, num_levels, scale_factor) -> [coarse .. fine]
 * replaces python/lucas_kanade_pyramidal.py:23-63; out_levels[l] must hold H_l*W_l floats.
 * Any scale_factor in (0, 1] whose Gaussian radius int(4 / scale_factor + 0.5) is at most 64 (scale_factor >= about 0.063).
 * A step runs the fused kernel (k_pyr_down: blur and resampling in one launch, the blurred tile in LDS) when the radius is 8,
 * i.e. scale_factor in (8/17, 8/15], and every 32 x 16 output tile's source span fits the 66 x 34 LDS tile: always at 0.5,
 * at some sizes elsewhere in that band.  Every other step runs the unfused chain (k_blur along y, k_blur along x,
 * k_resample) with the same operations in the same order.  oflk_pyramid_step_fused tells which. */
int oflk_build_pyramid(const float *image, int H, int W, int levels, double scale_factor,
                       float *const *out_levels);

/* The same with the Gaussian weights given by the caller: weights[k], k = 0 .. radius, is the normalised weight at distance k
 * of scipy.ndimage.gaussian_filter's kernel for sigma = 1 / scale_factor (radius = int(4 sigma + 0.5)).  SciPy forms them with
 * NumPy's exp, whose last bit differs from libm's for some arguments; oflk_build_pyramid embeds SciPy's table for the
 * reference's default scale_factor 0.5 and falls back to libm elsewhere.  The Python shim computes the weights with NumPy the
 * way SciPy does (lucas_kanade_pyramidal.build_gaussian_pyramid) and calls this entry point, so EVERY scale factor gives the
 * reference's pyramid (tests/golden/pyramid_scales*.npz, made by importing the reference). */
int oflk_build_pyramid_w(const float *image, int H, int W, int levels, double scale_factor, const double *weights,
                         int radius, float *const *out_levels);

/* warp_image(image, flow_u, flow_v) -> warped
 * replaces python/lucas_kanade_pyramidal.py:66-97 */
int oflk_warp(const float *image, const float *flow_u, const float *flow_v, int H, int W,
              float *out);

/* upsample_flow(flow_u, flow_v, (Ht, Wt)) -> (u, v)
 * replaces python/lucas_kanade_pyramidal.py:100-138.  Any coarse and target shape, shrinking included.  The staged kernel
 * (k_upsample: the coarse cells of a 256 x 16 output block in LDS) serves every target whose blocks each span at most 136
 * coarse columns and 10 coarse rows: every ratio of about 1.9 or more per axis (ratio 2 at every size), and any ratio on a
 * coarse field of at most 10 x 136.  Smaller ratios, equal shapes and shrinking targets on larger fields run the gathering
 * kernel (k_resample) with the same arithmetic.  oflk_upsample_staged tells which. */
int oflk_upsample_flow(const float *flow_u, const float *flow_v, int Hc, int Wc, int Ht, int Wt,
                       float *u_out, float *v_out);

/* Which kernel a stage call runs: host-only, never fail (0 for sizes below 1), usable without a GPU.  They evaluate the
 * launchers' own decisions, so that a test can name the kernel it compares.
 * oflk_upsample_staged: 1 when oflk_upsample_flow (and the flow upsampling of a pyramidal pass) of Hc x Wc to Ht x Wt runs
 * k_upsample, 0 when it runs k_resample.
 * oflk_pyramid_step_fused: 1 when the pyramid step from h x w to ho x wo with a Gaussian of this radius runs k_pyr_down, 0
 * when it runs the unfused chain (always 0 for a radius other than 8).
 * oflk_pyramid_step_form: which of the three paths that step takes.  2: k_pyr_down's tight tile (every 32 x 16 output tile
 * samples at most 32 x 64 blurred values: the half-scale ratio, every level of an even-sized frame), 1: its general tile
 * (at most 34 x 66: odd sizes, tiny levels), 0: the unfused chain.  Nonzero exactly when oflk_pyramid_step_fused is 1.
 * oflk_pyramid_step_half: 1 when that step runs the tight tile's half-scale instantiation (tap and staging offsets fixed at
 * compile time): oflk_pyramid_step_form is 2, ho and wo are at least 2, and on both axes floor(i * step) == 2 i for every
 * output i but the last, step being np.linspace(0, S - 1, T)'s.  Every level of an even-sized frame at scale factor 0.5; 0
 * for a tight step at another ratio of the band, which runs the tight tile as before.  Same values either way. */
int oflk_upsample_staged(int Hc, int Wc, int Ht, int Wt);
int oflk_pyramid_step_fused(int h, int w, int ho, int wo, int radius);
int oflk_pyramid_step_form(int h, int w, int ho, int wo, int radius);
int oflk_pyramid_step_half(int h, int w, int ho, int wo, int radius);

/* lucas_kanade_pyramidal(frame_prev, frame_curr, num_levels, window_size, num_iterations) -> (u, v)
 * replaces python/lucas_kanade_pyramidal.py:141-228.
 *   residual_log : [levels][iters][2] floats, mean|du|, mean|dv| of each executed
 *                  iteration (what the reference prints at :215-218); may be NULL
 *   iters_run    : [levels] ints, iterations executed per level (early exit at
 *                  :221-223); may be NULL */
int oflk_pyramidal(const float *prev, const float *curr, int H, int W, int levels,
                   int window_size, int iters, float *u, float *v, float *residual_log,
                   int *iters_run);

/* B independent frame pairs in one call; arrays are [B][H][W], residual_log is
 * [B][levels][iters][2], iters_run is [B][levels] (both may be NULL). */
int oflk_single_scale_batch(const float *prev, const float *curr, int B, int H, int W,
                            int window_size, float *u, float *v);
int oflk_pyramidal_batch(const float *prev, const float *curr, int B, int H, int W, int levels,
                         int window_size, int iters, float *u, float *v, float *residual_log,
                         int *iters_run);

/* The two reads above for the host entry points: they address the plan the last oflk_pyramidal* call
 * of this shape left in the current device's cache (OFLK_ERR_INVALID if there is none). */
int oflk_pyramidal_last_level_flow(int B, int H, int W, int levels, int window_size, int iters, int level,
                                   int pair, float *u, float *v);
int oflk_pyramidal_last_uncertain(int B, int H, int W, int levels, int window_size, int iters, int *uncertain);

/* ---- uint8 frames (the reference's on-disk format) ------------------------- */
/* Same as the batch entry points, for raw 8-bit frames [B][H][W] as generate_test_suite.py
 * writes them (frame_0x.bin, :259-261).  The kernels read the bytes themselves (2 B/px of frame
 * traffic instead of 8; no float32 copy of the frames exists on the device): the uint8 -> float32
 * conversion the verifier does on the host (python/optical_flow_verifier.py:61-65) happens in
 * registers and is exact, so results are identical to converting first. */
int oflk_single_scale_u8(const unsigned char *prev, const unsigned char *curr, int B, int H, int W,
                         int window_size, float *u, float *v);
int oflk_pyramidal_u8(const unsigned char *prev, const unsigned char *curr, int B, int H, int W,
                      int levels, int window_size, int iters, float *u, float *v, float *residual_log,
                      int *iters_run);
/* device-side conversion for pipelines that hold uint8 frames in HBM: d_out[i] = (float)d_in[i] */
int oflk_u8_to_f32(const unsigned char *d_in, float *d_out, size_t n, void *stream);

/* ---- reduced precision (BASELINE config 5), opt-in, never the default ------------ */
/* lucas_kanade_single_scale with fp16 gradients and fp16 window accumulators: float32 frames in,
 * float32 flow out, everything between the frame average and the 2x2 solve in half precision, window
 * sums separable.  This is NOT the reference's arithmetic (python/lucas_kanade_core.py:110-133 is fp32
 * throughout): results are close to, not equal to, oflk_single_scale_batch -- how close is measured,
 * per pattern, by tests/test_gpu_fp16.py (mean / median endpoint error against the exact path).
 *   pixel_max : upper bound of the frame values (255 for the reference's 8-bit frames); frames are
 *               scaled by a power of two so that a window sum of Ix^2 stays below fp16's 65504.
 *               Values beyond [0, pixel_max] may overflow to inf / nan. */
int oflk_single_scale_fp16(const float *prev, const float *curr, int B, int H, int W, int window_size,
                           float pixel_max, float *u, float *v);

/* ---- one process, several GPUs ------------------------------------------------- */
/* Frame pairs are independent units (python/lucas_kanade_pyramidal.py:141-228 touches only its two
 * inputs), so a batch spreads over GPUs with no data-path exchange.  How long a pair takes depends on its
 * data (the early exit of :221-223), so devices do not get fixed shards: the B pairs are cut into chunks of
 * consecutive pairs (about four per device) and each device -- a host thread of its own, its own plans --
 * pulls the next chunk from a shared counter until none is left; every chunk is written to its slice of
 * the host output arrays.  n_gpus <= 0 means all visible devices; n_gpus > visible devices is
 * OFLK_ERR_INVALID; with n_gpus == 1 the call is oflk_*_batch on the device of oflk_set_device.  Results
 * do not depend on n_gpus, nor on which device took which chunk.
 * (The multi-process form -- one rank per GPU, torch.distributed over RCCL -- is bench.py's.) */
int oflk_single_scale_batch_multi(const float *prev, const float *curr, int B, int H, int W,
                                  int window_size, int n_gpus, float *u, float *v);
int oflk_pyramidal_batch_multi(const float *prev, const float *curr, int B, int H, int W, int levels,
                               int window_size, int iters, int n_gpus, float *u, float *v,
                               float *residual_log, int *iters_run);
int oflk_pyramidal_u8_multi(const unsigned char *prev, const unsigned char *curr, int B, int H, int W,
                            int levels, int window_size, int iters, int n_gpus, float *u, float *v,
                            float *residual_log, int *iters_run);
/* ---- frame sequences (video) ---------------------------------------------------- */
/* T frames [T][H][W] in, the T-1 flows (t -> t+1) out: u, v are [T-1][H][W], residual_log [T-1][levels][iters][2] and
 * iters_run [T-1][levels] (both may be NULL) -- exactly what oflk_pyramidal_batch returns for the T-1 pairs
 * (frames[t], frames[t+1]), value for value, iteration counts and oflk_last_resolved() included.  Each frame is uploaded
 * once (a large call goes in chunks of C pairs, whose C+1 frames share the boundary frame with the next chunk) and its
 * Gaussian pyramid is built once, not once as curr and again as prev.  T < 2 is OFLK_ERR_INVALID.  The _multi form is
 * the chunk queue of oflk_pyramidal_batch_multi over the T-1 pairs (a chunk of pairs [b0, b1) reads frames [b0, b1]).
 * oflk_single_scale_sequence has no pyramid to share: it halves the upload, and keeps the two APIs alike. */
int oflk_pyramidal_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                            float *u, float *v, float *residual_log, int *iters_run);
int oflk_pyramidal_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                               float *u, float *v, float *residual_log, int *iters_run);
int oflk_pyramidal_sequence_multi(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                  int n_gpus, float *u, float *v, float *residual_log, int *iters_run);
int oflk_single_scale_sequence(const float *frames, int T, int H, int W, int window_size, float *u, float *v);

/* ---- forward-backward flow of frame sequences ---------------------------------- */
/* Both directions of every consecutive pair and their consistency: uf, vf [T-1][H][W] are the forward flows (frames t ->
 * t+1, oflk_pyramidal_sequence's values), ub, vb the backward flows (frames t+1 -> t, the values oflk_pyramidal_sequence
 * gives flow T-2-t on the reversed frames), all four required.  err_f / valid_f (forward, on frame t's grid) and err_b /
 * valid_b (backward, on frame t+1's grid) are oflk_fb_consistency's outputs with alpha, beta; each may be NULL (all four
 * NULL skips the check).  Flagged pairs of both directions are resolved (oflk_last_resolved() counts both), and
 * oflk_set_host_arithmetic applies.  Each frame is uploaded once and its pyramid built once for both directions.  A
 * large call goes in chunks of C pairs (C+1 frames, the boundary frame shared with the next chunk) one after the other,
 * without the PCIe overlap of oflk_pyramidal_sequence; results do not depend on the cut.  T < 2, NULL flows, alpha or beta
 * negative or not finite: OFLK_ERR_INVALID. */
int oflk_pyramidal_sequence_fb(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                               float alpha, float beta, float *uf, float *vf, float *ub, float *vb, float *err_f,
                               float *err_b, unsigned char *valid_f, unsigned char *valid_b);
int oflk_pyramidal_sequence_fb_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                  float alpha, float beta, float *uf, float *vf, float *ub, float *vb, float *err_f,
                                  float *err_b, unsigned char *valid_f, unsigned char *valid_b);
/* oflk_fb_consistency (below) on host arrays [B][H][W] (synchronous) */
int oflk_fb_consistency_host(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W,
                             float alpha, float beta, float *err_f, float *err_b, unsigned char *valid_f,
                             unsigned char *valid_b);

/* ---- point tracks through frame sequences ------------------------------------------------------------------------- */
/* Frames in, tracks out: run_sequence_fb's chunk loop (the bidirectional plan pass, flagged pairs of both directions
 * resolved), then one oflk_track_points launch per chunk that continues from the previous chunk's last row.  No flow and
 * no mask leaves the device: tracks [T][N][2] (x, y) and visible [T][N] (0 / 1) are the rows of frames 0 .. T-1 of
 * oflk_track_points (below) on the sequence's flows.  Queries: qt [N] frame indices (NULL: every query at frame 0), qxy
 * [N][2] (x, y).  oflk_set_host_arithmetic applies to the flows and oflk_last_resolved() counts the pairs redone; the
 * tracking arithmetic has one mode only.  T < 2, N < 1, a NULL qxy / tracks / visible, a query frame outside [0, T-1],
 * alpha or beta negative or not finite: OFLK_ERR_INVALID, before any device call. */
int oflk_pyramidal_sequence_tracks(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                   float alpha, float beta, const int *qt, const float *qxy, int N, float *tracks,
                                   unsigned char *visible);
int oflk_pyramidal_sequence_tracks_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                      float alpha, float beta, const int *qt, const float *qxy, int N, float *tracks,
                                      unsigned char *visible);
/* oflk_track_points (below) on host flows of a whole sequence (T = B+1 frames, t0 = 0; synchronous): tracks [B+1][N][2],
 * visible [B+1][N].  Checks as oflk_pyramidal_sequence_tracks, and the flows' as oflk_fb_consistency_host. */
int oflk_track_points_host(const float *uf, const float *vf, const float *ub, const float *vb, int B, int H, int W,
                           float alpha, float beta, const int *qt, const float *qxy, int N, float *tracks,
                           unsigned char *visible);

/* ---- motion-compensated frame interpolation on the dense flows ----------------------------------------------------- */
/* Frames in, in-between frames out: the statement (tests/interp_model.py).  Pair b has frames A = frame b and B = frame
 * b+1, each float32 or uint8, F = (uf, vf) the flow A -> B and G = (ub, vb) the flow B -> A.  The output time tau is a
 * double in the open interval (0, 1).  sample(img, x, y) is the reference's warp_image at one float64 point (map_coordinates,
 * order 1, cval 0; float32 result); a coordinate that is not inside [0, W-1] x [0, H-1] -- the negated closed comparison in
 * float64, so NaN and the infinities are not inside -- samples as 0 and reads no tap: a flow value never becomes an
 * address.  Every float32 and float64 operation is rounded on its own.  For output pixel (x, y), R = refine >= 1:
 *   side(img, F, G, s):                       s = f64(tau) for the A side, 1.0 - f64(tau) (one subtraction) for the B side
 *     px = f64(x); py = f64(y)
 *     repeat R times:                         the fixed-point solve of p + s F(p) = (x, y): gathers only, no scatter
 *       us = sample(F.u, px, py); vs = sample(F.v, px, py)
 *       px = f64(x) - s * f64(us); py = f64(y) - s * f64(vs)            product, then subtraction
 *     us = sample(F.u, px, py); vs = sample(F.v, px, py)                the flow at the solved point
 *     qx = px + f64(us); qy = py + f64(vs)                              where that point lies in the other frame
 *     bu = sample(G.u, qx, qy); bv = sample(G.v, qx, qy)
 *     eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
 *     ok = inside(px, py) and inside(qx, qy) and e2 <= f32(alpha)*m2 + f32(beta)
 *     return sample(img, px, py), ok          uint8 frames: the taps converted to float32 first, as the warps do
 *   a, ok_a = side(A, F, G, tau);  b, ok_b = side(B, G, F, 1 - tau);  t = f32(tau)
 *   both: out = a + t*(b - a);  only ok_a: out = a;  only ok_b: out = b;  neither: out = A[y][x] + t*(B[y][x] - A[y][x])
 *   status = ok_a | (ok_b << 1)               3, 1, 2, 0: a byte per output pixel
 *   uint8 frames: (unsigned char)rintf(out), half to even;  float32 frames: out
 * These are grey planes (packed colour and NV12: below); no splatting and no occlusion ordering beyond the forward-backward
 * test; the flows are taken as they are.
 *
 * oflk_interpolate_sequence{,_u8}: T frames [T][H][W] in, the (T-1) * n new frames out [T-1][n][H][W] (the frames' type), time
 * taus[j] of pair t at out[t][j], and status [T-1][n][H][W] (may be NULL).  oflk_pyramidal_sequence_fb's chunk loop (the
 * bidirectional plan pass, flagged pairs of both directions resolved, oflk_last_resolved() counts them,
 * oflk_set_host_arithmetic applies to the flows), then one interpolation launch per chunk: only out and status come down, no
 * flow leaves the device.  It equals oflk_pyramidal_sequence_fb followed by oflk_interpolate_frames_host on those flows, byte
 * for byte.  Refused before any device call: whatever oflk_pyramidal_sequence_fb refuses, with its codes; and, all
 * OFLK_ERR_INVALID, n < 1 or n > OFLK_INTERP_MAX_TAUS, a tau that is not finite or not strictly between 0 and 1, refine
 * outside [1, 8], alpha or beta negative or not finite, NULL taus or out, out overlapping the frames.
 * oflk_interpolate_frames_host{,_u8}: oflk_interpolate_frames (below) on host arrays -- frames [B+1][H][W], flows [B][H][W],
 * out and status (may be NULL) [B][n][H][W] -- synchronous; its refusals, NULL flows included. */
#define OFLK_INTERP_MAX_TAUS 16
int oflk_interpolate_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                              float beta, int refine, const double *taus, int n, float *out, unsigned char *status);
int oflk_interpolate_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                 float alpha, float beta, int refine, const double *taus, int n, unsigned char *out,
                                 unsigned char *status);
int oflk_interpolate_frames_host(const float *frames, int B, int H, int W, const float *uf, const float *vf, const float *ub,
                                 const float *vb, float alpha, float beta, int refine, const double *taus, int n, float *out,
                                 unsigned char *status);
int oflk_interpolate_frames_host_u8(const unsigned char *frames, int B, int H, int W, const float *uf, const float *vf,
                                    const float *ub, const float *vb, float alpha, float beta, int refine, const double *taus,
                                    int n, unsigned char *out, unsigned char *status);

/* Interpolation of colour and NV12 video: the statement (tests/interp_colour_model.py) on top of the grey one above, whose
 * side, sample, inside, status cases and rintf these are.  One solve per output position serves every channel.
 *
 * Packed colour: frames uint8 [B+1][H][W][C], C = 3 or 4, the flows [B][H][W] float32 taken as given, out [B][n][H][W][C],
 * status [B][n][H][W].  For every channel c, out[..., c] is the uint8 grey statement on the planes frames[..., c] under these
 * flows, and status is that statement's: ok depends on the flows only, so it is the same for every channel.  A fourth channel
 * is interpolated like the others.
 *
 * NV12: layout, siting and shapes as the NV12 warps' (oflk_nv12_frame_bytes, OFLK_SITING_*, H and W even and >= 4); out
 * [B][n][H W 3 / 2], status [B][n][H][W].  The Y plane of out is the uint8 grey statement on the Y planes (H W 3 / 2 bytes
 * apart) and status is that statement's.  Chroma: CH = H/2, CW = W/2, P_c[f] the CH x CW plane UV[f][:, :, c], c in {U, V};
 * the siting gives sx in {0, 0.5} and sy = 0.5.  Output chroma sample (column i, row j) sits at the luma position
 * X = f64(2 i) + sx, Y = f64(2 j) + sy, both exact, and runs the grey side's solve with (f64(x), f64(y)) replaced by (X, Y):
 * the same flows, R, forward-backward test and inside tests against the H x W luma frame.  That gives (px, py) and ok of the A
 * side (s = f64(tau)) and of the B side (s = 1.0 - f64(tau)).  A side's value for channel c is sample(P_c, cx, cy) with
 *     cx = clamp(0.5 * (px - sx), 0, CW - 1);  cy = clamp(0.5 * (py - sy), 0, CH - 1)        one subtraction, one product, float64
 *     clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v)
 * The clamp: a point inside the luma frame lies up to half a chroma sample beyond the chroma plane's first or last row or
 * column, where the sample's cval 0 would bleed saturated green into the frame's edge.  Where (px, py) is not inside the luma
 * frame ok is 0 and the value is not used (no chroma tap of that point is read).  With t = f32(tau): both sides ok
 * a + t*(b - a); only one its value; neither P_c[A][j][i] + t*(P_c[B][j][i] - P_c[A][j][i]); then (unsigned char)rintf(.).  The
 * chroma positions' ok bits are not returned.
 *
 * oflk_interpolate_sequence_packed: frames [T][H][W][C] in, out [T-1][n][H][W][C] and status [T-1][n][H][W] (may be NULL).  It
 * equals oflk_luma_u8_host(order) on the frames, oflk_pyramidal_sequence_fb_u8 on that luma and
 * oflk_interpolate_frames_packed_host on the colour frames and those flows, byte for byte.  oflk_interpolate_sequence_nv12:
 * frames [T][H W 3 / 2], out [T-1][n][H W 3 / 2]; it equals oflk_pyramidal_sequence_fb_u8 on the Y planes gathered
 * contiguously, then oflk_interpolate_frames_nv12_host.  Both run oflk_interpolate_sequence's chunk loop: a chunk's frames go
 * up once in their own layout, the luma or the Y planes of the flow pass are formed from them on the device, no flow leaves
 * it and only out and status come down; oflk_last_resolved() and oflk_set_host_arithmetic as there.
 * Refused before any device call, in this order: channels other than 3 or 4, an order (sequence call) or a siting that is
 * not one of the constants, H or W odd or below 4 (NV12): OFLK_ERR_INVALID; T < 2 (B < 1); H or W < 2, NULL frames or out:
 * OFLK_ERR_INVALID; 2^30 pixels or more, 2^23 rows or columns or more, packed frames of 2^31 bytes or more:
 * OFLK_ERR_UNSUPPORTED; then what the grey forms refuse, with out overlapping the frames measured in the layout's frame
 * bytes.  The _host forms: oflk_interpolate_frames_packed / _nv12 (below) on host arrays, synchronous. */
int oflk_interpolate_sequence_packed(const unsigned char *frames, int T, int H, int W, int channels, int order, int levels,
                                     int window_size, int iters, float alpha, float beta, int refine, const double *taus,
                                     int n, unsigned char *out, unsigned char *status);
int oflk_interpolate_sequence_nv12(const unsigned char *frames, int T, int H, int W, int siting, int levels, int window_size,
                                   int iters, float alpha, float beta, int refine, const double *taus, int n,
                                   unsigned char *out, unsigned char *status);
int oflk_interpolate_frames_packed_host(const unsigned char *frames, int B, int H, int W, int channels, const float *uf,
                                        const float *vf, const float *ub, const float *vb, float alpha, float beta,
                                        int refine, const double *taus, int n, unsigned char *out, unsigned char *status);
int oflk_interpolate_frames_nv12_host(const unsigned char *frames, int B, int H, int W, int siting, const float *uf,
                                      const float *vf, const float *ub, const float *vb, float alpha, float beta, int refine,
                                      const double *taus, int n, unsigned char *out, unsigned char *status);

/* ---- median filtering of dense flows ------------------------------------------------------------------------------------ */
/* The statement (tests/flow_median_model.py).  A plane p is [H][W] float32, the window size x size with size in {3, 5, 7, 9}.
 * Output pixel (y, x) takes the size^2 values p[clamp(y + j, 0, H-1)][clamp(x + i, 0, W-1)], i and j in -size/2 .. size/2 (the
 * border is replicated), orders them by their bits -- the key of bits b is ~b when the sign bit is set, else b ^ 0x80000000,
 * which gives -NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN, the temporal-median mosaic's order -- and returns
 * the value of rank size^2 / 2.  size^2 is odd, so the result is one of the inputs: nothing is averaged, nothing is rounded,
 * and equal keys are equal bytes, so the selection method cannot show.  Every plane is filtered on its own: of a flow this is
 * the component-wise median of u and of v, not a vector median, and it is one pass (a caller may call twice).
 *
 * oflk_flow_median_host: in and out are host arrays of P contiguous planes [P][H][W]; synchronous.  A large call goes in
 * chunks of min(64, 2^27 / (4 H W)) planes (one at least) through one pair of device buffers; planes are independent, so the
 * result does not depend on the cut.  The device form is oflk_flow_median (below).  Refused before any device call, all
 * OFLK_ERR_INVALID: NULL in or out, P < 1, a size that is not 3, 5, 7 or 9; then H or W < 1: OFLK_ERR_INVALID, 2^30 pixels or
 * more or 2^23 rows or columns or more: OFLK_ERR_UNSUPPORTED; then out overlapping in (the filter is not in place):
 * OFLK_ERR_INVALID.
 *
 * The _median sequence forms are oflk_pyramidal_sequence_fb{,_u8}, oflk_interpolate_sequence{,_u8},
 * oflk_interpolate_sequence_packed and oflk_interpolate_sequence_nv12 with one more setting, flow_median: 0 is that call
 * itself, byte for byte, with no launch and no buffer added; 3, 5, 7 or 9 filters the four flow arrays of every chunk on the
 * device, after the flagged pairs are resolved (oflk_last_resolved() is that call's), through one more [C][H][W] buffer.  The
 * flows that come down from oflk_pyramidal_sequence_fb_median are the filtered ones, and the errors, the masks, the status
 * bytes and the new frames are computed from them: the call equals the unfiltered call's flows put through
 * oflk_flow_median_host and then oflk_fb_consistency_host (oflk_interpolate_frames*_host), byte for byte.  The chunks are the
 * unfiltered call's.  Any other flow_median: OFLK_ERR_INVALID before any device call, beside what the unfiltered call refuses. */
int oflk_flow_median_host(const float *in, float *out, int P, int H, int W, int size);
int oflk_pyramidal_sequence_fb_median(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                      float alpha, float beta, int flow_median, float *uf, float *vf, float *ub, float *vb,
                                      float *err_f, float *err_b, unsigned char *valid_f, unsigned char *valid_b);
int oflk_pyramidal_sequence_fb_median_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                         int iters, float alpha, float beta, int flow_median, float *uf, float *vf, float *ub,
                                         float *vb, float *err_f, float *err_b, unsigned char *valid_f, unsigned char *valid_b);
int oflk_interpolate_sequence_median(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                     float alpha, float beta, int refine, const double *taus, int n, int flow_median, float *out,
                                     unsigned char *status);
int oflk_interpolate_sequence_median_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                        float alpha, float beta, int refine, const double *taus, int n, int flow_median,
                                        unsigned char *out, unsigned char *status);
int oflk_interpolate_sequence_packed_median(const unsigned char *frames, int T, int H, int W, int channels, int order, int levels,
                                            int window_size, int iters, float alpha, float beta, int refine, const double *taus,
                                            int n, int flow_median, unsigned char *out, unsigned char *status);
int oflk_interpolate_sequence_nv12_median(const unsigned char *frames, int T, int H, int W, int siting, int levels,
                                          int window_size, int iters, float alpha, float beta, int refine, const double *taus,
                                          int n, int flow_median, unsigned char *out, unsigned char *status);

/* ---- motion-compensated temporal denoising on the dense flows ----------------------------------------------------------- */
/* Frames in, the same frames out with their noise averaged along the motion: the statement (tests/denoise_model.py).  Frames
 * are [T][H][W], float32 or uint8.  F_s = (uf[s], vf[s]) is the flow from frame s to frame s+1 and G_s = (ub[s], vb[s]) the
 * flow from frame s+1 to frame s, taken as they are.  sample and inside are the interpolation's (above): a point that is not
 * inside samples as 0 and reads no tap, so a flow value never becomes an address.  R = radius is in [1,
 * OFLK_DENOISE_MAX_RADIUS]; h2 = f32(strength) * f32(strength).  Every float32 and float64 operation is rounded on its own.
 *   for output frame t, pixel (x, y):
 *     c = f32(frame[t][y][x]);  num = c;  den = 1.0f;  count = 0
 *     two chains, backward (sgn = -1) and forward (sgn = +1), each: (px, py) = (f64(x), f64(y)), alive
 *     for k = 1 .. R:   for sgn in (-1, +1), in this order:
 *       s' = t + sgn*k;  the chain has ended, or s' < 0, or s' > T-1: nothing
 *       forward:  (A, B) = (F_{s'-1}, G_{s'-1});   backward: (A, B) = (G_{s'}, F_{s'})
 *       us = sample(A.u, px, py); vs = sample(A.v, px, py)
 *       qx = px + f64(us); qy = py + f64(vs)
 *       bu = sample(B.u, qx, qy); bv = sample(B.v, qx, qy)
 *       eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
 *       ok = inside(qx, qy) and e2 <= f32(alpha)*m2 + f32(beta)
 *       not ok: the chain ends (no sample from this frame or any beyond it on this side)
 *       ok: (px, py) = (qx, qy);  v = sample(frame[s'], qx, qy);  d = v - c;  w = 1.0f - (d*d) / h2
 *           if w > 0:  num = num + w*v;  den = den + w;  count += 1        (a NaN w is not > 0)
 *     out = num / den     (float32 division, correctly rounded)
 *     uint8 frames: out clamped to [0, 255], then (unsigned char) rintf, half to even
 * This is the interpolation's side test with the point carried from frame to frame.  The weight has compact support: a
 * neighbour that differs from the pixel by `strength` grey levels or more contributes nothing, which keeps a wrong vector or
 * an uncovered background from ghosting; 3 x the noise's sigma is the suggested strength.  A non-finite pixel is a value like
 * any other: it reaches out as the centre c, and as a neighbour its w is not > 0 and it is skipped.  count is the number of
 * neighbours that entered the average, 2 R at most.  These are grey planes; the weight is temporal only (no patch and no
 * spatial term), and the caller gives strength (no noise estimate).
 *
 * oflk_denoise_frames_host{,_u8}: frames [B+1][H][W] and the four flows [B][H][W] in, out [B+1][H][W] of the frames' type and
 * count [B+1][H][W] uint8 (may be NULL); host arrays, synchronous, staged like oflk_interpolate_frames_host.  One lane per
 * output pixel of one output frame, the frames along the grid's z, cut at 65535.
 * oflk_denoise_sequence{,_u8}: T frames in, out and count [T][H][W].  It runs oflk_pyramidal_sequence_fb_median's chunk loop
 * on its chunks (flow_median 0, 3, 5, 7 or 9; the bidirectional plan pass, flagged pairs of both directions resolved,
 * oflk_last_resolved() counts them, oflk_set_host_arithmetic applies to the flows): every pair's flows are computed exactly
 * once.  The flows of the last 2 R pairs and their frames stay on the device from chunk to chunk; a frame is emitted once the R
 * pairs ahead of it exist, the rest after the last chunk, and the result does not depend on the cut.  It equals
 * oflk_pyramidal_sequence_fb_median{,_u8} on the frames followed by oflk_denoise_frames_host{,_u8} on those flows, byte for
 * byte; only out and count come down, no flow leaves the device.
 * Refused before any device call: by the sequence forms whatever oflk_pyramidal_sequence_fb_median refuses, with its codes;
 * by the host forms NULL flows, NULL frames, H or W < 1, B < 1: OFLK_ERR_INVALID, and 2^30 pixels or more or 2^23 rows or
 * columns or more: OFLK_ERR_UNSUPPORTED; then by all, OFLK_ERR_INVALID: radius outside [1, OFLK_DENOISE_MAX_RADIUS], strength
 * not finite or not > 0, alpha or beta negative or not finite, NULL out, out overlapping the frames. */
#define OFLK_DENOISE_MAX_RADIUS 4
int oflk_denoise_frames_host(const float *frames, int B, int H, int W, const float *uf, const float *vf, const float *ub,
                             const float *vb, float alpha, float beta, int radius, float strength, float *out,
                             unsigned char *count);
int oflk_denoise_frames_host_u8(const unsigned char *frames, int B, int H, int W, const float *uf, const float *vf,
                                const float *ub, const float *vb, float alpha, float beta, int radius, float strength,
                                unsigned char *out, unsigned char *count);
int oflk_denoise_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                          float beta, int flow_median, int radius, float strength, float *out, unsigned char *count);
int oflk_denoise_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                             float alpha, float beta, int flow_median, int radius, float strength, unsigned char *out,
                             unsigned char *count);

/* ---- sparse pyramidal LK: points in, points out, no dense flow --------------------------------------------------------- */
/* The statement (tests/sparse_model.py).  The shape of calcOpticalFlowPyrLK: points in, next points + status + error out,
 * at a cost proportional to N * window^2 * levels * iterations, not to H*W.  Pyramids: build_gaussian_pyramid of each frame,
 * level 0 the coarsest, level L-1 the frame itself, sizes (h_l, w_l) = oflk_pyramid_level_dims at scale 0.5; exact
 * arithmetic always (oflk_set_host_arithmetic and oflk_plan_set_arithmetic do not apply).  sample(img, x, y) is the
 * reference's warp_image at one float64 point (map_coordinates, order 1, cval 0; float32 result).  Window w = 2h+1, odd,
 * 3 <= w <= 11; K = iters >= 1.  float32 except where stated, each operation rounded on its own.
 *   step(A, B, x, y), a float32 point of frame A inside [0, W-1] x [0, H-1]:
 *     g = (0, 0)
 *     for l = 0 .. L-1:
 *       l > 0:  g = (g.x * f32(w_l / w_{l-1}), g.y * f32(h_l / h_{l-1}))          upsample_flow's ratios (float64 quotients)
 *       (xl, yl) = (f64(x), f64(y)) at l = L-1;  elsewhere (f64(x) * (w_l - 1) / (W - 1), f64(y) * (h_l - 1) / (H - 1)),
 *                  float64, multiply then divide: the linspace geometry the level was resampled with
 *       P[j][i] = sample(A_l, xl + i, yl + j),  i, j in [-(h+1), h+1]               the template, once per level
 *       for k = 0 .. K-1:
 *         Q[j][i] = sample(B_l, (xl + f64(g.x)) + i, (yl + f64(g.y)) + j)
 *         (du, dv) = the centre pixel (h+1, h+1) of the reference's lucas_kanade_single_scale(P, Q, w) on the two
 *                    (w+2) x (w+2) patches: (P + Q) / 2, Sobel / 8 in convolve2d's order, It = P - Q, five np.sum of w*w
 *                    contiguous products, Cramer's rule where abs(det) > 1e-4 (else 0);  solved = abs(det) > 1e-4
 *         g = g + (du, dv);  leave the level when abs(du) < f32(0.01) and abs(dv) < f32(0.01)
 *     qx = f64(x) + f64(g.x);  qy = f64(y) + f64(g.y)
 *     ok = solved of the finest level's last evaluated iteration, and qx, qy finite, and 0 <= qx <= W-1, 0 <= qy <= H-1
 *          (float64, closed)
 *     residual = f32(np.sum(abs(Pc - Qc)) / f32(w*w)):  Pc the w x w centre of the finest level's P,
 *                Qc[j][i] = sample(B, qx + i, qy + j), i, j in [-h, h]
 * oflk_sparse_lk: one pair, host pointers, synchronous.  pts [N][2] (x, y) in; next_pts [N][2] = (f32(qx), f32(qy)), status
 * [N] = ok, residual [N] out (written whatever ok says: where no system was solved the point stays where it was, status 0).
 * A point that is not finite or lies outside the frame gives status 0, a NaN position and a NaN residual.
 * Refusals, before any device call: a pyramid level with a dimension below 2, or a window outside the odd sizes 3 ... 11:
 * OFLK_ERR_UNSUPPORTED;  iters < 1, levels < 1, N < 1, NULL pointers: OFLK_ERR_INVALID.  Frames are finite. */
int oflk_sparse_lk(const float *prev, const float *curr, int H, int W, int levels, int window_size, int iters,
                   const float *pts, int N, float *next_pts, unsigned char *status, float *residual);
int oflk_sparse_lk_u8(const unsigned char *prev, const unsigned char *curr, int H, int W, int levels, int window_size,
                      int iters, const float *pts, int N, float *next_pts, unsigned char *status, float *residual);
/* Sparse tracks, frames in, tracks out.  Rows, queries and NaN conventions are oflk_pyramidal_sequence_tracks'; the step
 * of an alive point (x, y) on pair t is
 *   (qx, qy, g, ok, r) = step(frame t, frame t+1, x, y);   if ok: (_, _, g', ok', _) = step(frame t+1, frame t, f32(qx), f32(qy))
 *   us, vs = g;  bu, bv = g';  eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
 *   alive = ok and ok' and e2 <= alpha*m2 + beta and r <= max_residual;   (x, y) = (f32(qx), f32(qy))
 * The residual test is part of the tracker: a point the occluder has covered usually passes the forward-backward test (both
 * steps lock onto the occluder's texture) and fails this one.  max_residual = +inf disables it.  Chunks of C+1 frames go up
 * (the boundary frame shared, the last row carried, as oflk_pyramidal_sequence_tracks; with no flow on the device a chunk
 * holds up to 64 pairs), only the rows come down; positions are float32 between steps, so results do not depend on the cut.
 * Checks as oflk_sparse_lk and oflk_pyramidal_sequence_tracks; max_residual negative or NaN: OFLK_ERR_INVALID. */
int oflk_pyramidal_sequence_sparse_tracks(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                          float alpha, float beta, float max_residual, const int *qt, const float *qxy, int N,
                                          float *tracks, unsigned char *visible);
int oflk_pyramidal_sequence_sparse_tracks_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                             int iters, float alpha, float beta, float max_residual, const int *qt,
                                             const float *qxy, int N, float *tracks, unsigned char *visible);

/* ---- Shi-Tomasi corners and detect-then-track (KLT) -------------------------------------------------------------- */
/* The statement (tests/feature_model.py).  One frame f [H][W], float32 or uint8 (converted exactly); window w = 2h+1, odd,
 * 3 <= w <= 11 (other windows: OFLK_ERR_UNSUPPORTED).  Score map S [H][W] float32:
 *   Ix, Iy = compute_gradients(f, f) (Sobel/8 of (f + f) / 2, the "symm" ring);  P = Ix*Ix, Ix*Iy, Iy*Iy (float32)
 *   R[y,x] = ((P[y,x-h] + P[y,x-h+1]) + ...) + P[y,x+h];  A[y,x] = ((R[y-h,x] + R[y-h+1,x]) + ...) + R[y+h,x]  (float32)
 *   a, b, c = Axx, Axy, Ayy;  S = 0 where y < h, y >= H-h, x < h or x >= W-h;  elsewhere, float64, each op rounded:
 *   det = a*c - b*b;  S = f32(2*det / ((a + c) + sqrt((a-c)*(a-c) + 4*b*b))) if det > 0, else 0;  non-finite S: 0
 * Selection (q = quality_level in [0,1], md = min_distance >= 0, K = max_corners >= 1):
 *   M = max(S) (M == 0: no features);  candidate: S > 0, f64(S) > f64(q)*f64(M), S >= each of its (up to) 8 neighbours
 *   priority: S descending, then y*W + x ascending;  greedy in that order: accept unless an accepted point lies at
 *   dx*dx + dy*dy < md*md (integers, float64);  stop after K
 *   count;  xy [K][2] float32 (x, y) in acceptance order;  score [K];  rows from count on: (NaN, NaN), score 0
 * Frames smaller than the window give count 0.  F < 1, a NULL pointer, q outside [0,1] or not finite, md negative or not
 * finite, K < 1: OFLK_ERR_INVALID, before any device call. */
/* F frames -> F score maps (synchronous) */
int oflk_corner_score_host(const float *frames, int F, int H, int W, int window_size, float *score);
int oflk_corner_score_host_u8(const unsigned char *frames, int F, int H, int W, int window_size, float *score);
/* F frames -> count [F], xy [F][K][2], score [F][K] (synchronous) */
int oflk_good_features_host(const float *frames, int F, int H, int W, int window_size, float quality_level,
                            float min_distance, int max_corners, int *count, float *xy, float *score);
int oflk_good_features_host_u8(const unsigned char *frames, int F, int H, int W, int window_size, float quality_level,
                               float min_distance, int max_corners, int *count, float *xy, float *score);
/* Detect, then track: the features of frame 0 (window = the LK window_size, which must therefore be a corner window) are
 * the queries of oflk_pyramidal_sequence_tracks, N = K, every query at frame 0; the NaN rows are never-visible tracks.
 * Equals oflk_good_features_host on frame 0 followed by oflk_pyramidal_sequence_tracks on its xy, byte for byte; the
 * features are born on the device from chunk 0's frames, no host round trip.  count [1], xy [K][2], score [K],
 * tracks [T][K][2], visible [T][K].  Checks as both. */
int oflk_pyramidal_sequence_klt(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                float alpha, float beta, float quality_level, float min_distance, int max_corners,
                                int *count, float *xy, float *score, float *tracks, unsigned char *visible);
int oflk_pyramidal_sequence_klt_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                                   float alpha, float beta, float quality_level, float min_distance, int max_corners,
                                   int *count, float *xy, float *score, float *tracks, unsigned char *visible);

/* ---- replenished KLT: re-detect corners away from the live tracks --------------------------------------------------- */
/* The statement (tests/replenish_model.py).  A fixed budget of K = max_corners slots; a slot holds at most one live track at
 * a time, and when its track ends a later detection may start a new one in it.  detect_every = D >= 1; the LK window is
 * the detection window (a corner window).  State per slot n: position (x, y) float32 and alive; every slot starts dead.
 * For t = 0 .. T-1:
 *   step (t > 0):  every alive slot takes the step of pair t-1 of oflk_track_points (two samples of the forward flow, the
 *                  forward-backward test at the landing point, the position rounded to float32); a slot whose step fails is
 *                  dead from row t on
 *   detect (t % D == 0 and t < T-1):
 *                  free = the dead slots, ascending;  seeds = (rint(x_n), rint(y_n)) of the alive slots (float32
 *                  round-half-even, as integers; alive positions lie inside the frame, so the seeds do)
 *                  S, M and the candidates of frame t are those of the corner statement above (M over the whole frame), in
 *                  its priority order;  greedy in that order: accept unless a seed or an already accepted point lies at
 *                  dx*dx + dy*dy < md*md (integers, float64);  stop after len(free) acceptances.  md = 0 refuses nothing.
 *                  the i-th accepted point goes to slot free[i]: position ((float)x, (float)y), alive, born[t][slot] = 1;
 *                  detected[t] = the number of acceptances (0 on frames without detection)
 *   row t:         tracks[t][n] = (x, y) if alive, else (NaN, NaN);  visible[t][n] = alive
 * tracks [T][K][2], visible [T][K], born [T][K] (0 / 1; born implies visible), detected [T].  A slot's rows are cut into
 * tracks at its born marks.  With D >= T only frame 0 detects and tracks / visible equal oflk_pyramidal_sequence_klt's byte
 * for byte.  Everything stays on the device between the frames going up and the rows coming down: a chunk's pairs are
 * tracked in segments cut at the detection frames.  detect_every < 1, a NULL output and every check of
 * oflk_pyramidal_sequence_klt: OFLK_ERR_INVALID / OFLK_ERR_UNSUPPORTED before any device call. */
int oflk_pyramidal_sequence_klt_replenish(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                          float alpha, float beta, float quality_level, float min_distance, int max_corners,
                                          int detect_every, float *tracks, unsigned char *visible, unsigned char *born,
                                          int *detected);
int oflk_pyramidal_sequence_klt_replenish_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                             int iters, float alpha, float beta, float quality_level, float min_distance,
                                             int max_corners, int detect_every, float *tracks, unsigned char *visible,
                                             unsigned char *born, int *detected);
/* One detection of that statement on host arrays (synchronous): frame [H][W] of index t >= 0, the slots' row xy [K][2] and
 * visible [K] in; qt [K] and qxy [K][2] in and out (slot free[i] gets qt = t and the i-th point, every other slot keeps its
 * bytes); born [K] and detected [1] out.  A visible slot whose position is outside [0, W-1] x [0, H-1] (NaN included) keeps
 * its slot and seeds nothing. */
int oflk_replenish_features_host(const float *frame, int H, int W, int window_size, float quality_level, float min_distance,
                                 int max_corners, int t, const float *xy, const unsigned char *visible, int *qt, float *qxy,
                                 unsigned char *born, int *detected);
int oflk_replenish_features_host_u8(const unsigned char *frame, int H, int W, int window_size, float quality_level,
                                    float min_distance, int max_corners, int t, const float *xy, const unsigned char *visible,
                                    int *qt, float *qxy, unsigned char *born, int *detected);

/* ---- replenished KLT on the sparse tracker ------------------------------------------------------------------------- */
/* The statement (tests/sparse_replenish_model.py): the replenished-KLT statement above with the step of the sparse tracks
 * (statement at oflk_pyramidal_sequence_sparse_tracks) in the place of the dense one, and one more output.  K = max_corners
 * slots, each holding at most one live track, every slot dead at first; D = detect_every >= 1; the LK window is the
 * detection window.  For t = 0 .. T-1:
 *   step (t > 0):  every alive slot takes the step of pair t-1 of the sparse tracks: step forward, then step backward from
 *                  f32(q) if the forward step is ok;  alive = ok and ok' and e2 <= alpha*m2 + beta and r <= max_residual;
 *                  the position becomes (f32(qx), f32(qy))
 *                  residual[t][n] = the forward step's r where that step was ok, for every slot alive on row t-1, whether
 *                  or not the track survives the step.  Every other entry is NaN: a slot dead on row t-1 (one born on row t
 *                  in a slot that was dead keeps its NaN), a forward step that was not ok, and all of row 0.  A slot whose
 *                  track ends on row t and that is filled again on row t holds the ended track's residual there.
 *   detect (t % D == 0 and t < T-1):  exactly the detection of the replenished-KLT statement on frame t: the free slots
 *                  ascending, the seeds rint of the alive slots' positions after the step, the greedy stopped after
 *                  len(free) acceptances, the i-th accepted point into slot free[i] (alive, born[t][slot] = 1),
 *                  detected[t] = the number accepted
 *   row t:         tracks[t][n] = (x, y) if alive, else (NaN, NaN);  visible[t][n] = alive
 * With D >= T tracks and visible are those of the detection on frame 0 followed by the sparse tracks.  Positions are
 * float32 between steps and a call's last row is never a detection row of that call, so the result does not depend on how
 * the sequence is cut into calls or chunks.
 *
 * oflk_pyramidal_sequence_klt_sparse: detect once, then the sparse tracks.  Equals oflk_good_features_host on frame 0
 * followed by oflk_pyramidal_sequence_sparse_tracks on its xy (N = K, every query at frame 0, the NaN rows never-visible
 * tracks), byte for byte; the features are born on the device, straight into the query buffer.  Outputs as
 * oflk_pyramidal_sequence_klt.
 * oflk_pyramidal_sequence_klt_sparse_replenish: the statement.  tracks [T][K][2], visible, born [T][K], detected [T],
 * residual [T][K] (may be NULL).  Chunks as oflk_pyramidal_sequence_sparse_tracks (at most 64 pairs, sized by the frames
 * alone; the boundary frame shared, the last row carried); a chunk holds its frames and their pyramids, the rows and the
 * detection's workspace of one frame, and no flow.  Its pyramids are built once and its pairs tracked in segments cut at
 * the detection frames, the seven launches of a detection ahead of the segment that begins on one.  Only rows, born,
 * detected and residual come down.
 * Checks: those of oflk_pyramidal_sequence_sparse_tracks and of oflk_pyramidal_sequence_klt_replenish, with their codes,
 * before any device call. */
int oflk_pyramidal_sequence_klt_sparse(const float *frames, int T, int H, int W, int levels, int window_size, int iters,
                                       float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                       int max_corners, int *count, float *xy, float *score, float *tracks,
                                       unsigned char *visible);
int oflk_pyramidal_sequence_klt_sparse_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size,
                                          int iters, float alpha, float beta, float max_residual, float quality_level,
                                          float min_distance, int max_corners, int *count, float *xy, float *score,
                                          float *tracks, unsigned char *visible);
int oflk_pyramidal_sequence_klt_sparse_replenish(const float *frames, int T, int H, int W, int levels, int window_size,
                                                 int iters, float alpha, float beta, float max_residual, float quality_level,
                                                 float min_distance, int max_corners, int detect_every, float *tracks,
                                                 unsigned char *visible, unsigned char *born, int *detected,
                                                 float *residual /* [T][K], may be NULL */);
int oflk_pyramidal_sequence_klt_sparse_replenish_u8(const unsigned char *frames, int T, int H, int W, int levels,
                                                    int window_size, int iters, float alpha, float beta, float max_residual,
                                                    float quality_level, float min_distance, int max_corners, int detect_every,
                                                    float *tracks, unsigned char *visible, unsigned char *born, int *detected,
                                                    float *residual /* [T][K], may be NULL */);

/* ---- online sparse KLT tracker: frames pushed one at a time ------------------------------------------------------------ */
/* The statement (tests/tracker_model.py): the sparse-replenish statement above for video that arrives frame by frame and
 * has no known end.  A tracker keeps K = max_corners slots on the device (every slot dead at first) and takes one frame
 * per push.  D = detect_every >= 0.  Push of frame t (t = 0, 1, ...):
 *   step (t > 0):  every alive slot takes the step of pair t-1 of the sparse-replenish statement, unchanged: forward,
 *                  backward, the forward-backward test, r <= max_residual, the position f32(q), residual[n] as there
 *   detect (D > 0 and t % D == 0):  the detection of that statement on frame t with the rows after the step -- now, not when
 *                  the next frame arrives: a tracker knows no last frame, so that statement's t < T-1 falls away
 *   row t:         xy[n] = the position, or (NaN, NaN);  visible[n];  born[n] = 1 where a track began in slot n on this frame;
 *                  birth[n] = the index of the frame on which the slot's current track began (defined where visible[n]);
 *                  residual[n], all NaN on frame 0;  detected = the points accepted on this frame
 * So the rows of T pushes are rows 0 .. T-1 of oflk_pyramidal_sequence_klt_sparse_replenish on those frames followed by any
 * one more frame, byte for byte.  With D = 0 nothing is ever detected.
 * oflk_tracker_add_points after the push of frame t: points that are not finite or lie outside [0, W-1] x [0, H-1] are dropped
 * on the host; the i-th remaining point goes to the i-th dead slot, ascending, while dead slots last, and the rest are
 * dropped.  Such a slot gets position (x + 0, y + 0), visible = 1, born = 1, birth = t; a later read_row shows it, and from
 * the next push on it is an ordinary track that seeds later detections like any other.  With D = 0 a slot's track equals
 * the track of the query (t, x, y) in oflk_pyramidal_sequence_sparse_tracks.
 *
 * State: a ring of two frames in the input pixel type, their two pyramids, two rows, birth / the detection's queries / born /
 * residual / detected, the points of add_points and the oflk_replenish_features workspace of one frame.  Every pyramid step
 * runs the fused kernel, which at the pyramid's scale of 0.5 fits every admissible frame (a step that does not cannot occur at
 * that scale), so there are no blur temporaries and no float32 copy of uint8 frames.  Creation checks the configuration and
 * makes no device call; the first push allocates all of it, no later push allocates.  A push is enqueued from host-side state
 * -- the ring slot t & 1, the birth index t, whether t % D == 0 -- so a captured push replayed would repeat one frame's role:
 * pushes are not made for graph capture.  A push copies the frame into the free ring slot, builds that one frame's pyramid
 * (the previous frame's is kept), and runs one launch for the step of all slots; a detecting push adds the seven launches of a
 * detection and one that completes the rows of the newborn.  A push that fails part-way leaves the frame index and the
 * previous row as they were, and every later push is refused with OFLK_ERR_INVALID until oflk_tracker_reset.
 * A tracker is single-stream, like a plan: every call on it is ordered by the caller.
 * Refusals, before any device call: everything oflk_pyramidal_sequence_klt_sparse_replenish refuses about shape, window,
 * levels, iterations, alpha, beta, max_residual, quality_level, min_distance and max_corners, with its codes;
 * detect_every < 0: OFLK_ERR_INVALID;  row_device / read_row / add_points before the first push, n < 1 or a NULL tracker,
 * frame or points: OFLK_ERR_INVALID;  a push after frame index 2^31 - 2: OFLK_ERR_UNSUPPORTED (oflk_tracker_reset starts
 * again at frame 0). */
typedef struct oflk_tracker oflk_tracker;
int oflk_tracker_create(oflk_tracker **tr, int device, int H, int W, int u8, int levels, int window_size, int iters,
                        float alpha, float beta, float max_residual, float quality_level, float min_distance,
                        int max_corners /* K slots */, int detect_every /* D >= 1; 0: never detect */);
int oflk_tracker_destroy(oflk_tracker *tr);
int oflk_tracker_reset(oflk_tracker *tr, void *stream);      /* every slot dead, next push is frame 0 */
size_t oflk_tracker_workspace_bytes(const oflk_tracker *tr); /* what is allocated at the moment (0 before the first push) */
int oflk_tracker_frame_index(const oflk_tracker *tr);        /* index of the last pushed frame, -1 before the first */
/* device frame [H][W] (uint8 when created with u8); asynchronous on `stream`, no host synchronisation */
int oflk_tracker_push_device(oflk_tracker *tr, const void *d_frame, void *stream);
/* device pointers to the row of the last pushed frame (each may be NULL), valid until the next push / add / reset:
 * xy [K][2], visible [K], born [K], birth [K], residual [K], detected [1] */
int oflk_tracker_row_device(const oflk_tracker *tr, const float **d_xy, const unsigned char **d_visible,
                            const unsigned char **d_born, const int **d_birth, const float **d_residual,
                            const int **d_detected);
/* copy that row to host arrays (each may be NULL); synchronises `stream` */
int oflk_tracker_read_row(oflk_tracker *tr, float *xy, unsigned char *visible, unsigned char *born, int *birth,
                          float *residual, int *detected, void *stream);
/* host frame in, the row out: push_device + read_row on the null stream, the frame copied straight into the ring;
 * synchronous */
int oflk_tracker_push(oflk_tracker *tr, const void *frame, float *xy, unsigned char *visible, unsigned char *born,
                      int *birth, float *residual, int *detected);
/* n host points (x, y) start tracks on the last pushed frame, in the dead slots, ascending; the points are on the device
 * when the call returns (it synchronises `stream` once), the slots are filled in stream order */
int oflk_tracker_add_points(oflk_tracker *tr, const float *pts, int n, void *stream);

/* ---- global motion from point correspondences: deterministic RANSAC and a least-squares refit ------------------------- */
/* The statement (tests/motion_model.py), per step with hash index i: correspondences src[n] -> dst[n], a validity mask, a
 * model family, Hn hypotheses, a threshold (px) and a seed.
 *   families       OFLK_MOTION_TRANSLATION (sample m = 1), OFLK_MOTION_SIMILARITY (m = 2: x' = a x - b y + tx, y' = b x + a y
 *                  + ty), OFLK_MOTION_AFFINE (m = 3); a model is six float32 [a00 a01 tx; a10 a11 ty]
 *   compaction     valid: the mask byte non-zero (no mask: always) and the four coordinates finite; the M valid ones keep
 *                  their slot order.  M < m: the failure result -- six NaNs, mask all 0, counts (0, M, 0)
 *   sampling       draw(seed, i, h, j): x = fmix(seed ^ 0x9E3779B9); x = fmix(x + i); x = fmix(x + h); x = fmix(x + j) on
 *                  uint32 with murmur3's finaliser fmix.  Pick j of hypothesis h is r = draw % (M - j), the r-th position not
 *                  yet picked, ascending.  A step depends on its own inputs and its index only
 *   minimal solve  float64 on the points converted to double, each operation rounded on its own, differences taken from
 *                  the first point; the six coefficients rounded to float32.  Coincident points (similarity), a zero
 *                  determinant (affine) or a coefficient that is not finite: degenerate, score -1
 *   score          float32, one operation at a time: ex = ((a00 x + a01 y) + tx) - qx, ey likewise, r2 = ex ex + ey ey;
 *                  inlier: r2 <= threshold * threshold.  Score = inliers among the valid; best = largest, ties to the
 *                  lowest h; every hypothesis degenerate: the failure result
 *   refit          least squares of the family over the best hypothesis's inliers, centred on their centroids, float64
 *                  sums of the float32 inputs in a stated order: 256 partials, partial l adds positions l, l + 256, ...
 *                  ascending from +0.0, then partial[l] += partial[l + stride] for stride 128, 64, ..., 1.  No inlier, a
 *                  zero determinant / spread or a result not finite in float32: the best hypothesis's model is kept
 *   outputs        model [6];  inlier [N]: the score's test with the returned model on the valid correspondences, 0
 *                  elsewhere;  counts [3] = (n_inliers = the mask's sum, n_valid = M, status = 1)
 * These calls fit six coefficients: homographies have their own calls below, and iterative re-estimation is not offered.
 * Three kernel launches on `stream` (compaction, scoring with one wave per hypothesis, select-and-refit), no memset, no
 * atomics, nothing synchronised: the chain can be captured into a graph after one eager call.
 * Refusals, before any device call: an unknown model, hypotheses < 1 or > OFLK_MOTION_MAX_HYPOTHESES, a threshold that is
 * not finite and positive, S or N < 1 (T < 2, K < 1), NULL pointers (d_valid and d_born may be NULL), d_src / d_dst /
 * d_tracks not 8-byte aligned, a workspace that is too small or not 256-byte aligned: OFLK_ERR_INVALID. */
#define OFLK_MOTION_TRANSLATION 0
#define OFLK_MOTION_SIMILARITY 1
#define OFLK_MOTION_AFFINE 2
#define OFLK_MOTION_MAX_HYPOTHESES 65536
/* bytes of the caller's workspace for S steps of N correspondences */
int oflk_motion_workspace(int S, int N, int hypotheses, size_t *bytes);
/* device form: d_src, d_dst [S][N][2], d_valid [S][N] or NULL (finiteness alone decides); step s draws with index step0 + s
 * (uint32, wrapping).  d_model [S][6], d_inlier [S][N], d_counts [S][3].  Asynchronous on `stream`. */
int oflk_estimate_motion(const float *d_src, const float *d_dst, const unsigned char *d_valid, int S, int N, int step0,
                         int model, int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes,
                         float *d_model, unsigned char *d_inlier, int *d_counts, void *stream);
/* device form on rows as the track calls write them: d_tracks [T][K][2], d_visible [T][K], d_born [T][K] or NULL.  Step t
 * (0 <= t < T-1) runs from row t to row t+1 with index t0 + t; slot n is valid on it when it is visible on both rows and
 * not born on row t+1 (a slot that died and was refilled on one row is two different tracks).  The workspace is that of
 * S = T-1, N = K; d_model [T-1][6], d_inlier [T-1][K], d_counts [T-1][3]. */
int oflk_tracks_motion(const float *d_tracks, const unsigned char *d_visible, const unsigned char *d_born, int T, int K, int t0,
                       int model, int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes,
                       float *d_model, unsigned char *d_inlier, int *d_counts, void *stream);
/* host arrays in and out (valid may be NULL); synchronous */
int oflk_estimate_motion_host(const float *src, const float *dst, const unsigned char *valid, int S, int N, int step0, int model,
                              int hypotheses, float threshold, unsigned seed, float *model_out, unsigned char *inlier,
                              int *counts);
/* The tracker's motion row.  model = -1 turns it off (the default; the other arguments are then ignored), and a push
 * enqueues exactly what it does without this call.  With a model set, the push of frame t >= 1 enqueues, after its step and
 * any detection, the fit of step t-1 -> t on the tracker's two rows: slot n is valid when visible on both and not born on
 * frame t; the index is t-1.  Frame 0 (also after a reset) gets the failure result with M = 0.  So the motion rows of T
 * pushes are steps 0 .. T-2 of oflk_tracks_motion on the rows of those pushes.  May be called between pushes; it takes
 * effect on the next push, which (re)allocates the fit's buffers when they are missing or too small -- the one exception
 * to "no later push allocates"; oflk_tracker_workspace_bytes counts them.  Points of oflk_tracker_add_points join the fit
 * from the next step on.  motion_device / read_motion before a push with motion on: OFLK_ERR_INVALID. */
int oflk_tracker_set_motion(oflk_tracker *tr, int model, int hypotheses, float threshold, unsigned seed);
/* device pointers (each may be NULL) to the last push's motion row: model [6], inlier [K], counts [3] */
int oflk_tracker_motion_device(const oflk_tracker *tr, const float **d_model, const unsigned char **d_inlier,
                               const int **d_counts);
/* copy it to host arrays (each may be NULL); synchronises `stream` */
int oflk_tracker_read_motion(oflk_tracker *tr, float *model, unsigned char *inlier, int *counts, void *stream);

/* ---- homography from point correspondences: a four-point RANSAC and a normalised linear refit ------------------------- */
/* The statement (tests/homography_model.py), per step with hash index i: correspondences src[n] -> dst[n], a validity mask,
 * Hn hypotheses, a threshold (px) and a seed.  A model is nine float32, row-major [h00 h01 h02; h10 h11 h12; h20 h21 h22]
 * with h22 == 1.0f exactly: dst = (h00 x + h01 y + h02, h10 x + h11 y + h12) / (h20 x + h21 y + h22).
 *   compaction     as the motion fit's.  M < 4: the failure result -- nine NaNs, mask all 0, counts (0, M, 0)
 *   sampling       the motion fit's draw and rule with m = 4 picks: pick j is r = draw % (M - j), bumped once for each
 *                  earlier pick, taken in ascending order, that is <= it
 *   minimal solve  float64 on the points converted to double, each operation rounded on its own.  Q(x0, y0 .. x3, y3), the
 *                  map of the unit square onto a quadrilateral in pick order:  sx = (x0 - x1) + (x2 - x3), sy likewise;
 *                  dx1 = x1 - x2, dx2 = x3 - x2, dy1, dy2 likewise;  den = dx1 dy2 - dy1 dx2;  g = (sx dy2 - sy dx2) / den;
 *                  h = (dx1 sy - dy1 sx) / den;  Q = [(x1 - x0) + g x1, (x3 - x0) + h x3, x0;  (y1 - y0) + g y1,
 *                  (y3 - y0) + h y3, y0;  g, h, 1].  S = Q of the source points, D = Q of the destination points,
 *                  Hm = D adj(S) with adj(S), for S = [a b c; d e f; g h i], = [e i - f h, c h - b i, b f - c e;
 *                  f g - d i, a i - c g, c d - a f;  d h - e g, b g - a h, a e - b d] and the product's entries
 *                  (r0 c0 + r1 c1) + r2 c2;  the nine entries divided by Hm[2][2] and rounded to float32.  den == 0 on either
 *                  side, Hm[2][2] == 0 or a coefficient that is not finite: degenerate, score -1
 *   score          float32, one operation at a time:  w = (h20 x + h21 y) + h22;  ex = ((h00 x + h01 y) + h02) / w - qx, ey
 *                  likewise (IEEE division);  r2 = ex ex + ey ey;  inlier: w > 0 and r2 <= threshold * threshold.  Best =
 *                  largest count, ties to the lowest h; every hypothesis degenerate: the failure result
 *   refit          over the best hypothesis's inliers, float64, every sum in the motion fit's stated order.  (a) the count n
 *                  and the four coordinate sums give the centroids cpx, cpy, cqx, cqy.  (b) lp = sum(|X - cpx| + |Y - cpy|),
 *                  lq likewise;  sp = n / lp, sq = n / lq (no square root).  (c) x = (X - cpx) sp, y = (Y - cpy) sp,
 *                  u = (U - cqx) sq, v = (V - cqy) sq.  (d) the normal equations G h = b of the rows
 *                  [x y 1 0 0 0 -xu -yu | u] and [0 0 0 x y 1 -xv -yv | v]: with xx = x x, xy = x y, yy = y y,
 *                  r = u u + v v, the 22 sums of xx, xy, yy, x, y;  xx u, xy u, yy u, x u, y u;  the same five with v;
 *                  xx r, xy r, yy r;  u, v, x r, y r (a three-factor term is the two-factor product times the third), n
 *                  in G[2][2] and G[5][5].  (e) elimination without pivoting on [G | b]: for k = 0 .. 7, for i = k+1 .. 7,
 *                  f = G[i][k] / G[k][k], G[i][j] -= f G[k][j] for j = k+1 .. 8 ascending;  then for i = 7 .. 0,
 *                  h[i] = (b[i] - G[i][j] h[j], j = i+1 .. 7 ascending, one by one) / G[i][i].  (f) with Hn = [h0 .. h7, 1],
 *                  tx = sp cpx, ty = sp cpy:  A[r][0] = Hn[r][0] sp, A[r][1] = Hn[r][1] sp,
 *                  A[r][2] = Hn[r][2] - (Hn[r][0] tx + Hn[r][1] ty);  B[0][c] = A[0][c] / sq + cqx A[2][c],
 *                  B[1][c] = A[1][c] / sq + cqy A[2][c], B[2][c] = A[2][c];  the nine entries divided by B[2][2] and rounded
 *                  to float32.  No inlier, lp or lq zero, a pivot zero or not finite, B[2][2] zero or a result not finite
 *                  in float32: the best hypothesis's model is kept
 *   outputs        model [9];  inlier [N]: the score's test with the returned model on the valid correspondences, 0
 *                  elsewhere;  counts [3] = (n_inliers, n_valid = M, status = 1)
 * model[t] of oflk_tracks_homography maps row t to row t+1, so oflk_warp_perspective of frame t+1 under model[t] (converted
 * to double) registers frame t+1 onto frame t.  The tracker's motion row and the stabiliser keep six coefficients.
 * Three kernel launches on `stream` (the motion fit's compaction, scoring with one wave per hypothesis, select-and-refit), no
 * memset, no atomics, nothing synchronised: the chain can be captured into a graph after one eager call.
 * Refusals, before any device call: hypotheses < 1 or > OFLK_MOTION_MAX_HYPOTHESES, a threshold that is not finite and
 * positive, S or N < 1 (T < 2, K < 1), NULL pointers (d_valid and d_born may be NULL), d_src / d_dst / d_tracks not 8-byte
 * aligned, a workspace that is too small or not 256-byte aligned: OFLK_ERR_INVALID. */
/* bytes of the caller's workspace for S steps of N correspondences */
int oflk_homography_workspace(int S, int N, int hypotheses, size_t *bytes);
/* device form, as oflk_estimate_motion's: d_model [S][9], d_inlier [S][N], d_counts [S][3].  Asynchronous on `stream`. */
int oflk_estimate_homography(const float *d_src, const float *d_dst, const unsigned char *d_valid, int S, int N, int step0,
                             int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes,
                             float *d_model, unsigned char *d_inlier, int *d_counts, void *stream);
/* device form on rows, with oflk_tracks_motion's validity rule: the workspace is that of S = T-1, N = K; d_model [T-1][9],
 * d_inlier [T-1][K], d_counts [T-1][3] */
int oflk_tracks_homography(const float *d_tracks, const unsigned char *d_visible, const unsigned char *d_born, int T, int K, int t0,
                           int hypotheses, float threshold, unsigned seed, void *d_workspace, size_t workspace_bytes,
                           float *d_model, unsigned char *d_inlier, int *d_counts, void *stream);
/* host arrays in and out (valid may be NULL); synchronous */
int oflk_estimate_homography_host(const float *src, const float *dst, const unsigned char *valid, int S, int N, int step0,
                                  int hypotheses, float threshold, unsigned seed, float *model_out, unsigned char *inlier,
                                  int *counts);

/* ---- video stabilisation: a smoothed trajectory of the step models and an affine warp of whole frames ------------------ */
/* The statement (tests/stabilize_model.py).  Every operation is float64 unless stated and rounded on its own, in the order
 * written; nothing is contracted and the device computes no transcendental.
 * Trajectory: one correction per frame from the T-1 step models.
 *   inputs         model [T-1][6] float32 [a00 a01 tx; a10 a11 ty], step s mapping frame s to frame s+1, as
 *                  oflk_tracks_motion writes it;  counts [T-1][3] or NULL;  weights[0 .. r] float64, finite and positive,
 *                  formed by the caller on the host (as oflk_build_pyramid_w takes its Gaussian table);  the radius r,
 *                  0 <= r <= OFLK_STABILIZE_MAX_RADIUS;  T >= 1 (T == 1: model may be NULL)
 *   inverse        of [a00 a01 tx; a10 a11 ty]:  det = a00 a11 - a01 a10;  i00 = a11 / det, i01 = -a01 / det,
 *                  i10 = -a10 / det, i11 = a00 / det;  itx = -(i00 tx + i01 ty), ity = -(i10 tx + i11 ty)
 *   step s         A_s = the six coefficients as double, B_s = its inverse.  The step is held when counts[s][2] == 0, a
 *                  coefficient is not finite, det == 0 or a coefficient of B_s is not finite: then A_s = B_s = identity (the
 *                  camera is taken to stand still across a step that could not be fitted) and held[s] = 1, else 0
 *   composition    C = A o F (F first):  c00 = A00 F00 + A01 F10, c01 = A00 F01 + A01 F11, ctx = (A00 Ftx + A01 Fty) + Atx,
 *                  and the second row likewise
 *   frame t        r_t = min(r, t, T-1-t): the window is always symmetric, so frames 0 and T-1 are never moved and a
 *                  uniform camera motion is left alone on every frame.  acc = weights[0] I (six products),
 *                  ws = weights[0], F = G = I;  for i = 1 .. r_t:  F = A_{t+i-1} o F;  acc += weights[i] F;
 *                  ws += weights[i];  G = B_{t-i} o G;  acc += weights[i] G;  ws += weights[i].  Forward, then backward,
 *                  inside each i: that order makes a constant integer pan cancel exactly.
 *                  correction[t] = f32(acc / ws), six quotients;  map[t] = the inverse, by the formula above, of
 *                  correction[t] converted back to double.  det == 0 or anything not finite: both are the identity
 *   outputs        correction [T][6] float32 (where frame t's content is moved to), map [T][6] float64 (the output pixel's
 *                  source position: what oflk_warp_affine takes), held [T-1] bytes (may be NULL)
 * This is the relative-motion average of Gaussian motion filtering: a scene point's steadied path is the weighted mean of its
 * path over the window, and the mean of translations is a translation, of similarities a similarity.
 * Warp: out[f][y][x] = sample(frame f, xs, ys) with xs = (m0 f64(x) + m1 f64(y)) + m2, ys = (m3 f64(x) + m4 f64(y)) + m5,
 * m = map[f];  sample is the bilinear sample stated above (the reference's warp_image at one float64 point:
 * map_coordinates, order 1, cval 0, float32 result).  inside[f][y][x] = 1 where 0 <= xs <= W-1 and 0 <= ys <= H-1 (float64,
 * closed; the taps were read), else 0, and there the sample is 0.  float32 frames give float32; uint8 frames give
 * (unsigned char) rintf(sample), half to even (a sample of bytes lies in [0, 255]).  Frames are finite, H, W >= 2, and out
 * does not overlap the frames.  Cropping or zooming the border away (inside is what a caller needs for it) and
 * rolling-shutter correction are not offered; the trajectory and the sequence calls smooth six coefficients, not homographies.
 * Perspective warp (tests/homography_model.py): m = map[f] has nine coefficients;  w = (m6 f64(x) + m7 f64(y)) + m8;
 * xs = ((m0 x + m1 y) + m2) / w, ys = ((m3 x + m4 y) + m5) / w -- two IEEE float64 divisions, not one reciprocal;
 * inside = w > 0 and 0 <= xs <= W-1 and 0 <= ys <= H-1, a NaN anywhere meaning outside;  everything else as above.  A map
 * whose third row is (0, 0, 1) therefore gives oflk_warp_affine's bytes under its first two rows.
 * Refusals, before any device call: T < 1 (the sequence call: T < 2), F < 1, H or W < 2, a radius outside
 * [0, OFLK_STABILIZE_MAX_RADIUS], a weight that is not finite and positive, NULL pointers (d_counts, d_held, d_inside and
 * the sequence call's last four outputs may be NULL; d_model when T == 1), d_map not 8-byte aligned: OFLK_ERR_INVALID;
 * frames of 2^30 pixels or more: OFLK_ERR_UNSUPPORTED.  The sequence call also refuses whatever
 * oflk_pyramidal_sequence_klt_sparse_replenish and oflk_tracks_motion refuse, with their codes. */
#define OFLK_STABILIZE_MAX_RADIUS 64
/* device form, one launch (one thread per frame, the weights in the launch arguments), asynchronous on `stream`; can be
 * captured into a graph */
int oflk_stabilize_trajectory(const float *d_model, const int *d_counts, int T, const double *weights /* host, [radius + 1] */,
                              int radius, float *d_correction, double *d_map, unsigned char *d_held, void *stream);
/* device form, one launch for the F frames: d_frames, d_out [F][H][W] (uint8 when u8), d_map [F][6] float64, d_inside
 * [F][H][W] bytes or NULL.  Asynchronous on `stream`. */
int oflk_warp_affine(const void *d_frames, int u8, int F, int H, int W, const double *d_map, void *d_out,
                     unsigned char *d_inside, void *stream);
/* host arrays, synchronous.  The warp goes in chunks of at most 64 frames; frames are independent, so the result does not
 * depend on the cut. */
int oflk_stabilize_trajectory_host(const float *model, const int *counts, int T, const double *weights, int radius,
                                   float *correction, double *map, unsigned char *held);
int oflk_warp_affine_host(const float *frames, int F, int H, int W, const double *map, float *out, unsigned char *inside);
int oflk_warp_affine_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, unsigned char *out,
                             unsigned char *inside);
/* the perspective warp, with oflk_warp_affine's forms, refusals and chunks: d_map / map [F][9] float64 */
int oflk_warp_perspective(const void *d_frames, int u8, int F, int H, int W, const double *d_map, void *d_out,
                          unsigned char *d_inside, void *stream);
int oflk_warp_perspective_host(const float *frames, int F, int H, int W, const double *map, float *out, unsigned char *inside);
int oflk_warp_perspective_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, unsigned char *out,
                                  unsigned char *inside);
/* Frames in, steadied frames out.  By statement, byte for byte: oflk_pyramidal_sequence_klt_sparse_replenish on the frames,
 * oflk_tracks_motion on its rows with t0 = 0, oflk_stabilize_trajectory on the models and counts, oflk_warp_affine of the
 * frames under its maps.  Pass 1 is the replenish call's chunk loop, from which only rows come down; then the fit and the
 * trajectory of all T frames run at once on the rows (a few KB per frame); pass 2 sends the frames up again in chunks and
 * the steadied frames come down.  Nothing of the sequence's size is ever on the device.
 * out [T][H][W] in the input type;  correction [T][6], model_out [T-1][6], counts_out [T-1][3], held [T-1]: each may be
 * NULL. */
int oflk_stabilize_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                            float beta, float max_residual, float quality_level, float min_distance, int max_corners,
                            int detect_every, int model, int hypotheses, float threshold, unsigned seed, const double *weights,
                            int radius, float *out, float *correction, float *model_out, int *counts_out, unsigned char *held);
int oflk_stabilize_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters,
                               float alpha, float beta, float max_residual, float quality_level, float min_distance,
                               int max_corners, int detect_every, int model, int hypotheses, float threshold, unsigned seed,
                               const double *weights, int radius, unsigned char *out, float *correction, float *model_out,
                               int *counts_out, unsigned char *held);

/* ---- video mosaics: chained homographies, every frame blended onto one canvas ------------------------------------------- */
/* The statement (tests/mosaic_model.py).  Every operation is float64 unless stated and rounded on its own, in the order
 * written; nothing is contracted, there is no transcendental and no atomic, and no result depends on the launch geometry or on
 * how the frames are cut into calls.  The device equals it byte for byte, a NaN equal to a NaN.
 * Chain: the step models composed from an anchor frame.
 *   inputs         model [T-1][9] float32 and counts [T-1][3] (or NULL) as oflk_tracks_homography writes them;  the anchor a
 *                  in [0, T-1];  the frame size H, W >= 2;  extent, finite and positive;  T >= 1 (T == 1: model may be NULL)
 *   step s         A_s = the nine coefficients as double;  B_s = adj(A_s) / adj(A_s)[2][2]: the adjugate's nine cofactors
 *                  (each a b - c d, as the homography fit writes them: e i - f h, c h - b i, b f - c e;  f g - d i, a i - c g,
 *                  c d - a f;  d h - e g, b g - a h, a e - b d for the rows [a b c; d e f; g h i]) and nine divisions.  The
 *                  step is held when counts[s][2] == 0, a coefficient of A_s is not finite, adj[2][2] == 0 or a coefficient of
 *                  B_s is not finite: then A_s = B_s = I and held[s] = 1, else 0 (the stabiliser's rule)
 *   composition    C = X o Y (Y first):  C[r][c] = (X[r][0] Y[0][c] + X[r][1] Y[1][c]) + X[r][2] Y[2][c], then all nine
 *                  divided by C[2][2]
 *   chains         P_t maps anchor coordinates to frame t's:  P_a = I;  P_t = A_{t-1} o P_{t-1} for t > a;
 *                  P_t = B_t o P_{t+1} for t < a.  Q_t maps frame t's to the anchor's:  Q_a = I;  Q_t = Q_{t-1} o B_{t-1} for
 *                  t > a;  Q_t = Q_{t+1} o A_t for t < a.  Q is a chain of its own, not an inversion of P
 *   box            the corners (0,0), (W-1,0), (W-1,H-1), (0,H-1) under Q_t by the perspective warp's formula, divisions
 *                  included:  w = (q6 x + q7 y) + q8, X = ((q0 x + q1 y) + q2) / w, Y likewise;
 *                  box[t] = (xmin, ymin, xmax, ymax), each taken as min(min(c0, c1), min(c2, c3))
 *   dropped[t]     1 when a corner's w <= 0, anything in P_t, Q_t or the corners is not finite, or a corner coordinate
 *                  exceeds extent in absolute value;  and for every frame further from the anchor on that side, whose chain
 *                  runs through the dropped one.  The anchor is never dropped.  box of a dropped frame is four NaNs;  its
 *                  from_anchor and to_anchor hold what the chain computed
 *   outputs        from_anchor [T][9] = P (what oflk_mosaic_accumulate takes), to_anchor [T][9] = Q, box [T][4] float64;
 *                  held [T-1] (may be NULL) and dropped [T] bytes
 * Canvas (host integers): x0 = floor(min xmin), y0 = floor(min ymin) over the frames not dropped,
 * Wc = ceil(max xmax) - x0 + 1, Hc likewise.
 * Accumulate.  The state represents, per canvas pixel, a float64 sum, a float64 wsum and an int32 count; all-zero bytes are
 * the empty canvas (clear it with a memset); its layout is private.  Canvas pixel (x, y) has fx = f64(x0 + x),
 * fy = f64(y0 + y), the sums formed in integers.  For f = 0 .. F-1 ascending with skip[f] == 0, m = map[f]:
 *   w = (m6 fx + m7 fy) + m8;  xs = ((m0 fx + m1 fy) + m2) / w;  ys = ((m3 fx + m4 fy) + m5) / w;
 *   inside = w > 0 and 0 <= xs <= W-1 and 0 <= ys <= H-1, a NaN anywhere meaning outside
 * -- oflk_warp_perspective's, with (fx, fy) for the pixel indices.  Where inside, s = the float32 bilinear sample of frame f
 * at (xs, ys), and
 *   OFLK_MOSAIC_MEAN      sum += f64(s);  wsum += 1.0
 *   OFLK_MOSAIC_FEATHER   g = min(min(xs, (W-1) - xs), min(ys, (H-1) - ys)) + 1.0;  sum += g * f64(s) (the product rounded,
 *                         then the sum);  wsum += g
 *   OFLK_MOSAIC_FIRST     only when count == 0:  sum = f64(s), wsum = 1.0
 *   OFLK_MOSAIC_LAST      sum = f64(s), wsum = 1.0
 * and count += 1 in every mode.  A pixel's samples are added one by one in frame order, so a canvas accumulated in several
 * calls (frames 0 .. k, then k+1 .. F-1) holds the bytes of one call: a video may be fed as it arrives.
 * Resolve: where count > 0, v = f32(sum / wsum);  float32 output: v;  uint8 output: 0 if v is a NaN, otherwise
 * min(max(rint(v), 0), 255), rint half to even: -0.5 gives 0, 254.5 gives 254, 255.5 and everything above (+inf too) 255,
 * everything below -0.5 (-inf too) 0.  Elsewhere 0.  The state is not changed.  The resolve saturates because v need not lie
 * in [0, 255]: an exposure takes a sample anywhere, and the u8 flag here is the output's, so a state accumulated from float32
 * frames can be resolved to bytes.  The warps and the interpolation convert with a bare rintf and need no clamp: a bilinear
 * sample of bytes, and a + t (b - a) with a, b such samples and 0 < t < 1, each operation rounded to nearest, lies in
 * [0, 255] to within a float32 rounding, far inside the (-0.5, 255.5) that rintf takes to a byte
 * (tests/test_byte_range_cpu.py checks it on frames of 0 and 255).
 * Refusals, before any device call: T < 1 (the sequence call: T < 2), an anchor outside [0, T-1], an extent that is not finite
 * and positive, F < 1, H or W < 2, Hc or Wc < 1, an unknown blend, NULL pointers (d_counts, d_held, d_skip, d_count and the
 * sequence call's outputs after `canvas` may be NULL; d_model when T == 1), a map or chain output that is not 8-byte aligned, a
 * state that is too small or not 256-byte aligned: OFLK_ERR_INVALID;  a frame or a canvas of 2^30 pixels or more, a canvas
 * that reaches 2^30 from the origin: OFLK_ERR_UNSUPPORTED.  Bundle adjustment of the chain (its drift grows with the distance
 * from the anchor) is not offered;  exposure compensation is the _exposure forms below, the temporal median
 * oflk_mosaic_median further down. */
#define OFLK_MOSAIC_MEAN 0
#define OFLK_MOSAIC_FEATHER 1
#define OFLK_MOSAIC_FIRST 2
#define OFLK_MOSAIC_LAST 3
/* device form, one launch (one block, a lane for each side of the anchor), no workspace, asynchronous on `stream`; can be
 * captured into a graph */
int oflk_mosaic_chain(const float *d_model, const int *d_counts, int T, int anchor, int H, int W, double extent,
                      double *d_from_anchor, double *d_to_anchor, double *d_box, unsigned char *d_held, unsigned char *d_dropped,
                      void *stream);
/* host arrays, synchronous */
int oflk_mosaic_chain_host(const float *model, const int *counts, int T, int anchor, int H, int W, double extent,
                           double *from_anchor, double *to_anchor, double *box, unsigned char *held, unsigned char *dropped);
/* host only, no device call: the canvas of the boxes that are not dropped.  A box that is not finite: OFLK_ERR_INVALID */
int oflk_mosaic_canvas(const double *box, const unsigned char *dropped, int T, int *x0, int *y0, int *Wc, int *Hc);
/* bytes of the state of an Hc x Wc canvas; 0 for a canvas that is refused.  Host only */
size_t oflk_mosaic_state_bytes(int Hc, int Wc);
/* device form, one launch: adds the F frames d_frames [F][H][W] (uint8 when u8) under d_map [F][9] float64 to d_state
 * (256-byte aligned, state_bytes >= oflk_mosaic_state_bytes);  d_skip [F] bytes or NULL.  Asynchronous on `stream`. */
int oflk_mosaic_accumulate(const void *d_frames, int u8, int F, int H, int W, const double *d_map, const unsigned char *d_skip,
                           int x0, int y0, int Hc, int Wc, int blend, void *d_state, size_t state_bytes, void *stream);
/* device form, one launch: d_out [Hc][Wc] (uint8 when u8), d_count [Hc][Wc] int32 or NULL.  Asynchronous on `stream`. */
int oflk_mosaic_resolve(const void *d_state, int Hc, int Wc, int u8, void *d_out, int *d_count, void *stream);
/* host arrays, synchronous: the frames go up in chunks of at most 64 and are added to one state, which is then resolved;  the
 * cut does not show.  skip and count may be NULL */
int oflk_mosaic_composite_host(const float *frames, int F, int H, int W, const double *map, const unsigned char *skip, int x0,
                               int y0, int Hc, int Wc, int blend, float *out, int *count);
int oflk_mosaic_composite_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, const unsigned char *skip,
                                  int x0, int y0, int Hc, int Wc, int blend, unsigned char *out, int *count);
/* Exposure compensation (the statement: tests/mosaic_exposure_model.py).  The photometric alignment below gives every step
 * t -> t+1 a gain and a bias, "frame t+1 looks like g_t frame t + b_t".  oflk_exposure_chain_host composes them from the
 * anchor:  (eg_f, eb_f) takes frame f's values to the anchor's exposure, v_anchor = eg_f v_f + eb_f.  photo [T-1][2] float32
 * (NULL when T == 1), status [T-1] or NULL, exposure [T][2] float64 out.  The float32 inputs are widened first;  everything is
 * float64, every operation rounded on its own.  A step is held, that is taken as (1, 0), when its status is 0, when g or b is
 * not finite, or when g <= 0.
 *   E_anchor = (1, 0)
 *   forwards, t = anchor .. T-2:    eg_{t+1} = eg_t / g_t;     eb_{t+1} = eb_t - eg_{t+1} b_t
 *   backwards, t = anchor-1 .. 0:   eg_t = eg_{t+1} g_t;       eb_t = eg_{t+1} b_t + eb_{t+1}
 * Host only, no device call.  T < 1, an anchor outside [0, T-1], NULL pointers: OFLK_ERR_INVALID.
 * The compensated accumulation is oflk_mosaic_accumulate with one change: the float32 sample s of frame f enters the blend as
 * eg_f * f64(s) + eb_f, one multiply and one add, each rounded (d_exposure [F][2] float64, 8-byte aligned; NULL:
 * OFLK_ERR_INVALID).  The cull, the four blends, the counts and the resolve are unchanged, and so are the refusals.  A frame
 * darker than the anchor has eg_f > 1 and takes a highlight above 255, a negative eb_f takes a shadow below 0: the uint8
 * resolve saturates such a pixel to 255 or 0 by the rule above, it does not wrap.  One gain
 * and one bias per frame: per-channel gains (colour frames use the luma's pair for every channel), gamma and vignetting are
 * not modelled. */
int oflk_exposure_chain_host(const float *photo, const int *status, int T, int anchor, double *exposure);
int oflk_mosaic_accumulate_exposure(const void *d_frames, int u8, int F, int H, int W, const double *d_map,
                                    const unsigned char *d_skip, const double *d_exposure, int x0, int y0, int Hc, int Wc, int blend,
                                    void *d_state, size_t state_bytes, void *stream);
int oflk_mosaic_composite_exposure_host(const float *frames, int F, int H, int W, const double *map, const unsigned char *skip,
                                        const double *exposure, int x0, int y0, int Hc, int Wc, int blend, float *out, int *count);
int oflk_mosaic_composite_exposure_host_u8(const unsigned char *frames, int F, int H, int W, const double *map,
                                           const unsigned char *skip, const double *exposure, int x0, int y0, int Hc, int Wc,
                                           int blend, unsigned char *out, int *count);
/* The temporal median: the blend that drops what moves through (the statement: tests/mosaic_median_model.py).  The four
 * blends above paint an object that moves on its own into the canvas;  the median of a pixel's samples does not, wherever the
 * background is seen in more than half of the frames that cover the pixel.  It needs every sample of a pixel at once, so it
 * is no fifth blend of the accumulate / resolve pair but a call of its own with all F frames resident and no state.
 * Canvas pixel coordinates, w, xs, ys, inside and the float32 bilinear sample s of frame f are oflk_mosaic_accumulate's;
 * frames with skip[f] != 0 take no part.
 *   value     e = s;  with an exposure e = f32(eg_f * f64(s) + eb_f): the product rounded, then the sum, then to float32
 *   order     ascending by the uint32 key of e's bits b:  key = ~b when the sign bit is set, else b ^ 0x80000000, which is
 *             -NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN.  Equal keys are equal bytes, so ties cannot show,
 *             and the result does not depend on the frame order, on the selection method or on the launch geometry
 *   median    n = the number of covering frames, e_(0) <= .. <= e_(n-1) in that order.  n odd: v = e_((n-1)/2);  n even:
 *             v = f32((f64(e_(n/2-1)) + f64(e_(n/2))) * 0.5), so inf + -inf is a NaN;  n == 0: v = 0
 *   store     float32: v;  uint8: the resolve's saturating conversion of v (254.5 gives 254, a NaN 0);  count = n
 * (The sign of a NaN that an operation makes of other values -- inf * 0 in the sample, inf - inf -- is the hardware's;  a NaN
 * that comes in with a frame or an exposure keeps its own.)
 * u8 is the type of both the frames and the output.  One launch, no workspace, no atomics;  asynchronous on `stream`.  A pixel
 * keeps its oflk_mosaic_median_capacity() smallest samples on chip (host only, no device call), which holds the median of up
 * to twice as many frames less one;  a pixel covered by more gives the same bytes, more slowly: the frames are gathered again,
 * once for every further capacity's worth of samples below the median.
 * Refusals, before any device call, those of oflk_mosaic_accumulate without the blend: F < 1, H or W < 2, Hc or Wc < 1, NULL
 * frames, map or output, a map or exposure that is not 8-byte aligned: OFLK_ERR_INVALID;  a frame or a canvas of 2^30 pixels
 * or more: OFLK_ERR_UNSUPPORTED.  d_skip, d_exposure ([F][2] float64 (eg, eb)) and d_count may be NULL.  The host forms
 * upload all F frames at once -- the price of a median -- and return OFLK_ERR_NOMEM when the device cannot hold them.
 * A weighted median, a vector median for colour and a sequence call are not offered. */
int oflk_mosaic_median_capacity(void);
int oflk_mosaic_median(const void *d_frames, int u8, int F, int H, int W, const double *d_map, const unsigned char *d_skip,
                       const double *d_exposure, int x0, int y0, int Hc, int Wc, void *d_out, int *d_count, void *stream);
int oflk_mosaic_median_host(const float *frames, int F, int H, int W, const double *map, const unsigned char *skip,
                            const double *exposure, int x0, int y0, int Hc, int Wc, float *out, int *count);
int oflk_mosaic_median_host_u8(const unsigned char *frames, int F, int H, int W, const double *map, const unsigned char *skip,
                               const double *exposure, int x0, int y0, int Hc, int Wc, unsigned char *out, int *count);
/* Frames in, mosaic out.  By statement, byte for byte: oflk_pyramidal_sequence_klt_sparse_replenish on the frames,
 * oflk_tracks_homography on its rows with t0 = 0, oflk_mosaic_chain and oflk_mosaic_canvas, then oflk_mosaic_accumulate of all
 * frames under from_anchor with skip = dropped and the canvas's x0, y0, and oflk_mosaic_resolve.  Pass 1 is the replenish
 * call's chunk loop; the fit and the chain run on the rows; the boxes and flags come down for the canvas; pass 2 sends the
 * frames up again in chunks.  canvas [4] receives x0, y0, Wc, Hc;  out has room for `capacity` pixels: when Wc * Hc exceeds it
 * the call returns OFLK_ERR_UNSUPPORTED with canvas written, else out (and count) hold [Hc][Wc] packed.  count [capacity],
 * to_anchor [T][9], held [T-1], dropped [T], model_out [T-1][9], counts_out [T-1][3]: each may be NULL.  The call refuses
 * whatever its parts refuse, with their codes. */
int oflk_mosaic_sequence(const float *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha, float beta,
                         float max_residual, float quality_level, float min_distance, int max_corners, int detect_every,
                         int hypotheses, float threshold, unsigned seed, int anchor, double extent, int blend, float *out,
                         size_t capacity, int *canvas, int *count, double *to_anchor, unsigned char *held, unsigned char *dropped,
                         float *model_out, int *counts_out);
int oflk_mosaic_sequence_u8(const unsigned char *frames, int T, int H, int W, int levels, int window_size, int iters, float alpha,
                            float beta, float max_residual, float quality_level, float min_distance, int max_corners,
                            int detect_every, int hypotheses, float threshold, unsigned seed, int anchor, double extent, int blend,
                            unsigned char *out, size_t capacity, int *canvas, int *count, double *to_anchor, unsigned char *held,
                            unsigned char *dropped, float *model_out, int *counts_out);

/* ---- direct image alignment: step models refined on pixel intensities -------------------------------------------------- */
/* The statement (tests/align_model.py).  Inverse-compositional Lucas-Kanade registration of frame B to the template A over the
 * whole frame, coarse to fine, from a given step model (the RANSAC fits': model[t] maps frame t's coordinates to frame t+1's,
 * as oflk_warp_perspective(frames[t+1], model[t]) reads it).  The residual at pixel x of A is r(x) = B(M x) - A(x).  Every
 * operation is float64 unless stated and rounded on its own, in the order written; nothing is contracted, there is no atomic
 * and no result depends on the launch geometry or on how the steps are cut into calls.  The device equals it byte for byte, a
 * NaN equal to a NaN.  L = levels, n = iterations, NP = 6 parameters (OFLK_ALIGN_AFFINE, six float32 [a00 a01 tx; a10 a11 ty])
 * or 8 (OFLK_ALIGN_HOMOGRAPHY, nine float32 with [2][2] == 1);  both are carried as nine float64, an affine model with the
 * third row (0, 0, 1).
 *   refused step   status_in[s] == 0 or a model entry that is not finite: the model's bytes, status 0, stats four zeros
 *   pyramids       oflk_build_pyramid's levels (scale 0.5) of A and B as float32, uint8 frames converted first;  level 0 is
 *                  the coarsest, level L-1 the frame;  level l has H_l x W_l pixels
 *   sums(l, M)     for every pixel (x, y) of level l:  w = (m6 x + m7 y) + m8;  xs = ((m0 x + m1 y) + m2) / w;
 *                  ys = ((m3 x + m4 y) + m5) / w (the perspective warp's);  counted = w > 0 and 0 <= xs <= W_l - 1 and
 *                  0 <= ys <= H_l - 1, a NaN anywhere meaning not counted;  r = f64(sample(B_l, xs, ys) - A_l[y][x]), the
 *                  difference in float32;  Gx, Gy = oflk_compute_gradients(A_l, A_l)'s Ix, Iy as float64 (Sobel / 8, the
 *                  border clamped; a true convolution, so minus the derivatives);  xh = (x - cx) / s, yh = (y - cy) / s with
 *                  cx = (W_l - 1) / 2, cy = (H_l - 1) / 2, s = max(W_l, H_l) / 2;
 *                  sd = [Gx xh, Gx yh, Gx, Gy xh, Gy yh, Gy, -(t xh), -(t yh)], t = sd[0] + sd[4] (affine: the first six).
 *                  The NS = NP (NP + 1) / 2 + NP + 2 sums over the counted pixels (46 or 29):  sd[i] sd[j] for i = 0 .. NP-1,
 *                  j = i .. NP-1;  sd[i] r;  r r;  1.0 (the count)
 *   order          the level is cut into tiles of 64 columns by 32 rows from the origin.  In a tile, a column's partial starts
 *                  at +0.0 and adds its counted pixels top to bottom;  the 64 partials are combined by the motion fit's tree
 *                  (for stride 32, 16, .., 1: partial[c] += partial[c + stride] for c < stride);  the total starts at +0.0
 *                  and adds the tile sums one after another in raster order
 *   before         e0 / c0, the r r sum and the count of sums(L-1, M) under the input model
 *   level l        for l = 0 .. L-1, unless the step is frozen:  sx = W_l / W, sy = H_l / H;  M_l = D M D^-1:
 *                  [m0, (m1 sx) / sy, m2 sx;  (m3 sy) / sx, m4, m5 sy;  m6 / sx, m7 / sy, m8];  then n iterations;  then back:
 *                  [m0, (m1 sy) / sx, m2 / sx;  (m3 sx) / sy, m4, m5 / sy;  m6 sx, m7 sy, m8]
 *   iteration      S = sums(l, M_l).  [G | b]: G the symmetric matrix of the sd sd sums, b the sd r sums, eliminated without
 *                  pivoting by the homography refit's procedure on NP rows: q.  p = -(q / s) (the gradients' sign).
 *                  P = [p0 p1 p2; p3 p4 p5; p6 p7 0] (affine: p6 = p7 = 0);  A[r][0] = P[r][0] / s, A[r][1] = P[r][1] / s,
 *                  A[r][2] = P[r][2] - (A[r][0] cx + A[r][1] cy);  D[0][c] = s A[0][c] + cx A[2][c],
 *                  D[1][c] = s A[1][c] + cy A[2][c], D[2][c] = A[2][c];  dM = D with 1.0 added to the diagonal;
 *                  I = adj(dM) / adj(dM)[2][2] (the mosaic chain's cofactors, nine divisions);
 *                  N[r][c] = (M_l[r][0] I[0][c] + M_l[r][1] I[1][c]) + M_l[r][2] I[2][c];  M_l = N, one more accepted update
 *   freezing       the iteration is skipped and the step freezes with its M_l, which goes back to the frame at once and is
 *                  not touched again, when the count < f64(min_share) * f64(W_l H_l), a pivot is zero or not finite, an
 *                  entry of N is not finite, or (n6 x + n7 y) + n8 > 0 fails at a corner (0,0), (W_l-1,0), (W_l-1,H_l-1),
 *                  (0,H_l-1) of the level
 *   outputs        e1, c1 of sums(L-1, M) under the final model;  stats[s] = [e0 / c0, e1 / c1, c1 / f64(W H), accepted];
 *                  no accepted update: the input model's bytes, status 0;  not e1 / c1 <= e0 / c0 (a NaN on either side
 *                  included): the input model's bytes, status 2 (rejected);  else status 1 and the model as float32: affine m0 .. m5, homography m_k / m8
 * Refusals, before any device call: S < 1 (the sequence calls: T < 2), H or W < 1, iterations < 1, min_share outside (0, 1],
 * an unknown model, levels outside [1, OFLK_MAX_LEVELS], NULL pointers (d_status_in / status_in may be NULL: every step
 * refined), a workspace that is too small or not 256-byte aligned, d_stats not 8-byte aligned: OFLK_ERR_INVALID;  frames of
 * 2^30 pixels or more, levels whose coarsest would be smaller than 8 x 8: OFLK_ERR_UNSUPPORTED.  Early exit on a small
 * update, the ECC normalisation and translation and similarity models are not offered;  robust weights are the robust form's,
 * below. */
#define OFLK_ALIGN_AFFINE 0
#define OFLK_ALIGN_HOMOGRAPHY 1
/* bytes of the workspace of S steps (the sequence call: S = T - 1).  Host only */
int oflk_align_workspace(int S, int H, int W, int levels, int model, size_t *bytes);
/* device form: d_a, d_b [S][H][W] (uint8 when u8), d_model_in, d_model_out [S][6 | 9] float32, d_status_in [S] int32 or NULL,
 * d_status_out [S] int32, d_stats [S][4] float64.  The pyramids, then two launches per iteration and per residual, all
 * asynchronous on `stream` with no host round trip; can be captured into a graph (one chain, no parallel branches) */
int oflk_align_refine(const void *d_a, const void *d_b, int u8, int S, int H, int W, int levels, int iterations, int model,
                      float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace, size_t workspace_bytes,
                      float *d_model_out, int *d_status_out, double *d_stats, void *stream);
/* the same on the T-1 steps t -> t+1 of d_frames [T][H][W]; every frame's pyramid is built once */
int oflk_align_sequence(const void *d_frames, int u8, int T, int H, int W, int levels, int iterations, int model, float min_share,
                        const float *d_model_in, const int *d_status_in, void *d_workspace, size_t workspace_bytes,
                        float *d_model_out, int *d_status_out, double *d_stats, void *stream);
/* host arrays, synchronous.  The steps go up in chunks of at most 64; steps are independent and a frame's pyramid depends on
 * the frame alone, so the cut does not show */
int oflk_align_refine_host(const float *a, const float *b, int S, int H, int W, int levels, int iterations, int model,
                           float min_share, const float *model_in, const int *status_in, float *model_out, int *status_out,
                           double *stats);
int oflk_align_refine_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int levels, int iterations,
                              int model, float min_share, const float *model_in, const int *status_in, float *model_out,
                              int *status_out, double *stats);
int oflk_align_sequence_host(const float *frames, int T, int H, int W, int levels, int iterations, int model, float min_share,
                             const float *model_in, const int *status_in, float *model_out, int *status_out, double *stats);
int oflk_align_sequence_host_u8(const unsigned char *frames, int T, int H, int W, int levels, int iterations, int model,
                                float min_share, const float *model_in, const int *status_in, float *model_out, int *status_out,
                                double *stats);

/* The photometric form (the statement: tests/align_photo_model.py): the calls above with a gain and a bias estimated beside
 * every step model, for frames whose exposure differs.  It is the statement above with what follows changed.  A step carries
 * two more float64 values, g = 1.0 and b = 0.0 at the start: "B under the model looks like g A + b".
 *   sums_photo(l, M, g, b)   counted, xs, ys, Gx, Gy, xh, yh and sd[0 .. NP-1] as above;  v = sample(B_l, xs, ys) in float32;
 *                  a = f64(A_l[y][x]);  r = f64(v) - (g a + b), formed in float64, every operation rounded on its own;  the
 *                  NQ = NP + 2 columns c = [g sd[0], .., g sd[NP-1], a, 1.0];  the NQ (NQ + 1) / 2 + NQ + 2 sums over the
 *                  counted pixels (67 or 46):  c[i] c[j] for i = 0 .. NQ-1, j = i .. NQ-1;  c[i] r;  r r;  1.0.  The order of
 *                  every sum is the one above
 *   before, after  r r / count of sums_photo(L-1, M, 1, 0) under the input model, and of sums_photo(L-1, M, g, b) under the
 *                  final model and the final g, b;  stats keeps its four entries
 *   iteration      [G | rhs] of the sums, eliminated without pivoting by the same procedure on NQ rows: q.  The geometric
 *                  update is the one above on q[0 .. NP-1];  then g' = g + q[NP], b' = b + q[NP + 1].  (Minimising
 *                  sum (r + g sd.dp - a dg - db)^2, the normal equations in c solve for [-dp, dg, db].)
 *   freezing       the four conditions above, or g' or b' not finite, or g' <= 0.  A step that freezes keeps M_l, g and b.
 *                  g and b are not rescaled between levels
 *   outputs        model, status and stats by the rules above;  photo[s] = (f32(g), f32(b)) where the status is 1, else the
 *                  bytes of (1.0f, 0.0f), a refused step included
 * d_photo_out / photo_out [S][2] float32;  NULL: OFLK_ERR_INVALID;  the other refusals are the plain calls'.  The workspace is
 * larger: oflk_align_photo_workspace.  The device forms are asynchronous on `stream` and can be captured into a graph (one
 * chain, no parallel branches).  One gain and one bias per step over the whole frame: the ECC normalisation, per-channel
 * gains and gamma are not offered;  robust weights are the robust form's, below.  The sparse tracker still assumes brightness constancy: a step whose exposure
 * change exceeds its max_residual (4 grey levels by default) ends tracks before the refinement sees the step. */
int oflk_align_photo_workspace(int S, int H, int W, int levels, int model, size_t *bytes);
int oflk_align_refine_photo(const void *d_a, const void *d_b, int u8, int S, int H, int W, int levels, int iterations, int model,
                            float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace,
                            size_t workspace_bytes, float *d_model_out, int *d_status_out, double *d_stats, float *d_photo_out,
                            void *stream);
int oflk_align_sequence_photo(const void *d_frames, int u8, int T, int H, int W, int levels, int iterations, int model,
                              float min_share, const float *d_model_in, const int *d_status_in, void *d_workspace,
                              size_t workspace_bytes, float *d_model_out, int *d_status_out, double *d_stats, float *d_photo_out,
                              void *stream);
/* host arrays, synchronous, in the plain host forms' chunks of at most 64 steps */
int oflk_align_refine_photo_host(const float *a, const float *b, int S, int H, int W, int levels, int iterations, int model,
                                 float min_share, const float *model_in, const int *status_in, float *model_out, int *status_out,
                                 double *stats, float *photo_out);
int oflk_align_refine_photo_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int levels,
                                    int iterations, int model, float min_share, const float *model_in, const int *status_in,
                                    float *model_out, int *status_out, double *stats, float *photo_out);
int oflk_align_sequence_photo_host(const float *frames, int T, int H, int W, int levels, int iterations, int model,
                                   float min_share, const float *model_in, const int *status_in, float *model_out, int *status_out,
                                   double *stats, float *photo_out);
int oflk_align_sequence_photo_host_u8(const unsigned char *frames, int T, int H, int W, int levels, int iterations, int model,
                                      float min_share, const float *model_in, const int *status_in, float *model_out,
                                      int *status_out, double *stats, float *photo_out);

/* The robust form (the statement: tests/align_robust_model.py): the plain calls (photometric == 0) or the photometric ones
 * (photometric != 0) with a Huber weight on every residual, so that what moves on its own -- a person walking through the shot
 * -- does not pull the fit: iteratively reweighted least squares.  It is the statements above with what follows changed.
 * delta = f64(robust_delta), in grey levels, one value for every level.
 *   sums_robust    counted, r, sd and the columns c as above (plain: c = sd, NQ = NP;  photometric: c = [g sd, a, 1.0],
 *                  NQ = NP + 2).  Per counted pixel:  ar = |r|;  w = ar > delta ? delta / ar : 1.0;
 *                  rho = ar > delta ? delta (ar - delta 0.5) : (r r) 0.5;  wc[i] = w c[i].  A NaN r fails the comparison:
 *                  w = 1 and the NaN poisons the sums as it does above.  The NQ (NQ + 1) / 2 + NQ + 4 sums over the counted
 *                  pixels (31 affine, 48 homography;  photometric 48, 69):  wc[i] c[j] for i = 0 .. NQ-1, j = i .. NQ-1;
 *                  wc[i] r;  r r;  1.0;  rho;  w.  The order of every sum is the one above
 *   iteration      the one above on the weighted [G | b];  the freezes and the g, b update are unchanged.  The weights come
 *                  from the current residual on every pass, at every level
 *   before, after  sum(rho) / count at full resolution under the input model (photometric: at (g, b) = (1, 0)) and under the
 *                  final model (and g, b);  status 2 when not after <= before.  rho is what the iteration minimises: a step
 *                  that moves an outlier's large residual about while it registers the rest is not rejected for it
 *   outputs        stats[s] = [mean rho before, mean rho after, c1 / f64(W H), accepted, r r / count before, r r / count
 *                  after, sum(w) / count before, sum(w) / count after], eight zeros for a refused step;  model, status and
 *                  photo by the rules above
 * A suggested robust_delta is 4 grey levels, the sparse tracker's max_residual default in the same unit;  stats[s][7], the mean
 * weight under the final model, is how a caller tunes it (1.0: nothing was down-weighted).  d_stats / stats [S][8] float64;
 * d_photo_out / photo_out [S][2] float32 when photometric, otherwise NULL (it is not written).  The workspace is
 * oflk_align_robust_workspace's.  Refusals, before any device call: robust_delta not finite or <= 0, photometric without
 * d_photo_out: OFLK_ERR_INVALID;  and the plain calls'.  The device forms are asynchronous on `stream` and can be captured into
 * a graph (one chain, no parallel branches).  A scale estimated from the data and redescending weights are not offered. */
int oflk_align_robust_workspace(int S, int H, int W, int levels, int model, int photometric, size_t *bytes);
int oflk_align_refine_robust(const void *d_a, const void *d_b, int u8, int S, int H, int W, int levels, int iterations, int model,
                             float min_share, float robust_delta, int photometric, const float *d_model_in,
                             const int *d_status_in, void *d_workspace, size_t workspace_bytes, float *d_model_out,
                             int *d_status_out, double *d_stats, float *d_photo_out, void *stream);
int oflk_align_sequence_robust(const void *d_frames, int u8, int T, int H, int W, int levels, int iterations, int model,
                               float min_share, float robust_delta, int photometric, const float *d_model_in,
                               const int *d_status_in, void *d_workspace, size_t workspace_bytes, float *d_model_out,
                               int *d_status_out, double *d_stats, float *d_photo_out, void *stream);
/* host arrays, synchronous, in the plain host forms' chunks of at most 64 steps */
int oflk_align_refine_robust_host(const float *a, const float *b, int S, int H, int W, int levels, int iterations, int model,
                                  float min_share, float robust_delta, int photometric, const float *model_in,
                                  const int *status_in, float *model_out, int *status_out, double *stats, float *photo_out);
int oflk_align_refine_robust_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int levels,
                                     int iterations, int model, float min_share, float robust_delta, int photometric,
                                     const float *model_in, const int *status_in, float *model_out, int *status_out,
                                     double *stats, float *photo_out);
int oflk_align_sequence_robust_host(const float *frames, int T, int H, int W, int levels, int iterations, int model,
                                    float min_share, float robust_delta, int photometric, const float *model_in,
                                    const int *status_in, float *model_out, int *status_out, double *stats, float *photo_out);
int oflk_align_sequence_robust_host_u8(const unsigned char *frames, int T, int H, int W, int levels, int iterations, int model,
                                       float min_share, float robust_delta, int photometric, const float *model_in,
                                       const int *status_in, float *model_out, int *status_out, double *stats, float *photo_out);
/* The weight map of S steps at full resolution: weights[s][y][x] = f32(w) of sums_robust at the counted pixels of step s under
 * model[s] [6 | 9] float32 (no pyramid, no iteration), 0.0f elsewhere;  low values mark what moved on its own.  photo [S][2]
 * float32 gains and biases (the photometric residual, g = f64(photo[s][0]), b = f64(photo[s][1])) or NULL (the plain one).
 * Refusals: S, H, W < 1, an unknown model, robust_delta not finite or <= 0, NULL pointers: OFLK_ERR_INVALID;  frames of 2^30
 * pixels or more: OFLK_ERR_UNSUPPORTED.  The device form is one asynchronous launch on `stream` */
int oflk_align_weights(const void *d_a, const void *d_b, int u8, int S, int H, int W, int model, float robust_delta,
                       const float *d_model, const float *d_photo, float *d_weights, void *stream);
int oflk_align_weights_host(const float *a, const float *b, int S, int H, int W, int model, float robust_delta,
                            const float *model_in, const float *photo, float *weights);
int oflk_align_weights_host_u8(const unsigned char *a, const unsigned char *b, int S, int H, int W, int model, float robust_delta,
                               const float *model_in, const float *photo, float *weights);

/* ---- online video stabilisation: a fixed-lag stabiliser on the tracker --------------------------------------------------- */
/* The statement (tests/stabilize_online_model.py) is the trajectory above, read in the order in which a stream delivers its
 * steps.  The window of frame f is r_f = min(r, f, T-1-f) and reads steps f - r_f .. f + r_f - 1 only, so frame f is final
 * once frame f + r has been pushed, and the last r frames are final once the stream is known to have ended.  A stabiliser
 * of radius r therefore emits frame t - r on the push of frame t >= r (lag = r frames) and the remaining min(r, T) frames,
 * ascending, on a flush, which supplies the true T.  By statement, byte for byte: the frames and corrections of T pushes
 * and a flush are `out` and `correction` of oflk_stabilize_sequence[_u8] on the same T frames with the same arguments
 * (that call wants T >= 2 and detect_every >= 1; the stabiliser also takes one frame, and detect_every = 0).  A slot filled
 * by a detection on the last pushed frame does not count: its born mark keeps it out of the step into that frame, which is
 * what the sequence call, which never detects on its last frame, sees as a dead slot.  With r = 0 every push emits its own
 * frame under the identity.
 * oflk_stabilize_trajectory_ring is the trajectory of n consecutive frames f0 .. f0 + n - 1 whose steps lie in a ring: step
 * s at slot s % cap of d_model_ring [cap][6] float32 and d_counts_ring [cap][3] int32 (or NULL), cap >= max(2 r, 1).
 * T = -1: the stream is open, r_f = min(r, f) and n = 1; T >= 0: r_f = min(r, f, T-1-f) and f0 + n <= T.  Only the slots of
 * steps f - r_f .. f + r_f - 1 are read.  d_correction [n][6], d_map [n][6] as oflk_stabilize_trajectory's rows f0 ..
 * f0 + n - 1, every value formed by the same operations in the same order.  One launch, one block per frame (the window's
 * inversions side by side, the two chains on two lanes), the weights in the launch arguments; asynchronous; can be captured.
 *
 * State of a stabiliser: a tracker with its motion row on (its state is listed there), a delay line of r + 1 frames in the
 * input pixel type -- (r + 1) H W pixels, 33 MB for 1080p bytes at r = 15 --, the ring of 2 r step models and counts, and r
 * rows of correction and map.  Creation checks the configuration and makes no device call; the first push allocates all of
 * it and no later push allocates.  The host forms stage one frame and one mask on the device; those two planes come with
 * the first host call.  oflk_stabilizer_workspace_bytes counts everything, the inner tracker included.
 * A push of frame t enqueues on the one stream: the frame copied into delay slot t % (r + 1); the tracker's push of that
 * slot, whose fit (t >= 1) writes step t-1 straight into ring slot (t-1) % cap; and for t >= r the trajectory of frame
 * t - r (one launch) and one oflk_warp_affine launch of its delay slot into d_out.  A flush enqueues one trajectory launch
 * for its frames and at most two warp launches (the delay line wraps once).  Nothing synchronises in the device forms.
 * Pushes are enqueued from host-side state, so they are not made for graph capture (as the tracker's).  A push or flush
 * that fails part-way leaves the frame index as it was, and every later push is refused with OFLK_ERR_INVALID until
 * oflk_stabilizer_reset.  After a flush (also one that had nothing to emit) every push is refused with OFLK_ERR_INVALID
 * until oflk_stabilizer_reset; a second flush emits nothing.  A stabiliser is single-stream: every call on it is ordered by
 * the caller.
 * Refusals, before any device call: what oflk_tracker_create refuses about device, shape, window, levels, iterations,
 * alpha, beta, max_residual, quality_level, min_distance, max_corners and detect_every, what oflk_tracker_set_motion refuses
 * about model (a model is required: model < 0 is OFLK_ERR_INVALID), hypotheses and threshold, and what
 * oflk_stabilize_trajectory refuses about weights and radius, with their codes; H or W < 2: OFLK_ERR_INVALID.  A NULL
 * stabiliser, frame, output, `emitted`, `first` or `count` (d_inside, inside and correction may be NULL; the flush's output
 * when nothing is left), float32 device frames not 4-byte aligned, correction_device before the first emission:
 * OFLK_ERR_INVALID.  oflk_stabilize_trajectory_ring: the window's refusals, cap < max(2 radius, 1), n < 1 or n > 128,
 * f0 < 0, T < -1, T >= 0 with f0 + n > T, T = -1 with n != 1, NULL pointers (d_counts_ring may be NULL), d_map not 8-byte
 * aligned: OFLK_ERR_INVALID. */
typedef struct oflk_stabilizer oflk_stabilizer;
int oflk_stabilize_trajectory_ring(const float *d_model_ring, const int *d_counts_ring /* may be NULL */, int cap, int f0, int n,
                                   int T /* -1: the stream is open */, const double *weights /* host, [radius + 1] */, int radius,
                                   float *d_correction /* [n][6] */, double *d_map /* [n][6] */, void *stream);
int oflk_stabilizer_create(oflk_stabilizer **st, int device, int H, int W, int u8, int levels, int window_size, int iters,
                           float alpha, float beta, float max_residual, float quality_level, float min_distance,
                           int max_corners, int detect_every, int model, int hypotheses, float threshold, unsigned seed,
                           const double *weights /* host, [radius + 1], copied */, int radius);
int oflk_stabilizer_destroy(oflk_stabilizer *st);
int oflk_stabilizer_reset(oflk_stabilizer *st, void *stream);      /* frame index -1, the inner tracker reset, pushes taken again */
size_t oflk_stabilizer_workspace_bytes(const oflk_stabilizer *st); /* what is allocated at the moment, the tracker's included */
int oflk_stabilizer_lag(const oflk_stabilizer *st);                /* = radius: frame t - lag comes out of the push of frame t */
int oflk_stabilizer_frame_index(const oflk_stabilizer *st);        /* index of the last pushed frame, -1 before the first */
/* device frame [H][W] in, the steadied frame *emitted = t - r into d_out [H][W] (and d_inside [H][W] bytes, may be NULL) when
 * t >= r; else *emitted = -1 and neither is written.  *emitted is known on the host when the call returns.  Asynchronous
 * on `stream`, no host synchronisation */
int oflk_stabilizer_push_device(oflk_stabilizer *st, const void *d_frame, void *d_out, unsigned char *d_inside, int *emitted,
                                void *stream);
/* host frame in, host frame out (and inside, and the emitted frame's correction [6]; both may be NULL), through the staged
 * planes on the null stream; synchronous */
int oflk_stabilizer_push(oflk_stabilizer *st, const void *frame, void *out, unsigned char *inside, float *correction,
                         int *emitted);
/* the stream has ended: the *count = min(r, T) frames not yet emitted, *first .. *first + *count - 1, into d_out
 * [radius][H][W] (and d_inside, may be NULL) with the true T.  *count is 0 before any push and after a flush */
int oflk_stabilizer_flush_device(oflk_stabilizer *st, void *d_out, unsigned char *d_inside, int *first, int *count, void *stream);
/* host arrays: out [radius][H][W], inside (may be NULL), correction [radius][6] (may be NULL); synchronous */
int oflk_stabilizer_flush(oflk_stabilizer *st, void *out, unsigned char *inside, float *correction, int *first, int *count);
/* device pointers (each may be NULL) to the rows of the last emission -- one row after a push, *count after a flush --,
 * valid until the next push, flush or reset: correction [rows][6] float32, map [rows][6] float64 */
int oflk_stabilizer_correction_device(const oflk_stabilizer *st, const float **d_correction, const double **d_map);
/* The inner tracker, owned by the stabiliser, for oflk_tracker_row_device / read_row / motion_device / read_motion /
 * add_points / frame_index: the row and the step's motion of the last pushed frame (not of the emitted one).  Pushing it,
 * resetting it, destroying it or changing its motion directly is the caller's error: the stabiliser's frames and steps
 * would no longer be the tracker's. */
oflk_tracker *oflk_stabilizer_tracker(oflk_stabilizer *st);

/* ---- colour video: luma, warps of interleaved frames, colour stabilisers ------------------------------------------------- */
/* The statement (tests/colour_model.py).
 * Layout: colour frames are interleaved uint8, [F][H][W][C] with C = channels = 3 or 4 ("packed" below).  float32 colour is
 * not offered.  `order` says where R, G and B sit: OFLK_ORDER_RGB = R, G, B at bytes 0, 1, 2; OFLK_ORDER_BGR = B, G, R.
 * The byte at index 3 when C = 4 is a fourth channel: luma ignores it, every warp resamples it like the others.
 * Luma: Y = (77 R + 150 G + 29 B + 128) >> 8 in integers.  The weights sum to 256, so grey input (R = G = B = g) gives
 * Y = g and Y never leaves [0, 255]; there is no float arithmetic and nothing to round.
 * Packed warps: for every channel c, out[f][y][x][c] is the byte that oflk_warp_affine / oflk_warp_perspective writes at
 * [f][y][x] for the plane frames[f][:, :, c] under map[f] -- (unsigned char) rintf(sample), 0 outside the frame -- and
 * inside[f][y][x] is that call's inside: one byte per pixel, not per channel.  The kernels form the source position, the
 * test and the four weights once per pixel and finish C channels on them, by the planar kernels' operations in their order.
 * No load touches a byte outside [F][H][W][C].
 * Colour stabilisation, by statement, byte for byte: (1) the luma of every frame; (2) oflk_stabilize_sequence_u8 on the
 * luma frames for correction, model_out, counts_out and held; (3) the packed affine warp of the colour frames under the
 * maps of that trajectory.  The sequence call takes the luma in a chunked pass of its own (a chunk of packed frames goes
 * up, its luma comes down into a host array of T H W bytes), runs the grey call's pass 1 and trajectory on that array and
 * warps the packed frames chunk by chunk: nothing of the sequence's size is ever on the device.
 * The online form: a stabiliser made by oflk_stabilizer_create_packed holds packed frames in its delay line --
 * (r + 1) H W C bytes, counted by oflk_stabilizer_workspace_bytes with one more plane for the luma -- and its tracker is
 * pushed the luma of each frame, computed on the device inside the push (one more launch).  oflk_stabilizer_push, flush,
 * their _device forms, correction_device, lag, reset and destroy then take and return [H][W][C] frames for such an
 * object; d_inside / inside stays [H][W].  The frames and corrections of T pushes and a flush equal
 * oflk_stabilize_sequence_packed on the same T frames.  A stabiliser made by oflk_stabilizer_create is what it was.
 * Refusals, before any device call: channels not 3 or 4, an order outside the two values, NULL pointers (d_inside, inside
 * and the sequence call's last four outputs may be NULL), H or W < 2, F < 1 (the sequence call: T < 2), d_map not 8-byte
 * aligned: OFLK_ERR_INVALID;  frames of 2^30 pixels or more: OFLK_ERR_UNSUPPORTED.  Byte offsets inside a frame are 32-bit,
 * so frames of H W C >= 2^31 bytes are refused as well, with OFLK_ERR_UNSUPPORTED; offsets across frames are 64-bit.  The
 * sequence call and the stabiliser also refuse what their grey forms refuse, with their codes.  Frames and outputs may
 * have any alignment (an unaligned base or W % 4 != 0 runs the element-wise kernels). */
#define OFLK_ORDER_RGB 0
#define OFLK_ORDER_BGR 1
/* device form, one launch: d_frames [F][H][W][C] -> d_luma [F][H][W].  Asynchronous on `stream`. */
int oflk_luma_u8(const unsigned char *d_frames, int F, int H, int W, int channels, int order, unsigned char *d_luma, void *stream);
/* host arrays, synchronous, in chunks of at most 64 frames */
int oflk_luma_u8_host(const unsigned char *frames, int F, int H, int W, int channels, int order, unsigned char *luma);
/* device forms, one launch for the F frames: d_frames, d_out [F][H][W][C], d_map [F][6] (perspective: [F][9]) float64,
 * d_inside [F][H][W] bytes or NULL.  Asynchronous on `stream`. */
int oflk_warp_affine_packed(const unsigned char *d_frames, int F, int H, int W, int channels, const double *d_map,
                            unsigned char *d_out, unsigned char *d_inside, void *stream);
int oflk_warp_perspective_packed(const unsigned char *d_frames, int F, int H, int W, int channels, const double *d_map,
                                 unsigned char *d_out, unsigned char *d_inside, void *stream);
/* host arrays, synchronous, in chunks of at most 64 frames; the result does not depend on the cut */
int oflk_warp_affine_packed_host(const unsigned char *frames, int F, int H, int W, int channels, const double *map,
                                 unsigned char *out, unsigned char *inside);
int oflk_warp_perspective_packed_host(const unsigned char *frames, int F, int H, int W, int channels, const double *map,
                                      unsigned char *out, unsigned char *inside);
/* oflk_stabilize_sequence_u8's arguments with packed frames in and out: frames, out [T][H][W][C] */
int oflk_stabilize_sequence_packed(const unsigned char *frames, int T, int H, int W, int channels, int order, int levels,
                                   int window_size, int iters, float alpha, float beta, float max_residual, float quality_level,
                                   float min_distance, int max_corners, int detect_every, int model, int hypotheses,
                                   float threshold, unsigned seed, const double *weights, int radius, unsigned char *out,
                                   float *correction, float *model_out, int *counts_out, unsigned char *held);
/* oflk_stabilizer_create's arguments with channels and order in place of u8 */
int oflk_stabilizer_create_packed(oflk_stabilizer **st, int device, int H, int W, int channels, int order, int levels,
                                  int window_size, int iters, float alpha, float beta, float max_residual, float quality_level,
                                  float min_distance, int max_corners, int detect_every, int model, int hypotheses, float threshold,
                                  unsigned seed, const double *weights /* host, [radius + 1], copied */, int radius);

/* ---- NV12 video: one fused two-plane warp, NV12 stabilisers ---------------------------------------------------------------- */
/* The statement (tests/nv12_model.py).
 * Layout: an NV12 frame is H W 3 / 2 contiguous bytes: Y[H][W] first, then UV[H/2][W/2][2] with U at byte 0 and V at byte 1 of
 * a pair; H and W are even and at least 4; frames are contiguous, [F][H W 3 / 2] (oflk_nv12_frame_bytes).  Pitched surfaces
 * and separate plane pointers are not offered.
 * Siting: `siting` says where chroma sample (column i, row j) sits in luma coordinates, x = 2 i + sx, y = 2 j + sy:
 * OFLK_SITING_LEFT = (sx, sy) = (0, 0.5), the H.264 / HEVC default; OFLK_SITING_CENTER = (0.5, 0.5), as in JPEG and MPEG-1.
 * The chroma map, float64, every operation rounded on its own, in this order:
 *   c2 = (m0 sx + m1 sy) + m2,  c5 = (m3 sx + m4 sy) + m5,  perspective only: c8 = (m6 sx + m7 sy) + m8
 *   affine:      mc = [m0, m1, 0.5 (c2 - sx);  m3, m4, 0.5 (c5 - sy)]
 *   perspective: mc = [m0 - sx m6, m1 - sx m7, 0.5 (c2 - sx c8);  m3 - sy m6, m4 - sy m7, 0.5 (c5 - sy c8);  2 m6, 2 m7, c8]
 * the luma map conjugated by the siting: a chroma sample is fetched from where its own luma position is fetched from.
 * The warp: the Y plane of out[f] is the bytes oflk_warp_affine / oflk_warp_perspective (u8) writes for the plane Y[f] under
 * map[f], and inside[f] [H][W] is that call's inside.  U and V of out[f] are, per channel, the bytes the same planar warp
 * writes for the H/2 x W/2 plane UV[f][:, :, c] under mc, except that where that warp's own inside is 0 the chroma byte is
 * 128, not 0: zero chroma is saturated green, and Y = 0 with U = V = 128 is black.  Nothing else differs from the planar
 * statement.  Both planes of all F frames are one launch; no load touches a byte outside its own frame.
 * NV12 stabilisation, by statement, byte for byte: (1) oflk_stabilize_sequence_u8 on the Y planes for correction, model_out,
 * counts_out and held; (2) the NV12 affine warp of the frames under the maps of that trajectory.  The sequence call gathers
 * the Y planes into a host array of T H W bytes (no device work), runs the grey call's pass 1 and trajectory on it and warps
 * the NV12 frames chunk by chunk.
 * The online form: a stabiliser made by oflk_stabilizer_create_nv12 holds (r + 1) NV12 frames in its delay line, and its
 * tracker is pushed the frame's own first H W bytes: there is no luma launch and no luma plane.  oflk_stabilizer_push, flush,
 * their _device forms, correction_device, lag, reset, workspace_bytes and destroy then take and return frames of H W 3 / 2
 * bytes for such an object; d_inside / inside stays [H][W].  The frames and corrections of T pushes and a flush equal
 * oflk_stabilize_sequence_nv12 on the same T frames.  Grey and packed stabilisers are what they were.
 * Refusals, before any device call: H or W odd or below 4, a siting outside the two values, F < 1 (the sequence call: T < 2),
 * NULL pointers (d_inside, inside and the sequence call's last four outputs may be NULL), d_map not 8-byte aligned:
 * OFLK_ERR_INVALID;  H W >= 2^30: OFLK_ERR_UNSUPPORTED.  Byte offsets inside a frame are 32-bit, offsets across frames 64-bit.
 * The sequence call and the stabiliser also refuse what their grey forms refuse, with their codes.  Frames and outputs may
 * have any alignment: the Y plane and the mask are stored a dword a lane when W % 4 == 0 and d_out and d_inside are 4-byte
 * aligned, the UV plane 8 bytes a lane when also W % 8 == 0 and d_out is 8-byte aligned; everything else runs the
 * element-wise kernels. */
#define OFLK_SITING_LEFT 0
#define OFLK_SITING_CENTER 1
/* H W 3 / 2, or 0 for a shape the NV12 calls refuse */
size_t oflk_nv12_frame_bytes(int H, int W);
/* device forms, one launch for both planes of the F frames: d_frames, d_out [F][H W 3 / 2], d_map [F][6] (perspective:
 * [F][9]) float64, d_inside [F][H][W] bytes or NULL.  Asynchronous on `stream`, capturable. */
int oflk_warp_affine_nv12(const unsigned char *d_frames, int F, int H, int W, int siting, const double *d_map,
                          unsigned char *d_out, unsigned char *d_inside, void *stream);
int oflk_warp_perspective_nv12(const unsigned char *d_frames, int F, int H, int W, int siting, const double *d_map,
                               unsigned char *d_out, unsigned char *d_inside, void *stream);
/* host arrays, synchronous, in chunks of at most 64 frames; the result does not depend on the cut */
int oflk_warp_affine_nv12_host(const unsigned char *frames, int F, int H, int W, int siting, const double *map,
                               unsigned char *out, unsigned char *inside);
int oflk_warp_perspective_nv12_host(const unsigned char *frames, int F, int H, int W, int siting, const double *map,
                                    unsigned char *out, unsigned char *inside);
/* oflk_stabilize_sequence_u8's arguments with siting after W and NV12 frames in and out: frames, out [T][H W 3 / 2] */
int oflk_stabilize_sequence_nv12(const unsigned char *frames, int T, int H, int W, int siting, int levels, int window_size,
                                 int iters, float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                 int max_corners, int detect_every, int model, int hypotheses, float threshold, unsigned seed,
                                 const double *weights, int radius, unsigned char *out, float *correction, float *model_out,
                                 int *counts_out, unsigned char *held);
/* oflk_stabilizer_create's arguments with siting in place of u8 */
int oflk_stabilizer_create_nv12(oflk_stabilizer **st, int device, int H, int W, int siting, int levels, int window_size, int iters,
                                float alpha, float beta, float max_residual, float quality_level, float min_distance,
                                int max_corners, int detect_every, int model, int hypotheses, float threshold, unsigned seed,
                                const double *weights /* host, [radius + 1], copied */, int radius);

/* Rehearsal of the chunk queue above on a box with fewer GPUs than workers (tests): `workers` > 0 makes the *_multi entry
 * points run that many queue workers, worker i on device i % n_gpus (workers of one device take turns on it); 0 restores
 * one worker per device.  Results do not change. */
int oflk_multi_rehearsal(int workers);
/* [begin, end) of `total` units owned by shard `shard` of `n_shards` (contiguous, sizes differ by at
 * most one): the partition used above and by bench.py's ranks */
void oflk_shard_range(int total, int shard, int n_shards, int *begin, int *end);

/* ---- device-resident plan API (pipelines, bench) -------------------------- */
typedef struct oflk_plan oflk_plan;

/* A plan for B pairs of H x W on `device`.  Creation allocates the pyramids and the reduction scratch; the flow
 * ping-pong buffers and blur temporaries of the dense pyramidal passes are allocated by the plan's first such pass, so a
 * plan that only serves oflk_plan_sparse_tracks never holds them (and the first pass of a kind is not capturable).
 * oflk_plan_workspace_bytes reports what is allocated at the moment.  levels = 1 and iters = 0 gives a plan that
 * can only run oflk_plan_single_scale.
 *   window_size : 1 ... 45.  Like the reference (lucas_kanade_core.py:104, :110) a size w uses the (2*(w/2)+1)^2
 *                 window, so 4 and 5 both mean 5x5.  3x3 ... 11x11 (sizes 2 ... 11) run the tiled kernels.  Every other
 *                 size -- 1x1, 13x13 ... 45x45, where np.sum's pairwise order splits into blocks -- runs a generic
 *                 kernel (one thread per output pixel, the sums in NumPy's order for any length; a pyramidal pass
 *                 then runs pair by pair, unfused, with the exit test on the host): the reference's values, slowly.
 *                 Sizes above 45 return OFLK_ERR_UNSUPPORTED; the fp16 mode exists for 2 ... 11 only.
 *   A plan is single-stream: it owns one per-call state block, so at most ONE pass of a plan may be
 *   in flight at a time (enqueue passes of one plan on one stream, or synchronise between streams).
 *   Device pointers: when W % 4 == 0 the kernels move 16 bytes per lane and want every plane
 *   (d_prev, d_curr, d_u, d_v; uint8 frames: 4-byte) 16-byte aligned -- what hipMalloc and
 *   torch allocations give.  Other alignments are accepted and take the element-wise kernels. */
int oflk_plan_create(oflk_plan **plan, int device, int B, int H, int W, int levels,
                     int window_size, int iters);
int oflk_plan_destroy(oflk_plan *plan);
size_t oflk_plan_workspace_bytes(const oflk_plan *plan);

/* Enqueue one pass over the batch on `stream` (a hipStream_t; NULL = default
 * stream).  d_* are device pointers, [B][H][W] float32.  Asynchronous. */
int oflk_plan_single_scale(oflk_plan *plan, const float *d_prev, const float *d_curr,
                           float *d_u, float *d_v, void *stream);
int oflk_plan_pyramidal(oflk_plan *plan, const float *d_prev, const float *d_curr, float *d_u,
                        float *d_v, void *stream);
/* device-resident form of oflk_single_scale_fp16 (any plan; levels / iters are not used) */
int oflk_plan_single_scale_fp16(oflk_plan *plan, const float *d_prev, const float *d_curr, float *d_u, float *d_v,
                                float pixel_max, void *stream);
/* the same passes on device-resident uint8 frames [B][H][W] (see "uint8 frames" above) */
int oflk_plan_single_scale_u8(oflk_plan *plan, const unsigned char *d_prev, const unsigned char *d_curr,
                              float *d_u, float *d_v, void *stream);
int oflk_plan_pyramidal_u8(oflk_plan *plan, const unsigned char *d_prev, const unsigned char *d_curr,
                           float *d_u, float *d_v, void *stream);
/* The pyramidal pass over a frame sequence: a plan created with B pairs, d_frames = [B+1][H][W], d_u, d_v = [B][H][W]; flow b
 * is frames b -> b+1.  It is the pair pass with d_prev = d_frames and d_curr = d_frames + H*W (uint8: H*W bytes) -- same
 * values, log, iteration counts, uncertain flags and level flows as oflk_plan_pyramidal on copies of those two arrays --
 * except that the pyramid is built for the B+1 frames once instead of for 2B images.  Any plan serves both forms; the
 * workspace does not grow.  The reads below mean what they mean after a pair pass, and the resolve calls take the aliased
 * pointers: oflk_plan_resolve_uncertain{,_u8}(plan, d_frames, d_frames + H*W, d_u, d_v, ...). */
int oflk_plan_pyramidal_sequence(oflk_plan *plan, const float *d_frames, float *d_u, float *d_v, void *stream);
int oflk_plan_pyramidal_sequence_u8(oflk_plan *plan, const unsigned char *d_frames, float *d_u, float *d_v, void *stream);
/* Both directions of a sequence on one pyramid: the forward pass of oflk_plan_pyramidal_sequence into d_uf, d_vf, then the
 * backward pass (flow b is frames b+1 -> b) into d_ub, d_vb, all [B][H][W].  The B+1 frames' pyramid is built once; the
 * backward pass runs the same level loop with prev and curr exchanged, on a second per-call state block (iteration counts,
 * log, uncertain flags) that the plan allocates on its first bidirectional call.  Values, logs and flags of either
 * direction equal those of oflk_plan_pyramidal_sequence on the frames (forward) or on the reversed frames (backward, pair
 * B-1-b).  Asynchronous, no host synchronisation: after one eager call the pass can be captured into a graph.
 * oflk_plan_read_log / read_uncertain report the forward pass, the _backward forms below the backward one;
 * oflk_plan_read_level_flow reports the backward pass after a bidirectional call.  Flagged pairs are the caller's to
 * resolve (oflk_plan_resolve_uncertain_sequence_fb), before oflk_fb_consistency. */
int oflk_plan_pyramidal_sequence_fb(oflk_plan *plan, const float *d_frames, float *d_uf, float *d_vf, float *d_ub,
                                    float *d_vb, void *stream);
int oflk_plan_pyramidal_sequence_fb_u8(oflk_plan *plan, const unsigned char *d_frames, float *d_uf, float *d_vf,
                                       float *d_ub, float *d_vb, void *stream);
/* oflk_plan_read_log / oflk_plan_read_uncertain of the backward pass of the last bidirectional call (synchronise) */
int oflk_plan_read_log_backward(oflk_plan *plan, float *residual_log, int *iters_run, void *stream);
int oflk_plan_read_uncertain_backward(oflk_plan *plan, int *uncertain, void *stream);
/* oflk_plan_resolve_uncertain for both directions of a bidirectional call: forward pairs from (d_frames, d_frames + H*W)
 * into d_uf, d_vf, backward pairs from (d_frames + H*W, d_frames) into d_ub, d_vb, each into its own state block.
 * *resolved (may be NULL) counts the pairs redone in both directions.  Level flows (read_level_flow) stay the backward
 * pass's.  Synchronises. */
int oflk_plan_resolve_uncertain_sequence_fb(oflk_plan *plan, const float *d_frames, float *d_uf, float *d_vf, float *d_ub,
                                            float *d_vb, void *stream, int *resolved);
int oflk_plan_resolve_uncertain_sequence_fb_u8(oflk_plan *plan, const unsigned char *d_frames, float *d_uf, float *d_vf,
                                               float *d_ub, float *d_vb, void *stream, int *resolved);
/* Forward-backward consistency of B flow pairs (Sundaram, Brox & Keutzer 2010), one launch, device pointers [B][H][W]:
 * F = (d_uf, d_vf) frames b -> b+1, G = (d_ub, d_vb) frames b+1 -> b.  float32, each operation rounded on its own:
 *   bu = warp_image(ub, uf, vf), bv = warp_image(vb, uf, vf)   (the reference's warp_image, python/lucas_kanade_pyramidal.py:66-97)
 *   e2 = (uf+bu)^2 + (vf+bv)^2;  err_f = sqrt(e2) (correctly rounded)
 *   m2 = (uf^2 + vf^2) + (bu^2 + bv^2)
 *   valid_f = (0 <= x+uf <= W-1) & (0 <= y+vf <= H-1) (float64) & (e2 <= alpha*m2 + beta)   (1 or 0)
 * err_f / valid_f live on frame b's grid; err_b / valid_b are the same with F and G exchanged, on frame b+1's grid.
 * Any output may be NULL, not all four.  alpha, beta finite and >= 0 (Sundaram et al.: 0.01, 0.5).  Asynchronous. */
int oflk_fb_consistency(const float *d_uf, const float *d_vf, const float *d_ub, const float *d_vb, int B, int H, int W,
                        float alpha, float beta, float *d_err_f, float *d_err_b, unsigned char *d_valid_f,
                        unsigned char *d_valid_b, void *stream);
/* Point tracks through B flow pairs, one launch, device pointers: F = (d_uf, d_vf) and G = (d_ub, d_vb) [B][H][W] are pairs
 * t0 .. t0+B-1 of a sequence (F: frames t -> t+1, G: frames t+1 -> t).  Query n is (t_q, x_q, y_q): frame d_qt[n] (d_qt
 * NULL: every query at frame 0) and the float32 point d_qxy[n] = (x, y), x along W.  sample(img, x, y) is the reference's
 * warp_image at one float64 point (SciPy's map_coordinates, order 1, cval 0; float32 result).  float32, each operation
 * rounded on its own, positions carried as float32:
 *   rows t < t_q: (NaN, NaN), visible 0;  x_q, y_q not finite or outside [0, W-1] x [0, H-1]: every row NaN / 0
 *   row t_q: (x, y) = (x_q + 0, y_q + 0), visible 1                     (a query at -0 reads as +0)
 *   for t = t_q .. :  us = sample(uf[t], x, y); vs = sample(vf[t], x, y)
 *                     qx = f64(x) + f64(us); qy = f64(y) + f64(vs)
 *                     inside = 0 <= qx <= W-1 and 0 <= qy <= H-1                          (float64, closed)
 *                     bu = sample(ub[t], qx, qy); bv = sample(vb[t], qx, qy)
 *                     eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
 *                     ok = inside and e2 <= alpha*m2 + beta
 *                     not ok: every later row NaN / 0 (the track ends: occluded, inconsistent or out of the frame)
 *                     ok: (x, y) = (f32(qx), f32(qy)) (nearest even) is row t+1, visible 1
 * d_tracks [B+1][N][2] (8-byte aligned) and d_visible [B+1][N] are the rows of frames t0 .. t0+B.  Row 0 is READ for
 * queries with qt < t0 (the previous call's last row: the whole state of a track) and written for qt >= t0; every other
 * row is written, so calls over consecutive pieces of a sequence give the tracks of one call.  A query point outside the
 * frame is not an error (a never-visible track).  B, N < 1, t0 < 0, NULL flows / queries / outputs, alpha or beta
 * negative or not finite: OFLK_ERR_INVALID.  The point chain is serial: a few thousand points are bound by two dependent
 * gathers per pair.  Asynchronous. */
int oflk_track_points(const float *d_uf, const float *d_vf, const float *d_ub, const float *d_vb, int B, int H, int W,
                      float alpha, float beta, int t0, const int *d_qt, const float *d_qxy, int N, float *d_tracks,
                      unsigned char *d_visible, void *stream);
/* In-between frames of B pairs on their flows (the statement at oflk_interpolate_sequence), device pointers: d_frames
 * [B+1][H][W] float32, or uint8 with u8 != 0, in the sequence layout (pair b is frames b, b+1); the flows [B][H][W]; taus a
 * HOST array of n doubles, copied into the launch arguments; d_out [B][n][H][W] of the frames' type and d_status
 * [B][n][H][W] (may be NULL).  One thread per output pixel, the n times of a pair in adjacent slices of the grid; where B * n
 * exceeds the grid's z limit the slices go in several launches.  Asynchronous, and capturable into a graph.  B < 1, n < 1 or
 * n > OFLK_INTERP_MAX_TAUS, a tau that is not finite or not strictly between 0 and 1, refine outside [1, 8], alpha or beta
 * negative or not finite, NULL d_frames, flows, taus or d_out, d_out overlapping d_frames: OFLK_ERR_INVALID. */
int oflk_interpolate_frames(const void *d_frames, int u8, int B, int H, int W, const float *d_uf, const float *d_vf,
                            const float *d_ub, const float *d_vb, float alpha, float beta, int refine, const double *taus,
                            int n, void *d_out, unsigned char *d_status, void *stream);
/* The same for packed colour frames (the statement at oflk_interpolate_sequence_packed), device pointers: d_frames uint8
 * [B+1][H][W][channels], channels 3 or 4, d_out [B][n][H][W][channels], d_status [B][n][H][W] (may be NULL); flows and taus as
 * oflk_interpolate_frames.  One thread per output pixel: the two solves, the ok bits and the bilinear weights are formed once
 * and every channel is finished on them; a tap is one dword that holds all channels of its pixel, and no load leaves its
 * frame.  Slices and the grid's z limit as oflk_interpolate_frames.  No alignment is asked of any array.  Asynchronous, and
 * capturable into a graph.  Refusals: the list at oflk_interpolate_sequence_packed, with NULL flows. */
int oflk_interpolate_frames_packed(const unsigned char *d_frames, int B, int H, int W, int channels, const float *d_uf,
                                   const float *d_vf, const float *d_ub, const float *d_vb, float alpha, float beta, int refine,
                                   const double *taus, int n, unsigned char *d_out, unsigned char *d_status, void *stream);
/* The same for NV12 frames (the statement at oflk_interpolate_sequence_packed), device pointers: d_frames [B+1][H W 3 / 2],
 * d_out [B][n][H W 3 / 2], d_status [B][n][H][W] (may be NULL), siting OFLK_SITING_*; the flows [B][H][W] are the Y planes'.  One
 * launch for both planes of the slices: luma blocks, then the blocks of the H/2 x W/2 chroma plane, where a lane does one
 * solve per chroma sample, gathers each tap as one 2-byte load holding U and V and finishes both on one set of weights.  No
 * alignment is asked of any array.  Asynchronous, and capturable into a graph.  Refusals: the list at
 * oflk_interpolate_sequence_packed, with NULL flows. */
int oflk_interpolate_frames_nv12(const unsigned char *d_frames, int B, int H, int W, int siting, const float *d_uf,
                                 const float *d_vf, const float *d_ub, const float *d_vb, float alpha, float beta, int refine,
                                 const double *taus, int n, unsigned char *d_out, unsigned char *d_status, void *stream);
/* The median of flow planes (the statement at oflk_flow_median_host), device pointers: d_in and d_out are P contiguous planes
 * [P][H][W] float32.  One launch per 65535 planes: a block is a tile of oflk_flow_median_tile's rows x columns of one plane,
 * stages it and a halo of size / 2 in LDS as sort keys through clamped addresses (no load leaves the plane) and each lane
 * selects the middle of its size^2 keys in registers.  No workspace.  Asynchronous, and capturable into a graph.  Refusals:
 * the list at oflk_flow_median_host. */
int oflk_flow_median(const float *d_in, float *d_out, int P, int H, int W, int size, void *stream);
/* the rows and columns of output pixels of one block of oflk_flow_median (host only, no device call); NULL: OFLK_ERR_INVALID */
int oflk_flow_median_tile(int *tile_h, int *tile_w);
/* Sparse tracks (statement at oflk_sparse_lk) through the plan's B pairs, device pointers: d_frames [B+1][H][W] float32, or
 * uint8 with u8 != 0, are frames t0 .. t0+B.  Builds the B+1 pyramids once, then one track launch (one wave per query,
 * looping over the pairs).  d_qt, d_qxy, N, t0, d_tracks [B+1][N][2], d_visible [B+1][N] and the use of row 0 as
 * oflk_track_points.  Device workspace: the plan's pyramid levels below the frame and nothing of frame size -- a plan that
 * only serves sparse calls holds no flow slot and no blur temporary; only where a level is too small for the fused pyramid
 * kernel the unfused chain's temporaries for B+1 images (and float32 copies of uint8 frames) are allocated, on first need.
 * The plan's window, levels and iterations are checked as oflk_sparse_lk's.  Asynchronous, no host synchronisation; can be
 * captured into a graph after one eager call. */
int oflk_plan_sparse_tracks(oflk_plan *plan, const void *d_frames, int u8, float alpha, float beta, float max_residual,
                            int t0, const int *d_qt, const float *d_qxy, int N, float *d_tracks, unsigned char *d_visible,
                            void *stream);
/* Replenished KLT on the sparse tracker (statement at oflk_pyramidal_sequence_klt_sparse_replenish) through the plan's B
 * pairs, device pointers: d_frames [B+1][H][W] (uint8 with u8 != 0) are frames t0 .. t0+B of the sequence.  t0 == 0: the
 * call makes every slot dead itself.  t0 > 0: d_qt [K], d_qxy [K][2] and row 0 of d_tracks [B+1][K][2] / d_visible [B+1][K]
 * are the previous call's (row 0 is its last row).  It detects on the rows r < B whose frame t0 + r is a multiple of
 * detect_every, never on its last row; it writes d_born [B+1][K] and d_detected [B+1] completely and d_residual (may be
 * NULL) rows 1 .. B, row 0 only when t0 == 0.  The B+1 pyramids are built once; then one track launch per segment of pairs
 * between detection frames, on the buffers offset to the segment's first frame, the detection's seven launches ahead of
 * it.  d_workspace: oflk_replenish_features_workspace bytes, 256-byte aligned; d_qxy and d_tracks 8-byte aligned.  Checks as
 * oflk_plan_sparse_tracks and oflk_replenish_features, detect_every < 1 and t0 < 0: OFLK_ERR_INVALID, before any device
 * call.  Asynchronous, no synchronisation, no host round trip; a single chain on the one stream, which can be captured into
 * a graph after one eager call. */
int oflk_plan_sparse_klt_replenish(oflk_plan *plan, const void *d_frames, int u8, float alpha, float beta, float max_residual,
                                   float quality_level, float min_distance, int max_corners, int detect_every, int t0,
                                   void *d_workspace, size_t workspace_bytes, int *d_qt, float *d_qxy, float *d_tracks,
                                   unsigned char *d_visible, unsigned char *d_born, int *d_detected,
                                   float *d_residual /* may be NULL */, void *stream);
/* Shi-Tomasi scores (statement above) of F frames, device pointers: d_frames [F][H][W] float32, or uint8 with u8 != 0;
 * d_score [F][H][W].  Asynchronous; one launch. */
int oflk_corner_score(const void *d_frames, int u8, int F, int H, int W, int window_size, float *d_score, void *stream);
/* Bytes of the caller's workspace for oflk_good_features of this shape (the worst case: H*W candidates per frame, 8 bytes
 * each, the score maps and, for min_distance > 1, the occupancy grid). */
int oflk_good_features_workspace(int F, int H, int W, int window_size, float min_distance, int max_corners, size_t *bytes);
/* Features of F frames (statement above), device pointers: d_count [F], d_xy [F][K][2] (8-byte aligned), d_score [F][K];
 * d_workspace 256-byte aligned, of at least oflk_good_features_workspace bytes (less: OFLK_ERR_INVALID).  Four kernel
 * launches (the per-frame counters zeroed, score, candidates, selection: one workgroup per frame, no host round trip), so
 * the call can be captured into a graph.  Asynchronous. */
int oflk_good_features(const void *d_frames, int u8, int F, int H, int W, int window_size, float quality_level,
                       float min_distance, int max_corners, void *d_workspace, size_t workspace_bytes, int *d_count,
                       float *d_xy, float *d_score, void *stream);
/* Bytes of the caller's workspace for oflk_replenish_features: oflk_good_features' for one frame, the seed grid (one int
 * per cell of side ceil(min_distance), at most H*W), 12 bytes per slot and the free slots' count. */
int oflk_replenish_features_workspace(int H, int W, int window_size, float min_distance, int max_corners, size_t *bytes);
/* One detection of the replenish statement above, device pointers: d_frame [H][W] (uint8 with u8 != 0) of index t, the
 * slots' row d_xy [K][2] and d_visible [K] in; d_qt [K] and d_qxy [K][2] (8-byte aligned) in and out, so that the next
 * oflk_track_points launch with t0 = t starts the new points; d_born [K], d_detected [1] out.  d_workspace 256-byte
 * aligned, of at least oflk_replenish_features_workspace bytes (less: OFLK_ERR_INVALID).  Seven kernel launches (counters,
 * score, seed grid cleared, seeds linked, free list, candidates, selection), no host round trip: the call can be captured
 * into a graph.  Asynchronous. */
int oflk_replenish_features(const void *d_frame, int u8, int H, int W, int window_size, float quality_level,
                            float min_distance, int max_corners, int t, const float *d_xy, const unsigned char *d_visible,
                            void *d_workspace, size_t workspace_bytes, int *d_qt, float *d_qxy, unsigned char *d_born,
                            int *d_detected, void *stream);

/* After oflk_plan_pyramidal: copy the residual log / iteration counts of the last
 * enqueued pass to the host (synchronises `stream`).  Either pointer may be NULL.
 * A logged mean is NaN exactly where the reference's np.mean(np.abs(d)) is NaN, and +inf exactly where it is +inf
 * (finite frames give both: window products or the solve's numerators that overflow); a finite logged mean is the
 * device's fixed-point mean, within oflk_device_mean_error of the exact mean.  One exception: a block whose FINITE |d|
 * sum passes 2^28 px is clamped there, so where |d| is that large the logged mean is below the reference's and at
 * least 2^28 / (H*W) px, and the printed log can differ from the reference's stdout (tests/test_gpu_ranges.py asserts
 * this statement).  Exit decisions and iteration counts are the reference's.
 * Non-finite values: NaN and +-inf pixels and flows give the reference's values in every entry point, flows and stages
 * (oflk_gradients included: the zero taps of the Sobel kernels are multiplied too, so 0 * inf is NaN, as in the
 * reference's convolve2d).
 * Subnormal values: a Sobel product a * (1/8) or a * (1/4) is exact unless it is subnormal, where it rounds; convolve2d
 * rounds the product and then adds it, and so do oflk_gradients and the alignment kernels' template gradients (whose
 * float64 sums count subnormal gradients), value for value.  The flow kernels and the sparse tracker fuse the product
 * into the addition; where that could differ every product of two gradients underflows to 0, det is 0 and nothing is
 * solved, as in the reference.
 * Beyond the flow paths, the float32 forms of these calls are held to their statements on frames outside [0, 255]
 * (signed, x 257, x 1e9, x 1e12 with pixels near +-3e38, subnormal on and off the 2^9-ulp grid, underflowing products,
 * NaN / +-inf pixels; tests/test_gpu_ranges_features.py, every cell): oflk_sparse_lk, the sparse tracks and the online
 * tracker; oflk_warp_affine and oflk_warp_perspective; oflk_interpolate_frames; the mosaic's accumulate / resolve with
 * and without exposure; oflk_align_refine, its photometric and robust forms and oflk_align_weights.  A non-finite pixel
 * is a value like any other there: it reaches an output through every sample that reads it, with weight 0 too (0 * inf
 * and 0 * NaN are NaN, as in map_coordinates), and through no other; masks, counts and the status of interpolation
 * depend on positions only.  A sample at a NaN coordinate is cval 0, as one outside the frame (oflk_sparse_lk's residual
 * where the displacement is NaN: finite frames whose window sums overflow give that). */
int oflk_plan_read_log(oflk_plan *plan, float *residual_log, int *iters_run, void *stream);

/* After oflk_plan_pyramidal + read_log: uncertain[b*levels + l] has bit k set when the early-exit test
 * after iteration k of level l (python/lucas_kanade_pyramidal.py:221-223) was decided with a mean
 * within the level's band around the 0.01 threshold, oflk_decision_guard (below): NumPy's error bound
 * (ceil(npix / 8192) + 32) * 2^-24 plus the device's (oflk_device_mean_error at 0.01), at least 5e-5 relative, i.e.
 * 5e-5 up to 1080p, 6.3e-5 at 4K, 2.44e-4 at 8K.  The reference sums np.mean in fp32 (pairwise, in 8192-element
 * pieces); the device adds partial sums formed in fp32 / fp64 and each rounded to a 2^-20 px grid (one per block of
 * the tile kernel, one per wave of the streaming kernel) -- neither is exact, and the band covers both errors, so
 * 0 everywhere means "provably the reference's iteration counts".  Synchronises. */
int oflk_plan_read_uncertain(oflk_plan *plan, int *uncertain, void *stream);

/* Closes that band: every pair of the last pass with a flagged decision is redone -- that pair alone, with
 * the standalone kernels in the reference's own sequence (pyramid, warp, single-scale LK, flow += d,
 * upsample; value-identical to the fused path) and np.mean(np.abs(d)) evaluated in NumPy's own order
 * (fp32 pairwise inside 8192-element pieces, the pieces added serially), the exit test taken on the host.
 * The pair's slices of d_u / d_v, its log, iteration counts and flags are replaced, so afterwards the
 * whole batch is the reference's result with the reference's iteration counts.  Slow (a host round trip
 * per iteration) and rare (never seen outside constructed inputs).  d_prev / d_curr are the frames the
 * pass was given (after a sequence pass: d_frames and d_frames + H*W); *resolved (may be NULL) receives the number of
 * pairs redone.  Synchronises.
 * The host entry points (oflk_pyramidal*, oflk_pyramidal_u8*) do this themselves after every call;
 * oflk_last_resolved() tells how many pairs the calling thread's last such call redid. */
int oflk_plan_resolve_uncertain(oflk_plan *plan, const float *d_prev, const float *d_curr, float *d_u, float *d_v,
                                void *stream, int *resolved);
int oflk_plan_resolve_uncertain_u8(oflk_plan *plan, const unsigned char *d_prev, const unsigned char *d_curr,
                                   float *d_u, float *d_v, void *stream, int *resolved);
int oflk_last_resolved(void);

/* Final flow of a coarser pyramid level (level < levels-1; the finest level's flow is the result) of
 * pair `pair` of the last pass, to host arrays of that level's size -- what the reference hands to
 * visualize_pyramid_level at python/lucas_kanade_pyramidal.py:226.  After oflk_plan_pyramidal_sequence_fb{,_u8}: the
 * backward pass's level flows (pair b: frames b+1 -> b).  Synchronises. */
int oflk_plan_read_level_flow(oflk_plan *plan, int level, int pair, float *u, float *v, void *stream);

/* Arithmetic of the plan's fp64 stages.  OFLK_ARITH_EXACT (the default of plans and of the host entry points): results
 * equal the reference's value for value.  Every stage executes SciPy's operation sequence, each operation rounded on its
 * own, with one exception that keeps the results: the fused pyramid kernel forms each blurred value with fused
 * multiply-adds, proves on the device that it rounds to the float32 SciPy's sequence rounds to, and executes SciPy's
 * sequence where the proof fails.
 * OFLK_ARITH_CONTRACTED (opt-in): the same fused sums without that proof, in the sampling as well: the Gaussian pyramid (python/lucas_kanade_pyramidal.py:46-59) accumulates with fused
 * multiply-adds, 17 instead of 25 fp64 operations per blurred value on a kernel the fp64 pipe binds.  Intermediates
 * differ from SciPy's by a few 1e-16 relative before they are rounded to float32 where SciPy rounds, so a pyramid value
 * differs from the reference's only where the fp64 value lies that close to a float32 rounding boundary (about one in
 * 10^7, by one ulp); coarse-to-fine LK then amplifies such a difference locally.  Measured on the 13 verification
 * patterns (tests/test_gpu_round3.py, profiles/): mean EPE against the reference far below the 1e-4 bar.  Affects
 * oflk_plan_pyramidal / _u8 only.
 * OFLK_ARITH_TOLERANT (opt-in): relaxations whose cost in endpoint error against the reference was measured, and which are
 * applied only inside the ENVELOPE below:
 *   - the contracted pyramid (above);
 *   - on the TWO FINEST levels, 5x5 window, the fused iteration runs as a streaming kernel (k_lks) whose window sums are
 *     separable -- five rows added vertically, then five columns horizontally, not np.sum's pairwise order of
 *     python/lucas_kanade_core.py:115-119 -- and whose warp (python/lucas_kanade_pyramidal.py:88-96) forms the bilinear
 *     sample as three fused lerps in fp64 instead of SciPy's 15 operations, with the flow upsampling into such a level
 *     fused into its first iteration in the same fused-lerp form; gradients, products, the 2x2 solve (IEEE divisions) and
 *     flow += d are the reference's operations;
 *   - coarser levels: exact.
 * The envelope is the set of (levels, iterations) cells of the 5x5 window where the worst mean EPE of the 13 verification
 * patterns (320x240) against the reference is at most a third of the north star's bar of 1e-4 px and every iteration count
 * is the reference's: {(1,1), (1,2), (3,2), (3,3)}.  The bar is promised for frames whose pixels lie in [-255, 255] (the
 * 8-bit range and its normalised, signed, subnormal and underflowing forms: tests/test_gpu_ranges.py, every cell); on
 * larger values it is not (16-bit frames with a 25 000 temporal step: mean EPE 0.13 .. 0.3 px at (1,1) and (1,2), 30 ..
 * 100 px at (3,2) and (3,3)).  Measured worst mean EPE per cell (tests/test_tolerant_model.py):
 *       L \ K    1        2        3        4        5
 *         1      0        2.3e-5   4.6e-4   5.6e-4   1.7e-3
 *         2      3.5e-5   7.7e-5   9.6e-5   5.7e-4   2.6e-4
 *         3      5.0e-5   1.1e-5   1.7e-5   5.8e-5   1.2e-4
 *         4      1.3e-4   0.131    1.6e-4   1.1e-4   7.1e-4
 * The error outside the envelope is amplification at ill-conditioned pixels (at L=4, K=2 a few pixels of rotate_large move
 * by hundreds of px), not a drift the arithmetic could be tuned out of.  Every other cell -- other (levels, iterations),
 * other windows -- runs exactly, pyramid included: a tolerant plan there returns OFLK_ARITH_EXACT's values
 * (oflk_tolerant_relaxes tells which cells relax).  Inside the envelope, against dense flows of the reference itself
 * (tests/golden/dense_reference_flows.npz) at L=3, K=3: worst of the 13 patterns 1.7e-5 px (translate_extreme), the 1080p
 * bench pair 5.6e-7 px.  The arithmetic is stated on the CPU by oracle/oflk_tolerant_model.c (test infrastructure) and the
 * kernels are held to that statement bit for bit in every cell (tests/test_gpu_tolerant_envelope.py), so the tolerance is a
 * property of one written-down arithmetic, not of a GPU run.
 * In both opt-in modes the exit-decision flags keep their meaning: a decision is flagged when the level's mean |d| lies within
 * the band around 0.01 of the kernel that summed it (oflk_decision_guard: NumPy's summation error at the level's pixel count
 * plus the device's, at least 5e-5 relative).  The band needs no widening for the opt-in arithmetic itself: on constructed near-threshold pairs in every envelope
 * cell, a logged mean within [0.5, 2] x 0.01 differs from the reference's by at most 8.1e-7 relative (the tests hold it to a
 * quarter of the band).  oflk_plan_resolve_uncertain redoes a flagged pair in EXACT arithmetic from the caller's frames (its
 * own exact pyramid): a redone pair is the reference's result, which is inside any tolerance.  Windows without a fused
 * iteration kernel (1x1, 13x13 ...) always run exactly. */
#define OFLK_ARITH_EXACT 0
#define OFLK_ARITH_CONTRACTED 1
#define OFLK_ARITH_TOLERANT 2
int oflk_plan_set_arithmetic(oflk_plan *plan, int mode);
/* The same choice for the host-pointer entry points (oflk_pyramidal*, oflk_pyramidal_u8*, the *_multi forms): process-wide,
 * default OFLK_ARITH_EXACT.  The Python shims call it once when the environment variable OFLK_ARITH is set to "contracted" or
 * "tolerant"; without it the drop-in functions return the reference's values.  Pairs whose exit decision is flagged are
 * redone exactly in every mode (oflk_last_resolved). */
int oflk_set_host_arithmetic(int mode);
/* 1 when OFLK_ARITH_TOLERANT relaxes anything in a pass of `levels` levels, `window_size` window and `iterations`
 * iterations (its envelope, above), 0 when the mode runs that configuration exactly.  Host-only; never fails. */
int oflk_tolerant_relaxes(int levels, int window_size, int iterations);
/* The exit band's two terms for one pair's level of level_h x level_w pixels, by how the level sums |d|:
 * OFLK_SUM_TILES (the tile kernels: every level of exact / contracted plans, coarse levels of tolerant ones),
 * OFLK_SUM_STREAMING (the streaming kernel: the tolerant mode's two finest levels inside its envelope), OFLK_SUM_HOST
 * (windows without a fused iteration kernel: NumPy's own mean, taken on the host).  oflk_device_mean_error: E_dev, the
 * worst-case relative error of the logged / compared mean against the exact mean `mean` of the same d (it grows as the
 * mean shrinks: the grid roundings are absolute); for OFLK_SUM_HOST, NumPy's bound.  oflk_decision_guard: the relative
 * half-width of the band in which decisions are flagged (0 for OFLK_SUM_HOST, which decides as NumPy does).  The
 * derivation is at decision_guard in csrc/oflk_kernels.hpp.  Host-only; never fail. */
#define OFLK_SUM_TILES 0
#define OFLK_SUM_STREAMING 1
#define OFLK_SUM_HOST 2
double oflk_device_mean_error(int path, int level_h, int level_w, double mean);
double oflk_decision_guard(int path, int level_h, int level_w);

/* Which kernel runs a single-scale pass (oflk_plan_single_scale / _u8; results are the reference's either way).
 * The 5x5 and 7x7 windows have a streaming kernel (no LDS; window sums vertical-then-horizontal), which equals np.sum's order exactly
 * wherever the frames are integers in [0, 255] -- what python/optical_flow_verifier.py:61-65 makes of the 8-bit files -- and a
 * window's sum Ix^2, sum Iy^2 stay below 2^16 (every partial sum is then exact in any order; proof in csrc/oflk_stream.hpp);
 * tiles where either is in doubt are flagged on the device and redone by the tile kernel in NumPy's order within the same call.
 * OFLK_KERNELS_AUTO (default): the streaming kernel for launches large enough to fill the chip with it (it walks rows serially
 * inside a wave: a single small pair is faster on the tile kernel), the tile kernel otherwise.  OFLK_KERNELS_TILE: the tile
 * kernel for everything (NumPy's order throughout).  OFLK_KERNELS_STREAM: the streaming kernel whenever the window is 5x5 or 7x7. */
#define OFLK_KERNELS_AUTO 0
#define OFLK_KERNELS_TILE 1
#define OFLK_KERNELS_STREAM 2
int oflk_plan_set_kernels(oflk_plan *plan, int choice);

/* Per-kernel timing with HIP events on the launch stream.  While enabled, every
 * kernel launch of the plan is bracketed by an event pair; oflk_plan_kernel_times
 * synchronises, accumulates and reports per kernel class.
 *   names[i]  : static strings (kernel class names), up to max entries
 *   total_ms  : summed duration per class since profiling was enabled/reset
 *   launches  : launch count per class
 * Returns the number of classes written (>= 0) or an error code.
 * enabled: 0 off, 1 every kernel, 2 only the dominant kernel (fused LK iteration at the
 * finest level; three event pairs per pyramidal call instead of 15). */
int oflk_plan_set_profiling(oflk_plan *plan, int enabled);
int oflk_plan_kernel_times(oflk_plan *plan, const char **names, double *total_ms, long *launches,
                           int max_entries);

/* ---- masked flow metrics on the device -------------------------------------- */
/* compute_all_metrics(u_pred, v_pred, u_true, v_true, mask) of python/flow_metrics.py:166-201
 * (mean_absolute_error :14-40, root_mean_square_error :43-70, endpoint_error :73-103,
 * angular_error :106-163) for the rectangular test regions the verifier builds
 * (mask[y0:y1, x0:x1] = True, python/optical_flow_verifier.py:96-138).
 *   u_true, v_true : host arrays [B], the constant ground-truth vector of each pair, taken as float32
 *   out            : host array [B][5] = mae_u, mae_v, rmse, epe, aae (degrees), each a float32 value
 * The statement (tests/metrics_model.py states it in NumPy, tests/test_gpu_metrics_edges.py holds the kernel to it):
 *   rectangle  NumPy slice semantics per bound: i < 0 -> i + n, then clip to [0, n]; bounds beyond the frame are
 *              clipped, a reversed or zero-width slice is empty.  No pixel outside the rectangle is read.
 *   per pixel  the reference's fp32 operations, each rounded on its own: eu = u - ut, ev = v - vt, sq = eu*eu + ev*ev,
 *              sqrt(sq), mag2 = u*u + v*v, c = (u*ut + v*vt + 1) / (sqrt(mag2 + 1) * sqrt(ut*ut + vt*vt + 1)), c clipped
 *              to [-1, 1] as np.clip does: a NaN c stays NaN
 *   sums       of |eu|, |ev|, sq, sqrt(sq) and acos((double)c) * 57.29577951308232 in fp64 over the n pixels
 *   out        (float)(sum / n) for mae_u, mae_v, epe, aae; sqrtf((float)(sum_sq / n)) for rmse.  An empty rectangle
 *              gives NaN (0 / 0).  aae is 0.0 exactly when sqrt(ut^2 + vt^2) < 1e-6 and every pixel of the rectangle
 *              has sqrtf(mag2) < 1e-6f ("nothing moves and nothing was predicted", :141-145): a NaN pixel has not, an
 *              empty rectangle has.
 * Non-finite inputs give the reference's values: a NaN flow value inside the rectangle makes that plane's mae, rmse,
 * epe and aae NaN; an infinite one makes its mae, rmse and epe +inf and aae NaN (inf / inf); a finite value whose
 * square overflows makes rmse and epe +inf and leaves aae finite (that pixel's cosine is 0); values outside the
 * rectangle change nothing.  A finite result is within one float32 ulp of the exact-sum value (the fp64 sums of n <=
 * 3.3e7 non-negative terms are within 3.7e-9 relative) and agrees with the reference's fp32 pairwise means to NumPy's
 * own bound, (ceil(n / 8192) + 32) * 2^-24 relative (aae: plus NumPy's fp32 arccos, 1.5e-5 degrees per term); it is
 * not bit-equal to them.  A pair's numbers do not depend on the batch it is in; any B >= 1 is accepted (beyond 65 535
 * pairs a block of the kernel walks several).  NULL pointers and B, H, W < 1 return OFLK_ERR_INVALID.
 * oflk_plan_metrics reads device-resident flows [B][H][W] of the plan's shape (4-byte alignment is enough) and
 * synchronises `stream`; oflk_flow_metrics takes host arrays. */
int oflk_plan_metrics(oflk_plan *plan, const float *d_u, const float *d_v, const float *u_true,
                      const float *v_true, int y0, int y1, int x0, int x1, double *out, void *stream);
int oflk_flow_metrics(const float *u, const float *v, int B, int H, int W, const float *u_true,
                      const float *v_true, int y0, int y1, int x0, int x1, double *out);

/* ---- RTL-bit-accurate integer mode ------------------ */
/* What the reference's single-scale RTL computes for a frame pair streamed by
 * rtl/common/frame_buffer_simple.sv -- rtl/common/line_buffer_5x5.sv:75-151 (window geometry),
 * rtl/unopt/gradient_compute.sv:89-139 (averaged-frame Sobel >>> 3, It = prev - curr),
 * rtl/unopt/window_accumulator.sv:100-189 (25 products per quantity, 32-bit sums),
 * rtl/unopt/flow_solver.sv:82-149 (low-32-bit products, |det| > 1000, (num <<< 7) / det truncating,
 * clamp to +-1024) -- i.e. the values `flow_u` / `flow_v` carry in S8.7 fixed point when the
 * accumulator has ingested element k of the gradient stream.  It replaces an xsim run of
 * tb/tb_optical_flow_top.sv as the golden model of the RTL; python/rtl_golden_model.py turns the
 * per-element values into the testbench's sample sequence, summary and flow_field.txt.
 *   prev, curr : uint8 [B][H][W], 5 <= H <= 512, 5 <= W <= 1024 (flow_y is 9, flow_x 10 bits wide)
 *   u, v       : int16 [B][oflk_rtl_stream_length(H, W)] = [B][(H-4)(W-4)]
 * The RTL's geometry is kept with its quirks (one-pixel stream offset, the accumulator's rows are
 * not image rows, the window of a row's last position is mostly zero): oracle/rtl_model.py
 * states it.  PARITY UNPINNED: the model is held equal to a cycle-by-cycle execution of the modules
 * (oracle/rtl_cycle_sim.py), but no simulator output of the RTL as committed exists to pin either. */
long oflk_rtl_stream_length(int H, int W);
int oflk_rtl_flow_u8(const unsigned char *prev, const unsigned char *curr, int B, int H, int W, short *u, short *v);
/* device-resident form; enqueues one kernel on `stream` */
int oflk_rtl_flow_u8_device(const unsigned char *d_prev, const unsigned char *d_curr, int B, int H, int W, short *d_u,
                            short *d_v, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OFLK_H */
