"""Drop-in for the reference's ``python/lucas_kanade_core.py``: same module name,
same function names, signatures and defaults, but every function runs
hand-written HIP kernels on an MI355X through liboflk's C ABI.

Put this directory on ``sys.path`` / ``PYTHONPATH`` in place of the reference's
``python/`` directory and ``from lucas_kanade_core import ...`` keeps working
(reference import sites: optical_flow_verifier.py:19, lucas_kanade_reference.py:14,
lucas_kanade_pyramidal.py:15).

Outputs equal the reference's value for value (see DESIGN.md "Exactness").
No CPU fallback exists: without the built library or a GPU the calls raise.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import numpy.typing as npt

import _oflk


def compute_gradients(
    frame_prev: npt.NDArray[np.float32], frame_curr: npt.NDArray[np.float32]
) -> Tuple[npt.NDArray[np.float32], npt.NDArray[np.float32], npt.NDArray[np.float32]]:
    """Sobel/8 spatial gradients of the frame average and It = prev - curr.

    Replaces reference lucas_kanade_core.py:15-45 (oflk_compute_gradients).
    """
    p, c = _oflk.as_f32(frame_prev), _oflk.as_f32(frame_curr)
    H, W = _oflk.same_shape(p, c)
    Ix = np.empty((H, W), np.float32)
    Iy = np.empty((H, W), np.float32)
    It = np.empty((H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_compute_gradients(_oflk.ptr(p), _oflk.ptr(c), H, W, _oflk.ptr(Ix),
                                                   _oflk.ptr(Iy), _oflk.ptr(It)))
    return Ix, Iy, It


def _pair(frame_prev, frame_curr):
    """(prev, curr, u8): two raw 8-bit frames as they are (converted on the device: the values of .astype(np.float32) first),
    anything else as float32"""
    if _oflk.both_u8(frame_prev, frame_curr):
        return np.ascontiguousarray(frame_prev), np.ascontiguousarray(frame_curr), True
    return _oflk.as_f32(frame_prev), _oflk.as_f32(frame_curr), False


def lucas_kanade_single_scale(
    frame_prev: npt.NDArray[np.float32],
    frame_curr: npt.NDArray[np.float32],
    window_size: int = 5,
) -> Tuple[npt.NDArray[np.float32], npt.NDArray[np.float32]]:
    """Dense single-scale Lucas-Kanade flow (u, v); one fused GPU kernel.

    Replaces reference lucas_kanade_core.py:48-70 (oflk_single_scale).
    """
    p, c, u8 = _pair(frame_prev, frame_curr)
    H, W = _oflk.same_shape(p, c)
    u = np.empty((H, W), np.float32)
    v = np.empty((H, W), np.float32)
    src, fn = _oflk.pixels(p, "oflk_single_scale")
    _oflk.check(fn(src, _oflk.pix(c), *((1,) if u8 else ()), H, W, int(window_size), _oflk.ptr(u), _oflk.ptr(v)))
    return u, v


def lucas_kanade_single_scale_sequence(frames, window_size: int = 5):
    """(u, v), each (T-1, H, W) float32: single-scale flow of every consecutive pair of a (T, H, W) float frame sequence
    (uint8 frames are converted to float32 first, which gives the same values).  Each frame is uploaded once."""
    arr, _ = _oflk.as_sequence(frames)
    arr = np.ascontiguousarray(arr, np.float32)
    T, H, W = arr.shape
    u = np.empty((T - 1, H, W), np.float32)
    v = np.empty((T - 1, H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_single_scale_sequence(_oflk.ptr(arr), T, H, W, int(window_size), _oflk.ptr(u), _oflk.ptr(v)))
    return u, v


def lucas_kanade_single_scale_fp16(frame_prev, frame_curr, window_size: int = 5, pixel_max: float = 255.0):
    """Opt-in reduced-precision single-scale flow: fp16 gradients and fp16 window accumulators
    (BASELINE.json config 5; oflk_single_scale_fp16).  No counterpart in the reference, whose
    arithmetic is fp32 (lucas_kanade_core.py:110-133): close to ``lucas_kanade_single_scale``,
    not equal to it (tests/test_gpu_fp16.py reports the endpoint error per pattern)."""
    p, c = _oflk.as_f32(frame_prev), _oflk.as_f32(frame_curr)
    H, W = _oflk.same_shape(p, c)
    u = np.empty((H, W), np.float32)
    v = np.empty((H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_single_scale_fp16(_oflk.ptr(p), _oflk.ptr(c), 1, H, W, int(window_size),
                                                   float(pixel_max), _oflk.ptr(u), _oflk.ptr(v)))
    return u, v


def lucas_kanade_from_gradients(
    Ix: npt.NDArray[np.float32],
    Iy: npt.NDArray[np.float32],
    It: npt.NDArray[np.float32],
    window_size: int = 5,
) -> Tuple[npt.NDArray[np.float32], npt.NDArray[np.float32]]:
    """Window sums of the gradient products and the per-pixel 2x2 solve.

    Replaces reference lucas_kanade_core.py:73-135 (oflk_from_gradients).
    """
    gx, gy, gt = _oflk.as_f32(Ix), _oflk.as_f32(Iy), _oflk.as_f32(It)
    H, W = _oflk.same_shape(gx, gy, gt)
    u = np.empty((H, W), np.float32)
    v = np.empty((H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_from_gradients(_oflk.ptr(gx), _oflk.ptr(gy), _oflk.ptr(gt), H, W,
                                                int(window_size), _oflk.ptr(u), _oflk.ptr(v)))
    return u, v


def corner_min_eigenvalue(frame_or_frames, window_size: int = 5) -> npt.NDArray[np.float32]:
    """Shi-Tomasi score: the smaller eigenvalue of the structure tensor the LK solve inverts, on the GPU.

    frame_or_frames: one (H, W) frame or an (F, H, W) batch (all uint8: the uint8 path).  The tensor is the window sum
    (window_size odd in [3, 11]) of Ix*Ix, Ix*Iy, Iy*Iy of compute_gradients(f, f); the score is 0 outside the pixels the
    solve covers.  Returns float32 of the input's shape.  The arithmetic is stated in include/oflk.h.
    """
    _, _, _, win = _oflk.check_feature_params(1, 0.0, 0.0, window_size)
    arr, _ = _oflk.as_frames(frame_or_frames)
    F, H, W = arr.shape
    S = np.empty((F, H, W), np.float32)
    src, fn = _oflk.pixels(arr, "oflk_corner_score_host")
    _oflk.check(fn(src, F, H, W, win, _oflk.ptr(S)))
    return S[0] if np.ndim(frame_or_frames) == 2 else S


def good_features_to_track_batch(frames, max_corners: int, quality_level: float = 0.01, min_distance: float = 10.0,
                                 window_size: int = 5):
    """Shi-Tomasi features of every frame of a batch, on the GPU (goodFeaturesToTrack semantics, deterministic).

    Candidates are local maxima (>= their 8 neighbours) of corner_min_eigenvalue above quality_level times the frame's
    maximum; they are taken by score, ties by raster index, and one within min_distance of an accepted point is skipped,
    up to max_corners.  Returns (xy (F, K, 2) float32 (x, y) in acceptance order, (NaN, NaN) beyond the count;
    score (F, K) float32, 0 beyond the count; count (F,) int32).
    """
    K, q, md, win = _oflk.check_feature_params(max_corners, quality_level, min_distance, window_size)
    arr, _ = _oflk.as_frames(frames)
    F, H, W = arr.shape
    count = np.empty(F, np.int32)
    xy = np.empty((F, K, 2), np.float32)
    score = np.empty((F, K), np.float32)
    src, fn = _oflk.pixels(arr, "oflk_good_features_host")
    _oflk.check(fn(src, F, H, W, win, q, md, K, count.ctypes.data_as(_oflk._i32p), _oflk.ptr(xy), _oflk.ptr(score)))
    return xy, score, count


def good_features_to_track(frame, max_corners: int, quality_level: float = 0.01, min_distance: float = 10.0,
                           window_size: int = 5):
    """good_features_to_track_batch of one (H, W) frame, trimmed to its count: (xy (n, 2) float32 (x, y), score (n,))."""
    if np.ndim(frame) != 2:
        raise ValueError(f"expected one (H, W) frame, got shape {np.shape(frame)}")
    xy, score, count = good_features_to_track_batch(np.asarray(frame)[None], max_corners, quality_level, min_distance,
                                                    window_size)
    n = int(count[0])
    return xy[0, :n], score[0, :n]


def features_to_queries(xy, count=None, t: int = 0) -> npt.NDArray[np.float32]:
    """Features as the (N, 3) (t, x, y) queries lucas_kanade_pyramidal_sequence_tracks takes.  xy: (n, 2), or a batch
    (F, K, 2) with its count (F,), frame f's features then being queries at frame t + f; rows beyond a count are left
    out."""
    xy = np.asarray(xy, np.float32)
    if xy.ndim == 2:
        xy = xy[None]
        count = [xy.shape[1]] if count is None else count
    if xy.ndim != 3 or xy.shape[2] != 2 or count is None or len(count) != xy.shape[0]:
        raise ValueError(f"expected (n, 2) features, or (F, K, 2) with a count per frame; got shape {xy.shape}")
    rows = [np.column_stack([np.full(int(n), t + f, np.float32), xy[f, :int(n)]]) for f, n in enumerate(count)]
    return np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, 3), np.float32)


def replenish_features(frame, xy, visible, max_corners=None, quality_level: float = 0.01, min_distance: float = 10.0,
                       window_size: int = 5, t: int = 0, qt=None, qxy=None):
    """One detection of the replenished KLT on the GPU: Shi-Tomasi features of `frame` (H, W) away from the live tracks.

    xy (K, 2) float32 (x, y) and visible (K,) are the slots' row on this frame: a slot that is not visible is free.  The
    candidates of good_features_to_track are taken in its order, skipping one within min_distance of the rounded position
    of a visible slot or of a point already taken, until every free slot is filled; the i-th point goes to the i-th free
    slot.  Returns (qt (K,) int32, qxy (K, 2) float32, born (K,) bool, detected): qt / qxy are the given arrays (default
    -1 / NaN) with the born slots set to t and their points, every other slot unchanged; they are what
    oflk_track_points takes to start the new tracks at frame t.  The statement is in include/oflk.h.
    """
    if np.ndim(frame) != 2:
        raise ValueError(f"expected one (H, W) frame, got shape {np.shape(frame)}")
    xy = np.ascontiguousarray(xy, np.float32)
    vis = np.ascontiguousarray(np.asarray(visible) != 0, np.uint8)
    if xy.ndim != 2 or xy.shape[1] != 2 or vis.shape != (xy.shape[0],):
        raise ValueError(f"expected xy (K, 2) and visible (K,), got {xy.shape} and {vis.shape}")
    K = xy.shape[0]
    if max_corners is not None and int(max_corners) != K:
        raise ValueError(f"max_corners {max_corners!r} is not the number of slots {K}")
    K, q, md, win = _oflk.check_feature_params(K, quality_level, min_distance, window_size)
    _oflk.check_int("t", t, 0)
    arr, _ = _oflk.as_frames(frame)
    _, H, W = arr.shape
    qt = np.full(K, -1, np.int32) if qt is None else np.array(qt, np.int32, copy=True, order="C")
    qxy = np.full((K, 2), np.nan, np.float32) if qxy is None else np.array(qxy, np.float32, copy=True, order="C")
    if qt.shape != (K,) or qxy.shape != (K, 2):
        raise ValueError(f"expected qt ({K},) and qxy ({K}, 2), got {qt.shape} and {qxy.shape}")
    born = np.empty(K, np.uint8)
    detected = np.zeros(1, np.int32)
    src, fn = _oflk.pixels(arr, "oflk_replenish_features_host")
    _oflk.check(fn(src, H, W, win, q, md, K, int(t), _oflk.ptr(xy), vis.ctypes.data, qt.ctypes.data_as(_oflk._i32p),
                   _oflk.ptr(qxy), born.ctypes.data, detected.ctypes.data_as(_oflk._i32p)))
    return qt, qxy, born.astype(bool), int(detected[0])


def split_tracks(visible, born):
    """The tracks of a replenished call's slots: [(slot, t_first, t_last)] sorted by slot, then t_first.  visible, born:
    (T, K); a track begins where born is set and lasts while its slot stays visible and no new track is born in it.  Host
    only.  ValueError if the masks do not go together (born without visible, or visible rising without born)."""
    vis, born = np.asarray(visible) != 0, np.asarray(born) != 0
    if vis.ndim != 2 or vis.shape != born.shape:
        raise ValueError(f"expected visible and born of one (T, K) shape, got {vis.shape} and {born.shape}")
    before = np.vstack([np.zeros((1, vis.shape[1]), bool), vis[:-1]])
    if (born & ~vis).any() or (vis & ~before & ~born).any():
        raise ValueError("born must imply visible, and visible may only rise where born is set")
    T = vis.shape[0]
    out = []
    for n in np.flatnonzero(born.any(0)).tolist():
        starts = np.flatnonzero(born[:, n]).tolist()
        for i, t0 in enumerate(starts):
            stop = starts[i + 1] if i + 1 < len(starts) else T
            gone = np.flatnonzero(~vis[t0:stop, n])
            out.append((n, t0, t0 + int(gone[0]) - 1 if len(gone) else stop - 1))
    return out


class Motion(NamedTuple):
    """A global 2-D motion model fitted to point correspondences (estimate_motion)."""
    model: np.ndarray      # (2, 3) float32 [a00 a01 tx; a10 a11 ty]: dst = A src + t; NaN when status is 0.  Batched: (S, 2, 3)
    inlier: np.ndarray     # (N,) bool: the correspondences within the threshold of the returned model.  Batched: (S, N)
    n_inliers: int         # the mask's sum.  Batched: (S,) int32
    n_valid: int           # correspondences that entered the fit
    status: int            # 1: a model was found; 0: fewer valid correspondences than the sample, or every sample degenerate


def _motion(out, inl, cnt, batched: bool) -> Motion:
    m = Motion(out.reshape(-1, 2, 3), inl.astype(bool), cnt[:, 0].copy(), cnt[:, 1].copy(), cnt[:, 2].copy())
    return m if batched else Motion(m.model[0], m.inlier[0], int(m.n_inliers[0]), int(m.n_valid[0]), int(m.status[0]))


def estimate_motion(src, dst, valid=None, model: str = "similarity", hypotheses: int = 256, threshold: float = 1.0, seed: int = 0,
                    step0: int = 0) -> Motion:
    """A robust global motion model between point sets, on the GPU: a deterministic RANSAC and a least-squares refit.

    src, dst: (N, 2) float32 (x, y), or a batch of steps (S, N, 2) fitted independently; valid: (N,) / (S, N) or None.  A
    correspondence enters the fit when its mask is set and its coordinates are finite.  model: "translation",
    "similarity" (rotation, uniform scale, translation) or "affine".  `hypotheses` minimal samples are drawn from a
    counter-based hash of (seed, step0 + s, hypothesis), scored by the number of correspondences within `threshold` pixels,
    and the best one (ties to the lowest) is refitted over its inliers.  The same inputs give the same bytes.  The statement
    is in include/oflk.h; this call fits six coefficients (estimate_homography fits nine) and iterative re-estimation is not
    offered.
    """
    fit = _oflk.check_motion_params(model, hypotheses, threshold, seed)
    a, b, v, batched = _correspondences(src, dst, valid, step0)
    return _motion(*_oflk.estimate_motion_host(a, b, v, *fit, int(step0)), batched)


def _correspondences(src, dst, valid, step0):
    """the arrays of estimate_motion / estimate_homography as the host forms take them: (src, dst (S, N, 2) float32, valid
    (S, N) uint8 or None, batched)"""
    a, b = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    if a.ndim not in (2, 3) or a.shape[-1] != 2 or a.shape != b.shape or a.size == 0:
        raise ValueError(f"expected src and dst of one shape (N, 2) or (S, N, 2), got {a.shape} and {b.shape}")
    batched = a.ndim == 3
    if not batched:
        a, b = a[None], b[None]
    v = None
    if valid is not None:
        v = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
        v = v if batched else v[None]
        if v.shape != a.shape[:2]:
            raise ValueError(f"valid must have shape {a.shape[:2] if batched else a.shape[1:2]}, got {np.shape(valid)}")
    _oflk.check_int("step0", step0, 0, 2 ** 31 - 1, "in [0, 2^31)")
    return a, b, v, batched


def tracks_motion(tracks, visible, born=None, model: str = "similarity", hypotheses: int = 256, threshold: float = 1.0,
                  seed: int = 0, t0: int = 0) -> Motion:
    """The T-1 motions between consecutive rows of any of the track calls: tracks (T, K, 2), visible (T, K), born (T, K) or
    None.  Step t runs from row t to row t+1 with hash index t0 + t; a slot is valid on it when it is visible on both rows
    and not born on row t+1 (a slot that died and was refilled on one row is two different tracks).  Returns a batched
    Motion of T-1 steps."""
    tr, ok = _track_steps(tracks, visible, born)
    return estimate_motion(tr[:-1], tr[1:], ok, model, hypotheses, threshold, seed, t0)


def _track_steps(tracks, visible, born):
    """(tracks (T, K, 2) float32, valid (T-1, K)): a slot is valid on step t when visible on rows t and t+1 and not born on
    row t+1"""
    tr, vis = np.asarray(tracks, np.float32), np.asarray(visible) != 0
    if tr.ndim != 3 or tr.shape[2] != 2 or tr.shape[0] < 2 or vis.shape != tr.shape[:2]:
        raise ValueError(f"expected tracks (T, K, 2) with T >= 2 and visible (T, K), got {tr.shape} and {vis.shape}")
    ok = vis[:-1] & vis[1:]
    if born is not None:
        b = np.asarray(born) != 0
        if b.shape != vis.shape:
            raise ValueError(f"born must have shape {vis.shape}, got {b.shape}")
        ok &= ~b[1:]
    return tr, ok


class Homography(NamedTuple):
    """A homography fitted to point correspondences (estimate_homography)."""
    model: np.ndarray      # (3, 3) float32, model[2, 2] == 1: dst ~ model @ (x, y, 1); NaN when status is 0.  Batched: (S, 3, 3)
    inlier: np.ndarray     # (N,) bool: the correspondences within the threshold of the returned model.  Batched: (S, N)
    n_inliers: int         # the mask's sum.  Batched: (S,) int32
    n_valid: int           # correspondences that entered the fit
    status: int            # 1: a model was found; 0: fewer than four valid correspondences, or every sample degenerate


def estimate_homography(src, dst, valid=None, hypotheses: int = 256, threshold: float = 1.0, seed: int = 0,
                        step0: int = 0) -> Homography:
    """A robust homography between point sets, on the GPU: a deterministic four-point RANSAC and a normalised linear refit.

    src, dst, valid, hypotheses, threshold, seed and step0 are estimate_motion's.  A hypothesis is the closed-form
    homography of four correspondences; a correspondence is an inlier of it when it lies in front of the camera
    (h20 x + h21 y + 1 > 0) and reprojects within `threshold` pixels; the best hypothesis (ties to the lowest) is refitted
    over its inliers by the normalised direct linear transform.  The same inputs give the same bytes.  The statement is in
    include/oflk.h.
    """
    ransac = _oflk.check_ransac_params(hypotheses, threshold, seed)
    a, b, v, batched = _correspondences(src, dst, valid, step0)
    out, inl, cnt = _oflk.estimate_homography_host(a, b, v, *ransac, int(step0))
    m = Homography(out.reshape(-1, 3, 3), inl.astype(bool), cnt[:, 0].copy(), cnt[:, 1].copy(), cnt[:, 2].copy())
    return m if batched else Homography(m.model[0], m.inlier[0], int(m.n_inliers[0]), int(m.n_valid[0]), int(m.status[0]))


def tracks_homography(tracks, visible, born=None, hypotheses: int = 256, threshold: float = 1.0, seed: int = 0,
                      t0: int = 0) -> Homography:
    """The T-1 homographies between consecutive rows of any of the track calls, with tracks_motion's arguments and validity
    rule.  Returns a batched Homography of T-1 steps, model (T-1, 3, 3), NaN where status is 0.  model[t] maps row t to row
    t+1, so warp_perspective(frames[t+1], model[t]) registers frame t+1 onto frame t."""
    tr, ok = _track_steps(tracks, visible, born)
    return estimate_homography(tr[:-1], tr[1:], ok, hypotheses, threshold, seed, t0)


class Trajectory(NamedTuple):
    """The smoothed camera trajectory of a sequence (stabilize_trajectory)."""
    correction: np.ndarray  # (T, 2, 3) float32: where frame t's content is moved to; the identity on frames 0 and T-1
    map: np.ndarray         # (T, 2, 3) float64: its inverse, the source position of an output pixel: what warp_affine takes
    held: np.ndarray        # (T-1,) bool: the step could not be used (status 0, not finite, singular) and counts as no motion


def stabilize_trajectory(models, status=None, radius: int = 15, sigma=None) -> Trajectory:
    """One steadying correction per frame from the T-1 step models of tracks_motion, on the GPU.

    models: (T-1, 2, 3) or (T-1, 6) float32, step s mapping frame s to frame s+1 (an empty array: T = 1); status: (T-1,) or
    None -- a step with status 0 is held, like one whose model is not finite or singular: the camera is taken to stand still
    across it.  Frame t's correction is the Gaussian-weighted mean (weights exp(-0.5 (i / sigma)^2), sigma = radius / 2 by
    default, formed here with NumPy) of the motions from frame t to frames t-r_t .. t+r_t, with r_t = min(radius, t, T-1-t):
    the window is always symmetric, so the first and last frame are never moved and a uniform camera motion is left alone.
    The same inputs give the same bytes; the statement is in include/oflk.h.
    """
    w = _oflk.check_window(radius, sigma).weights
    m = np.ascontiguousarray(models, np.float32)
    if m.ndim == 3 and m.shape[1:] == (2, 3):
        m = m.reshape(-1, 6)
    if m.ndim != 2 or m.shape[1] != 6:
        if m.size:
            raise ValueError(f"expected models of shape (T-1, 2, 3) or (T-1, 6), got {np.shape(models)}")
        m = m.reshape(0, 6)
    S = m.shape[0]
    counts = None
    if status is not None:
        st = np.asarray(status)
        if st.shape != (S,):
            raise ValueError(f"status must have shape {(S,)}, got {st.shape}")
        counts = np.zeros((S, 3), np.int32)
        counts[:, 2] = st != 0
    corr, mp, held = _oflk.stabilize_trajectory_host(m, counts, S + 1, w)
    return Trajectory(corr.reshape(-1, 2, 3), mp.reshape(-1, 2, 3), held.astype(bool))


def rgb_to_luma(frames, order: str = "rgb"):
    """The luma of interleaved colour frames, on the GPU: Y = (77 R + 150 G + 29 B + 128) >> 8 in integers, so grey input
    returns itself.  frames: (H, W, C) or (F, H, W, C) uint8 with C = 3 or 4 (a fourth channel is ignored); order: "rgb" or
    "bgr", where R, G and B sit among the first three bytes.  Returns (H, W) or (F, H, W) uint8: what the tracking and flow
    calls, which take one plane, are given for colour video."""
    code = _oflk.check_colour_order(order)
    single = isinstance(frames, np.ndarray) and frames.ndim == 3
    arr = _oflk.as_packed(frames[None] if single else frames, "(H, W, C) or (F, H, W, C)")
    out = _oflk.luma_host(arr, code)
    return out[0] if single else out


def _maps(maps, F: int, n: int) -> np.ndarray:
    """F affine (n = 6: (2, 3) or (6,) each) or perspective (n = 9: (3, 3) or (9,)) maps as one contiguous float64 (F, n) array;
    ValueError for any other shape"""
    m = np.ascontiguousarray(maps, np.float64)
    if m.size != n * F or m.ndim not in (1, 2, 3) or m.shape[-1] not in (3, n) or (n == 9 and m.shape[-1] == 3 and (m.ndim < 2 or m.shape[-2] != 3)):
        raise ValueError(f"expected {F} maps of shape {(2, 3) if n == 6 else (3, 3)} or ({n},), got {np.shape(maps)}")
    return m.reshape(F, n)


def _warp(frames, maps, return_inside: bool, n: int):
    """warp_affine (n = 6) / warp_perspective (n = 9): a 4-D array is interleaved colour frames"""
    if _oflk.is_packed(frames):
        arr = _oflk.as_packed(frames)
        out, ins = _oflk.warp_packed_host(arr, _maps(maps, arr.shape[0], n), bool(return_inside))
        return (out, ins.astype(bool)) if return_inside else out
    single = isinstance(frames, np.ndarray) and frames.ndim == 2
    arr, _ = _oflk.as_frames(frames)
    F, H, W = arr.shape
    if H < 2 or W < 2:
        raise ValueError(f"frames must be at least 2 x 2, got {H} x {W}")
    out, ins = _oflk.warp_affine_host(arr, _maps(maps, F, n), bool(return_inside))
    out = out[0] if single else out
    if not return_inside:
        return out
    return out, (ins[0] if single else ins).astype(bool)


def warp_affine(frames, maps, return_inside: bool = False):
    """Resample frames under one 2 x 3 map each, on the GPU: out[f, y, x] is the bilinear sample (zero outside) of frame f at
    (xs, ys) = maps[f] applied to (x, y) in float64.  frames: (H, W) or (F, H, W), float32 or uint8 (uint8 out: rounded half
    to even); maps: (2, 3) / (6,) for one frame, (F, 2, 3) / (F, 6) for a batch, e.g. Trajectory.map.  With return_inside
    also the (F, H, W) bool mask of the pixels whose source position lies inside the frame.

    A 4-D uint8 array (F, H, W, C), C = 3 or 4, is a batch of interleaved colour frames: the source position is formed once
    per pixel and every channel is sampled there, each channel's bytes being those of this call on its plane; the result has
    the same shape and the mask stays (F, H, W).  A 3-D array keeps meaning (F, H, W) grey frames, so one colour frame is
    passed as frame[None]; float32 colour is refused."""
    return _warp(frames, maps, return_inside, 6)


def warp_perspective(frames, maps, return_inside: bool = False):
    """Resample frames under one 3 x 3 map each, on the GPU: out[f, y, x] is the bilinear sample (zero outside) of frame f at
    (xs, ys) = the first two rows of maps[f] applied to (x, y, 1) and divided by the third, in float64.  A pixel is outside
    where the divisor is not positive or the source position leaves the frame.  frames: (H, W) or (F, H, W), float32 or
    uint8 (uint8 out: rounded half to even); maps: (3, 3) / (9,) for one frame, (F, 3, 3) / (F, 9) for a batch, e.g.
    Homography.model: the map takes an output pixel to its source, so warp_perspective(frames[t+1], model[t]) registers
    frame t+1 onto frame t.  With return_inside also the (F, H, W) bool mask of the pixels that were sampled.

    A 4-D uint8 array (F, H, W, C), C = 3 or 4, is a batch of interleaved colour frames, as in warp_affine: the same shape
    comes back, the mask stays (F, H, W), a 3-D array keeps meaning (F, H, W) grey frames and float32 colour is refused."""
    return _warp(frames, maps, return_inside, 9)


class MosaicChain(NamedTuple):
    """The step homographies of a sequence composed from an anchor frame (mosaic_chain)."""
    from_anchor: np.ndarray   # (T, 3, 3) float64: anchor coordinates to frame t's: what mosaic_composite takes
    to_anchor: np.ndarray     # (T, 3, 3) float64: frame t's coordinates to the anchor's; a chain of its own, not an inversion
    box: np.ndarray           # (T, 4) float64 (xmin, ymin, xmax, ymax) of frame t's corners in anchor coordinates; NaN where dropped
    held: np.ndarray          # (T-1,) bool: the step could not be used and counts as no motion
    dropped: np.ndarray       # (T,) bool: the frame cannot be placed (behind the camera, not finite, beyond extent), or lies past one
    origin: tuple             # (x0, y0): the anchor coordinates of canvas pixel (0, 0)
    canvas_shape: tuple       # (Hc, Wc): the canvas that holds every frame that is not dropped


def mosaic_chain(model, status, shape, anchor: int = 0, extent=None) -> MosaicChain:
    """Every frame of a sequence placed in the coordinates of one anchor frame, on the GPU: the T-1 step models of
    tracks_homography composed forwards and backwards from frame `anchor`.

    model: (T-1, 3, 3) or (T-1, 9) float32, step s mapping frame s to frame s+1 (an empty array: T = 1); status: (T-1,) or None
    -- a step with status 0 is held (taken as no motion), like one that is not finite or singular; shape: (H, W) of the frames.
    A frame whose corners land behind the camera, are not finite or lie more than `extent` (default 8 max(H, W)) from the
    anchor's origin is dropped, and so is every frame beyond it; the anchor never is.  The same inputs give the same bytes;
    the statement is in include/oflk.h."""
    if len(shape) != 2 or int(shape[0]) < 2 or int(shape[1]) < 2:
        raise ValueError(f"shape must be (H, W) with H, W >= 2, got {shape!r}")
    H, W = int(shape[0]), int(shape[1])
    m = np.ascontiguousarray(model, np.float32)
    if m.ndim == 3 and m.shape[1:] == (3, 3):
        m = m.reshape(-1, 9)
    if m.ndim != 2 or m.shape[1] != 9:
        if m.size:
            raise ValueError(f"expected models of shape (T-1, 3, 3) or (T-1, 9), got {np.shape(model)}")
        m = m.reshape(0, 9)
    S = m.shape[0]
    _oflk.check_int("anchor", anchor, 0, S)
    extent = 8.0 * max(H, W) if extent is None else float(extent)
    if not (np.isfinite(extent) and extent > 0):
        raise ValueError(f"extent must be finite and > 0, got {extent!r}")
    counts = None
    if status is not None:
        st = np.asarray(status)
        if st.shape != (S,):
            raise ValueError(f"status must have shape {(S,)}, got {st.shape}")
        counts = np.zeros((S, 3), np.int32)
        counts[:, 2] = st != 0
    fr, to, box, held, drop = _oflk.mosaic_chain_host(m, counts, S + 1, int(anchor), H, W, extent)
    x0, y0, Wc, Hc = _oflk.mosaic_canvas(box, drop)
    return MosaicChain(fr.reshape(-1, 3, 3), to.reshape(-1, 3, 3), box, held.astype(bool), drop.astype(bool), (x0, y0), (Hc, Wc))


def exposure_chain(gain, bias, status=None, anchor: int = 0) -> np.ndarray:
    """The step gains and biases of a photometric refinement (PhotometricAlignment.gain, .bias of sequence_refine_alignment)
    composed from frame `anchor`: (T, 2) float64 (eg, eb) with v_anchor = eg[f] v_f + eb[f], what mosaic_composite takes as
    `exposure`.  gain, bias: (T-1,) -- step t says that frame t+1 looks like gain[t] frame t + bias[t]; status: (T-1,) or None.
    A step with status 0, with a value that is not finite or with gain <= 0 is held, that is taken as (1, 0).  Host only; the
    statement is in include/oflk.h."""
    g, b = np.asarray(gain, np.float32).reshape(-1), np.asarray(bias, np.float32).reshape(-1)
    if g.shape != b.shape:
        raise ValueError(f"gain and bias must have one shape, got {np.shape(gain)} and {np.shape(bias)}")
    S = g.size
    _oflk.check_int("anchor", anchor, 0, S)
    st = None
    if status is not None:
        st = np.asarray(status)
        if st.shape != (S,):
            raise ValueError(f"status must have shape {(S,)}, got {st.shape}")
        st = np.ascontiguousarray(st != 0, np.int32)
    return _oflk.exposure_chain_host(np.ascontiguousarray(np.stack([g, b], axis=1)), st, S + 1, int(anchor))


def mosaic_composite(frames, maps, canvas_shape, origin=(0, 0), skip=None, blend: str = "mean", return_count: bool = False,
                     exposure=None):
    """Blend frames onto one canvas, on the GPU.  Canvas pixel (x, y) has the coordinates (origin[0] + x, origin[1] + y); frame
    f covers it where maps[f] (3 x 3, canvas coordinates to frame f's, e.g. MosaicChain.from_anchor) takes it inside the
    frame, and contributes its bilinear sample there.  blend: "mean"; "feather" (each sample weighted by one plus its distance
    from the frame's nearest edge); "first" / "last" (the lowest / highest frame that covers the pixel).  frames: (F, H, W)
    float32 or uint8 (uint8 out: rounded half to even and saturated to [0, 255]); skip: (F,) flags of frames to leave out,
    e.g. MosaicChain.dropped.  Returns the (Hc, Wc) canvas, zero where no frame reaches; with return_count also the (Hc, Wc) int32 number of frames that
    cover each pixel.

    A 4-D uint8 array (F, H, W, C), C = 3 or 4, is a batch of interleaved colour frames: every channel's plane is blended by a
    call of its own under the same maps and the canvases are stacked to (Hc, Wc, C); the count is the one count of them all.

    exposure: None, or (F, 2) float64 (eg, eb), e.g. of exposure_chain: frame f's sample s enters the blend as eg[f] s + eb[f]
    (exposure compensation; colour frames: the same pair for every channel)."""
    if _oflk.is_packed(frames):
        arr = _oflk.as_packed(frames)
        planes = [mosaic_composite(np.ascontiguousarray(arr[..., c]), maps, canvas_shape, origin, skip, blend, True, exposure)
                  for c in range(arr.shape[-1])]
        canvas = np.stack([p[0] for p in planes], axis=-1)
        return (canvas, planes[0][1]) if return_count else canvas
    arr, _ = _oflk.as_frames(frames)
    F, H, W = arr.shape
    if H < 2 or W < 2:
        raise ValueError(f"frames must be at least 2 x 2, got {H} x {W}")
    code = _oflk.check_mosaic_blend(blend)
    Hc, Wc, x0, y0 = _oflk.check_mosaic_canvas(canvas_shape, origin)
    m = _maps(maps, F, 9)
    sk, ex = _oflk.check_mosaic_flags(F, skip, exposure)
    out, cnt = _oflk.mosaic_composite_host(arr, m, sk, x0, y0, Hc, Wc, code, bool(return_count), ex)
    return (out, cnt) if return_count else out


def mosaic_median(frames, maps, canvas_shape, origin=(0, 0), skip=None, return_count: bool = False, exposure=None):
    """The temporal median of frames on one canvas, on the GPU: the blend that drops what moves through.  Canvas pixels, maps,
    skip, exposure and the count are mosaic_composite's; a pixel's value is the median of the bilinear samples of the frames
    that cover it (each taken to exposure[f] first when that is given), the mean of the two middle ones when their number is
    even, and 0 where no frame reaches.  An object that crosses the shot is in a minority of a pixel's samples wherever the
    background is seen more often than not, and leaves no trace there; "mean" and "feather" paint it in.  The result does not
    depend on the order of the frames.  frames: (F, H, W) float32 or uint8 (uint8 out: rounded half to even and saturated to
    [0, 255]).  All F frames are on the device at once, which is the price of a median; the statement is in include/oflk.h.

    A 4-D uint8 array (F, H, W, C), C = 3 or 4, is a batch of interleaved colour frames: every channel's plane goes through
    the grey call under the same maps and the canvases are stacked to (Hc, Wc, C).  This is a per-channel median, not a vector
    median: a pixel's three channels may come from different frames."""
    if _oflk.is_packed(frames):
        arr = _oflk.as_packed(frames)
        planes = [mosaic_median(np.ascontiguousarray(arr[..., c]), maps, canvas_shape, origin, skip, True, exposure)
                  for c in range(arr.shape[-1])]
        canvas = np.stack([p[0] for p in planes], axis=-1)
        return (canvas, planes[0][1]) if return_count else canvas
    arr, _ = _oflk.as_frames(frames)
    F, H, W = arr.shape
    if H < 2 or W < 2:
        raise ValueError(f"frames must be at least 2 x 2, got {H} x {W}")
    Hc, Wc, x0, y0 = _oflk.check_mosaic_canvas(canvas_shape, origin)
    m = _maps(maps, F, 9)
    sk, ex = _oflk.check_mosaic_flags(F, skip, exposure)
    out, cnt = _oflk.mosaic_median_host(arr, m, sk, ex, x0, y0, Hc, Wc, bool(return_count))
    return (out, cnt) if return_count else out


class Alignment(NamedTuple):
    """Step models refined on pixel intensities (refine_alignment, sequence_refine_alignment)."""
    model: np.ndarray    # (S, 3, 3) (homography, model[2, 2] == 1) or (S, 2, 3) (affine) float32; the input model where status != 1
    status: np.ndarray   # (S,) int32: 1 refined; 0 not refined (input status 0, not finite, or frozen before an update); 2 rejected
    stats: np.ndarray    # (S, 4) float64: mean squared residual before and after, counted share of the frame, accepted updates


class PhotometricAlignment(NamedTuple):
    """Step models refined together with a gain and a bias (refine_alignment, sequence_refine_alignment with photometric=True):
    b under the model looks like gain a + bias."""
    model: np.ndarray    # as Alignment.model
    status: np.ndarray   # as Alignment.status
    stats: np.ndarray    # as Alignment.stats, the residuals being b(M x) - (gain a(x) + bias)
    gain: np.ndarray     # (S,) float32; 1 where status != 1
    bias: np.ndarray     # (S,) float32; 0 where status != 1


class RobustAlignment(NamedTuple):
    """Step models refined under Huber weights (refine_alignment, sequence_refine_alignment with robust_delta given)."""
    model: np.ndarray    # as Alignment.model
    status: np.ndarray   # as Alignment.status; 2: the mean Huber loss grew
    stats: np.ndarray    # (S, 8) float64: mean Huber loss before and after, counted share, accepted updates, mean squared
                         # residual before and after, mean weight before and after (1.0: nothing was down-weighted)
    gain: np.ndarray     # (S,) float32; 1 without photometric or where status != 1
    bias: np.ndarray     # (S,) float32; 0 without photometric or where status != 1


def _align_models(model, status, S: int, kind: str):
    nc = 9 if kind == "homography" else 6
    m = np.ascontiguousarray(model, np.float32)
    if m.size != nc * S:
        raise ValueError(f"expected {S} {kind} models of {nc} coefficients, got {np.shape(model)}")
    st = None
    if status is not None:
        st = np.asarray(status)
        if st.shape != (S,):
            raise ValueError(f"status must have shape {(S,)}, got {st.shape}")
        st = np.ascontiguousarray(st != 0, np.int32)
    return m.reshape(S, nc), st


def _alignment(result, out, st, stats, photo, kind: str, single: bool):
    """the `result` record (Alignment; with photo, PhotometricAlignment or RobustAlignment) of a host alignment call's arrays"""
    fields = (out.reshape((-1, 3, 3) if kind == "homography" else (-1, 2, 3)), st, stats)
    if photo is not None:
        fields += (np.ascontiguousarray(photo[:, 0]), np.ascontiguousarray(photo[:, 1]))
    return result(fields[0][0], int(st[0]), *(f[0] for f in fields[2:])) if single else result(*fields)


def _refine(a, b, m, st, kind: str, settings, delta, photometric: bool, single: bool):
    """refine_alignment's (b given) and sequence_refine_alignment's (b None) call, once their arguments are checked"""
    code, L, n, ms = settings
    if delta is not None:
        return _alignment(RobustAlignment, *_oflk.align_robust_host(a, b, m, st, L, n, code, ms, delta, bool(photometric)), kind, single)
    if photometric:
        return _alignment(PhotometricAlignment, *_oflk.align_host(a, b, m, st, L, n, code, ms, True), kind, single)
    return _alignment(Alignment, *_oflk.align_host(a, b, m, st, L, n, code, ms), None, kind, single)


def refine_alignment(a, b, model, status=None, kind: str = "homography", levels: int = 3, iterations: int = 5,
                     min_share: float = 0.25, photometric: bool = False, robust_delta: Optional[float] = None):
    """Refine step models on the pixels themselves, on the GPU: inverse-compositional Lucas-Kanade registration of frame b to
    the template a over the whole frame, coarse to fine, `iterations` Gauss-Newton updates on each of `levels` pyramid levels.

    a, b: (H, W) or (S, H, W), float32 or uint8, of one type; model: the (3, 3) / (S, 3, 3) homographies of
    estimate_homography (kind "homography") or the (2, 3) / (S, 2, 3) models of estimate_motion (kind "affine"), mapping a's
    coordinates to b's; status: (S,) or None -- a step with status 0 comes back as it went in.  A step that cannot be
    refined (fewer than `min_share` of the pixels land inside b, a flat template, a singular system) keeps its input model
    with status 0, and one whose mean squared residual grew keeps it with status 2.  The same inputs give the same bytes; the
    statement is in include/oflk.h.

    photometric=True estimates a gain and a bias with every step (b under the model looks like gain a + bias: an exposure
    change between the frames) and returns a PhotometricAlignment; a step also stops when its gain would leave (0, inf).

    robust_delta (grey levels; None: the plain sum of squares) puts a Huber weight min(1, robust_delta / |residual|) on every
    pixel, renewed on every iteration, so that an object moving on its own does not pull the fit, and returns a
    RobustAlignment, with or without photometric; status 2 then means that the mean Huber loss grew.  4.0 is a good start:
    the sparse tracker's max_residual default, in the same unit and with the same meaning.  stats[:, 7], the mean weight
    under the refined model, is how to tune it: near 1.0 nothing is down-weighted, far below it the threshold cuts into the
    static scene.  alignment_weights gives the per-pixel map.
    """
    settings = _oflk.check_align_params(kind, levels, iterations, min_share)
    delta = None if robust_delta is None else _oflk.check_robust_delta(robust_delta)
    single = isinstance(a, np.ndarray) and a.ndim == 2
    fa, ua = _oflk.as_frames(a)
    fb, ub = _oflk.as_frames(b)
    if fa.shape != fb.shape or ua != ub:
        raise ValueError(f"a and b must have one shape and type, got {fa.shape} {fa.dtype} and {fb.shape} {fb.dtype}")
    m, st = _align_models(model, status, fa.shape[0], kind)
    return _refine(fa, fb, m, st, kind, settings, delta, photometric, single)


def sequence_refine_alignment(frames, model, status=None, kind: str = "homography", levels: int = 3, iterations: int = 5,
                              min_share: float = 0.25, photometric: bool = False, robust_delta: Optional[float] = None):
    """refine_alignment on the T-1 steps t -> t+1 of frames (T, H, W): model[t] (e.g. of tracks_homography or tracks_motion)
    maps frame t's coordinates to frame t+1's.  Every frame's pyramid is built once.  Returns a batched Alignment, or with
    photometric=True a batched PhotometricAlignment, or with robust_delta given (refine_alignment) a batched RobustAlignment."""
    settings = _oflk.check_align_params(kind, levels, iterations, min_share)
    delta = None if robust_delta is None else _oflk.check_robust_delta(robust_delta)
    arr, _ = _oflk.as_frames(frames)
    if arr.shape[0] < 2:
        raise ValueError(f"a sequence needs at least two frames, got {arr.shape[0]}")
    m, st = _align_models(model, status, arr.shape[0] - 1, kind)
    return _refine(arr, None, m, st, kind, settings, delta, photometric, False)


def alignment_weights(a, b, model, kind: str = "homography", robust_delta: float = 4.0, gain=None, bias=None):
    """The Huber weights of refine_alignment(..., robust_delta=...) under `model`, per pixel and at full resolution, on the
    GPU: (S, H, W) float32, min(1, robust_delta / |b(model x) - a(x)|) where the model lands inside b and 0 elsewhere.  Low
    values mark what moved on its own.

    a, b: (H, W) or (S, H, W), float32 or uint8, of one type; model as refine_alignment's (typically its refined output);
    gain, bias: (S,) or scalars, both or neither -- the residual is then b(model x) - (gain a(x) + bias), as with
    photometric=True.  The statement is in include/oflk.h (oflk_align_weights)."""
    if not isinstance(kind, str) or kind not in _oflk.ALIGN_KINDS:
        raise ValueError(f"kind must be one of {sorted(_oflk.ALIGN_KINDS)}, got {kind!r}")
    delta = _oflk.check_robust_delta(robust_delta)
    fa, ua = _oflk.as_frames(a)
    fb, ub = _oflk.as_frames(b)
    if fa.shape != fb.shape or ua != ub:
        raise ValueError(f"a and b must have one shape and type, got {fa.shape} {fa.dtype} and {fb.shape} {fb.dtype}")
    S = fa.shape[0]
    m, _ = _align_models(model, None, S, kind)
    if (gain is None) != (bias is None):
        raise ValueError("gain and bias go together")
    photo = None
    if gain is not None:
        photo = np.empty((S, 2), np.float32)
        try:
            photo[:, 0], photo[:, 1] = np.asarray(gain, np.float32), np.asarray(bias, np.float32)
        except ValueError:
            raise ValueError(f"gain and bias must be scalars or have shape {(S,)}, got {np.shape(gain)} and {np.shape(bias)}") from None
    return _oflk.align_weights_host(fa, fb, m, _oflk.ALIGN_KINDS[kind], delta, photo)
