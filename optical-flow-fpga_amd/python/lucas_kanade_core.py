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

from typing import Tuple

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


def lucas_kanade_single_scale(
    frame_prev: npt.NDArray[np.float32],
    frame_curr: npt.NDArray[np.float32],
    window_size: int = 5,
) -> Tuple[npt.NDArray[np.float32], npt.NDArray[np.float32]]:
    """Dense single-scale Lucas-Kanade flow (u, v); one fused GPU kernel.

    Replaces reference lucas_kanade_core.py:48-70 (oflk_single_scale).
    """
    if _oflk.both_u8(frame_prev, frame_curr):
        # raw 8-bit frames: converted on the device (same values as .astype(np.float32) first)
        p, c = np.ascontiguousarray(frame_prev), np.ascontiguousarray(frame_curr)
        H, W = _oflk.same_shape(p, c)
        u = np.empty((H, W), np.float32)
        v = np.empty((H, W), np.float32)
        _oflk.check(_oflk.lib().oflk_single_scale_u8(p.ctypes.data, c.ctypes.data, 1, H, W, int(window_size),
                                                     _oflk.ptr(u), _oflk.ptr(v)))
        return u, v
    p, c = _oflk.as_f32(frame_prev), _oflk.as_f32(frame_curr)
    H, W = _oflk.same_shape(p, c)
    u = np.empty((H, W), np.float32)
    v = np.empty((H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_single_scale(_oflk.ptr(p), _oflk.ptr(c), H, W, int(window_size),
                                              _oflk.ptr(u), _oflk.ptr(v)))
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
    arr, u8 = _oflk.as_frames(frame_or_frames)
    F, H, W = arr.shape
    S = np.empty((F, H, W), np.float32)
    if u8:
        _oflk.check(_oflk.lib().oflk_corner_score_host_u8(arr.ctypes.data, F, H, W, win, _oflk.ptr(S)))
    else:
        _oflk.check(_oflk.lib().oflk_corner_score_host(_oflk.ptr(arr), F, H, W, win, _oflk.ptr(S)))
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
    arr, u8 = _oflk.as_frames(frames)
    F, H, W = arr.shape
    count = np.empty(F, np.int32)
    xy = np.empty((F, K, 2), np.float32)
    score = np.empty((F, K), np.float32)
    fn = _oflk.lib().oflk_good_features_host_u8 if u8 else _oflk.lib().oflk_good_features_host
    src = arr.ctypes.data if u8 else _oflk.ptr(arr)
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
