"""Drop-in for the reference's ``python/lucas_kanade_pyramidal.py``: same module
name, function names, signatures and defaults; the arithmetic runs as HIP kernels
on an MI355X through liboflk's C ABI (no CPU fallback).

``lucas_kanade_pyramidal`` is one C call (pyramids, warps, fused LK iterations,
residual reduction and the data-dependent early exit all stay on the device);
the progress lines the reference prints (lucas_kanade_pyramidal.py:172-222) are
reproduced afterwards from the residual log the call returns.

The reference also dumps python/output/pyramid_level_{l}.png from inside the
function (:226), on every call.  Here that side effect is opt-in and best-effort:
with OFLK_DUMP_LEVELS=1 every level's final flow is read back from the device
after the call and handed to ``visualize_pyramid_level`` (skipped silently when
matplotlib is missing); without it nothing leaves the device but the result.

Environment switches (host-side behaviour only, never the arithmetic):
  OFLK_QUIET=1         suppress the progress lines
  OFLK_DUMP_LEVELS=1   write python/output/pyramid_level_{l}.png like the reference
                       (OFLK_DUMP_DIR overrides the directory)
"""
from __future__ import annotations

import argparse
import ctypes
import os
from pathlib import Path
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np
import numpy.typing as npt

import _oflk
from lucas_kanade_core import (_maps, _pair, Alignment, Homography, MosaicChain, Motion, PhotometricAlignment, Trajectory,  # noqa: F401
                               estimate_homography, estimate_motion, exposure_chain, lucas_kanade_single_scale, mosaic_chain,
                               mosaic_composite, mosaic_median, refine_alignment, alignment_weights,
                               rgb_to_luma, sequence_refine_alignment, stabilize_trajectory, tracks_homography, tracks_motion, warp_affine,
                               warp_perspective)

SCRIPT_DIR = Path(__file__).resolve().parent
PROJECT_ROOT = SCRIPT_DIR.parent
DEFAULT_FRAME_DIR = PROJECT_ROOT / "tb" / "test_frames"

_i32p = ctypes.POINTER(ctypes.c_int)
_f32p = ctypes.POINTER(ctypes.c_float)


def _say(msg: str) -> None:
    if os.environ.get("OFLK_QUIET", "0") != "1":
        print(msg)


def pyramid_level_shapes(shape: Tuple[int, int], num_levels: int, scale_factor: float = 0.5) -> List[Tuple[int, int]]:
    """(H, W) per level, coarse to fine: int(H * scale_factor) per step (reference :51-52)."""
    dims = (ctypes.c_int * (2 * num_levels))()
    _oflk.check(_oflk.lib().oflk_pyramid_level_dims(int(shape[0]), int(shape[1]), int(num_levels),
                                                    float(scale_factor), dims))
    return [(dims[2 * l], dims[2 * l + 1]) for l in range(num_levels)]


def build_gaussian_pyramid(
    image: npt.NDArray[np.float32], num_levels: int, scale_factor: float = 0.5
) -> List[npt.NDArray[np.float32]]:
    """Gaussian pyramid, list from coarse (smallest) to fine (original).

    Replaces reference lucas_kanade_pyramidal.py:23-63 (oflk_build_pyramid):
    gaussian_filter(sigma = 1/scale_factor) then bilinear sampling on a linspace grid.
    """
    img = _oflk.as_f32(image)
    H, W = img.shape
    if num_levels < 1:
        return []  # range(0) in the reference: nothing is appended
    shapes = pyramid_level_shapes((H, W), num_levels, scale_factor)
    levels = [np.empty(s, np.float32) for s in shapes]
    arr = (_f32p * num_levels)(*[_oflk.ptr(a) for a in levels])
    # The Gaussian weights as SciPy forms them (scipy/ndimage/_filters.py _gaussian_kernel1d: NumPy's exp, normalised by
    # the kernel's sum), handed to the library: its own fallback for sigma != 2 is libm's exp, which differs from NumPy's
    # in the last bit for some arguments.  With the caller's weights every scale factor gives the reference's values.
    sigma = 1.0 / float(scale_factor)   # :46
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    w = np.ascontiguousarray(phi[radius:], np.float64)
    _oflk.check(_oflk.lib().oflk_build_pyramid_w(_oflk.ptr(img), H, W, int(num_levels), float(scale_factor),
                                                 w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), radius, arr))
    return levels


def warp_image(
    image: npt.NDArray[np.float32],
    flow_u: npt.NDArray[np.float32],
    flow_v: npt.NDArray[np.float32],
) -> npt.NDArray[np.float32]:
    """Bilinear backward warp: out[y, x] = image(y + v[y, x], x + u[y, x]), 0 outside.

    Replaces reference lucas_kanade_pyramidal.py:66-97 (oflk_warp).
    """
    img, u, v = _oflk.as_f32(image), _oflk.as_f32(flow_u), _oflk.as_f32(flow_v)
    H, W = _oflk.same_shape(img, u, v)
    out = np.empty((H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_warp(_oflk.ptr(img), _oflk.ptr(u), _oflk.ptr(v), H, W, _oflk.ptr(out)))
    return out


def upsample_flow(
    flow_u: npt.NDArray[np.float32],
    flow_v: npt.NDArray[np.float32],
    target_shape: Tuple[int, int],
) -> Tuple[npt.NDArray[np.float32], npt.NDArray[np.float32]]:
    """Bilinear flow upsampling with magnitudes scaled by the resolution ratio.

    Replaces reference lucas_kanade_pyramidal.py:100-138 (oflk_upsample_flow).
    """
    u, v = _oflk.as_f32(flow_u), _oflk.as_f32(flow_v)
    Hc, Wc = _oflk.same_shape(u, v)
    Ht, Wt = int(target_shape[0]), int(target_shape[1])
    uo = np.empty((Ht, Wt), np.float32)
    vo = np.empty((Ht, Wt), np.float32)
    _oflk.check(_oflk.lib().oflk_upsample_flow(_oflk.ptr(u), _oflk.ptr(v), Hc, Wc, Ht, Wt,
                                               _oflk.ptr(uo), _oflk.ptr(vo)))
    return uo, vo


def lucas_kanade_pyramidal_with_log(
    frame_prev, frame_curr, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3
):
    """Like lucas_kanade_pyramidal but silent; returns (u, v, residual_log, iters_run).

    residual_log[l, k] = (mean|du|, mean|dv|) of iteration k at level l (coarse first);
    iters_run[l] = iterations executed at level l.
    """
    log = np.zeros((max(num_levels, 1), max(num_iterations, 1), 2), np.float32)
    runs = np.zeros(max(num_levels, 1), np.int32)
    p, c, u8 = _pair(frame_prev, frame_curr)
    H, W = _oflk.same_shape(p, c)
    u = np.empty((H, W), np.float32)
    v = np.empty((H, W), np.float32)
    src, fn = _oflk.pixels(p, "oflk_pyramidal")
    _oflk.check(fn(src, _oflk.pix(c), *((1,) if u8 else ()), H, W, int(num_levels), int(window_size), int(num_iterations),
                   _oflk.ptr(u), _oflk.ptr(v), _oflk.ptr(log), runs.ctypes.data_as(_i32p)))
    return u, v, log, runs


def lucas_kanade_pyramidal(
    frame_prev: npt.NDArray[np.float32],
    frame_curr: npt.NDArray[np.float32],
    num_levels: int = 3,
    window_size: int = 5,
    num_iterations: int = 3,
) -> Tuple[npt.NDArray[np.float32], npt.NDArray[np.float32]]:
    """Coarse-to-fine pyramidal Lucas-Kanade flow (u, v) at the input resolution.

    Replaces reference lucas_kanade_pyramidal.py:141-228 (oflk_pyramidal).
    """
    u, v, log, runs = lucas_kanade_pyramidal_with_log(frame_prev, frame_curr, num_levels,
                                                      window_size, num_iterations)

    shapes = pyramid_level_shapes(np.shape(frame_prev), num_levels)
    H, W = int(np.shape(frame_prev)[0]), int(np.shape(frame_prev)[1])
    key = (1, H, W, int(num_levels), int(window_size), int(num_iterations))
    # exit decisions taken too close to the 0.01 threshold were redone by the library in NumPy's own summation order
    # (oflk_plan_resolve_uncertain, see oflk.h): the result is the reference's either way; say so when it happened
    resolved = int(_oflk.lib().oflk_last_resolved())
    _say(f"Building {num_levels}-level Gaussian pyramids...")
    _say("Pyramid levels:")
    for i, (h, w) in enumerate(shapes):
        _say(f"  Level {i}: {w}x{h} pixels")
    for level in range(num_levels):
        _say(f"\nProcessing pyramid level {level}/{num_levels-1}...")
        if level > 0:
            _say(f"  Upsampled flow to {shapes[level][1]}x{shapes[level][0]}")
        for it in range(int(runs[level])):
            mu, mv = log[level, it]
            _say(f"  Iteration {it+1}/{num_iterations}: mean residual = ({mu:.4f}, {mv:.4f})")
            if mu < 0.01 and mv < 0.01:
                _say(f"  Converged after {it+1} iterations")
    if resolved:
        _say("  note: an exit decision of this pair lay within the summation error of the 0.01 threshold and was "
             "re-evaluated in NumPy's summation order")
    if os.environ.get("OFLK_DUMP_LEVELS", "0") == "1":
        _dump_levels(key, shapes, u, v)
    return u, v


def lucas_kanade_pyramidal_sequence_with_log(frames, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3):
    """Flows (t -> t+1) of a frame sequence, silently; returns (u, v, residual_log, iters_run).

    frames: a (T, H, W) array or a sequence of T 2-D arrays, T >= 2 (all uint8: the uint8 path, as for a pair).
    u, v are (T-1, H, W) float32; residual_log is (T-1, levels, iters, 2) and iters_run (T-1, levels), each pair's entries
    as lucas_kanade_pyramidal_with_log gives them.  Every flow equals that of the pair (frames[t], frames[t+1]); the
    library uploads each frame once and builds its pyramid once.  The reference has no sequence function: nothing is printed.
    """
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    log = np.zeros((T - 1, max(num_levels, 1), max(num_iterations, 1), 2), np.float32)
    runs = np.zeros((T - 1, max(num_levels, 1)), np.int32)
    u = np.empty((T - 1, H, W), np.float32)
    v = np.empty((T - 1, H, W), np.float32)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence")
    _oflk.check(fn(src, T, H, W, int(num_levels), int(window_size), int(num_iterations), _oflk.ptr(u), _oflk.ptr(v), _oflk.ptr(log),
                   runs.ctypes.data_as(_i32p)))
    return u, v, log, runs


def lucas_kanade_pyramidal_sequence(frames, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3):
    """(u, v), each (T-1, H, W) float32: the pyramidal flow of every consecutive pair of a (T, H, W) frame sequence."""
    u, v, _, _ = lucas_kanade_pyramidal_sequence_with_log(frames, num_levels, window_size, num_iterations)
    return u, v


class SequenceFB(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_fb; every field is (T-1, H, W).  Index t is the pair (frames[t],
    frames[t+1]): *_fwd fields live on frame t's grid, *_bwd fields on frame t+1's."""
    u_fwd: np.ndarray      # flow frames[t] -> frames[t+1] (float32)
    v_fwd: np.ndarray
    u_bwd: np.ndarray      # flow frames[t+1] -> frames[t] (float32)
    v_bwd: np.ndarray
    err_fwd: np.ndarray    # |F + G(x + F)| in px (float32)
    err_bwd: np.ndarray    # |G + F(x + G)| in px (float32)
    valid_fwd: np.ndarray  # bool: the forward vector passes the forward-backward test
    valid_bwd: np.ndarray


def lucas_kanade_pyramidal_sequence_fb(frames, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                       alpha: float = 0.01, beta: float = 0.5, flow_median: int = 0) -> SequenceFB:
    """Forward and backward flows of every consecutive pair of a frame sequence, and their consistency.

    frames: a (T, H, W) array or a sequence of T 2-D arrays, T >= 2 (all uint8: the uint8 path).  u_fwd / v_fwd equal
    lucas_kanade_pyramidal_sequence(frames); u_bwd[t] / v_bwd[t] equal the flow of the pair (frames[t+1], frames[t]).  A
    forward vector is valid when its target lies inside frame t+1 and |F + G(x + F)|^2 <= alpha (|F|^2 + |G(x + F)|^2) +
    beta (Sundaram, Brox & Keutzer 2010; G(x + F) is warp_image's bilinear sample, 0 outside the frame); the backward test
    is the same with F and G exchanged.  Each frame is uploaded once and its pyramid built once for both directions.
    flow_median = 3, 5, 7 or 9: the four flows go through median_filter_flow of that size on the device before the test; the
    filtered flows are the ones returned and tested.
    """
    a, b = _oflk.check_fb_params(alpha, beta)
    k = _oflk.check_flow_median(flow_median)
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    out = [np.empty((T - 1, H, W), np.float32) for _ in range(6)]
    valid = [np.empty((T - 1, H, W), np.uint8) for _ in range(2)]
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_fb" + ("_median" if k else ""))
    _oflk.check(fn(src, T, H, W, int(num_levels), int(window_size), int(num_iterations), a, b, *((k,) if k else ()),
                   *(_oflk.ptr(o) for o in out), valid[0].ctypes.data, valid[1].ctypes.data))
    return SequenceFB(*out[:4], out[4], out[5], valid[0].astype(bool), valid[1].astype(bool))


def median_filter_flow(flow, size: int = 5):
    """The size x size median (size 3, 5, 7 or 9) of every plane of a float32 array (..., H, W), the same shape: each output
    value is the middle one of the window's size^2 values, the border replicated, in the order of the values' bits (-NaN <
    -inf < ... < -0 < +0 < ... < +inf < +NaN), so it is one of the inputs, bit for bit.  Of a flow this is the component-wise
    median of u and of v: the standard regulariser of a local flow method."""
    return _oflk.flow_median_host(flow, size)


class SequenceTracks(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_tracks: row t is frame t."""
    tracks: np.ndarray    # (T, N, 2) float32 (x, y); NaN where not visible
    visible: np.ndarray   # (T, N) bool


def lucas_kanade_pyramidal_sequence_tracks(frames, queries, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                           alpha: float = 0.01, beta: float = 0.5) -> SequenceTracks:
    """Point tracks through a frame sequence, stopped at occlusions.

    frames: as lucas_kanade_pyramidal_sequence_fb (all uint8: the uint8 path).  queries: (N, 3) (t, x, y) or (N, 2) (x, y,
    at frame 0), x along W.  Each point starts on its frame and follows the forward flow (bilinear samples at its float32
    position) while every step passes the forward-backward test of lucas_kanade_pyramidal_sequence_fb at that position
    (alpha, beta); the track ends at the first step that fails or leaves the frame, and a point outside the frame never
    starts.  The flows stay on the device: only the tracks come back.
    """
    a, b = _oflk.check_fb_params(alpha, beta)
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    qt, qxy = _oflk.as_queries(queries, T)
    N = qxy.shape[0]
    tracks, visible = np.empty((T, N, 2), np.float32), np.empty((T, N), np.uint8)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_tracks")
    _oflk.check(fn(src, T, H, W, int(num_levels), int(window_size), int(num_iterations), a, b,
                   None if qt is None else qt.ctypes.data_as(_oflk._i32p), _oflk.ptr(qxy), N, _oflk.ptr(tracks),
                   visible.ctypes.data))
    return SequenceTracks(tracks, visible.astype(bool))


def _interp_layout(frames, order, what):
    """(layout, contiguous array, H, W) of grey frames (the default layout) or of a 4-D uint8 array of colour frames"""
    if _oflk.is_packed(frames):
        arr = _oflk.as_packed(frames, what)
        if arr.shape[0] < 2:
            raise ValueError(f"a sequence needs at least 2 frames, got {arr.shape[0]}")
        return _oflk.FrameLayout("_packed", (arr.shape[3], _oflk.check_colour_order(order))), arr, arr.shape[1], arr.shape[2]
    arr, _ = _oflk.as_sequence(frames)
    return _oflk.FrameLayout(), arr, arr.shape[1], arr.shape[2]


def _interp_nv12(frames, siting, what):
    code = _oflk.check_nv12_siting(siting)
    arr = _oflk.as_nv12(frames, what)
    if arr.shape[0] < 2:
        raise ValueError(f"a sequence needs at least 2 frames, got {arr.shape[0]}")
    return _oflk.FrameLayout("_nv12", (code,)), arr, 2 * arr.shape[1] // 3, arr.shape[2]


def _interpolate_frames(layout, arr, H, W, flows, cfg, return_status):
    new, status = _oflk.interpolate_host(layout, arr, H, W, flows, cfg, bool(return_status))
    return (new, status) if return_status else new


def interpolate_frames(frames, u_fwd, v_fwd, u_bwd, v_bwd, taus=(0.5,), alpha: float = 0.01, beta: float = 0.5, refine: int = 2,
                       return_status: bool = False):
    """In-between frames of a (B+1, H, W) frame sequence on given dense flows, motion compensated.

    frames: as lucas_kanade_pyramidal_sequence_fb (all uint8: the uint8 path); the flows are (B, H, W) float32 as that call
    returns them.  Returns new (B, n, H, W) in the frames' type, new[b, j] at time taus[j] in (0, 1) between frames b and
    b+1; with return_status also status (B, n, H, W) uint8: bit 0 the sample of frame b passed, bit 1 that of frame b+1.
    Each side solves p + s F(p) = (x, y) by `refine` fixed-point steps (gathers only), samples its frame at p when p and its
    target pass the forward-backward test (alpha, beta), and the two are blended by tau; where only one side passes it is
    taken alone, where neither does the frames are cross-faded.
    A 4-D uint8 array (B+1, H, W, C), C = 3 or 4, is interleaved colour: new is (B, n, H, W, C), every channel the grey result
    of its plane from one solve per pixel, and status stays (B, n, H, W).
    """
    cfg = _oflk.check_interp(alpha, beta, refine, taus)
    layout, arr, H, W = _interp_layout(frames, "rgb", "(B+1, H, W, C)")
    return _interpolate_frames(layout, arr, H, W, (u_fwd, v_fwd, u_bwd, v_bwd), cfg, return_status)


def interpolate_frames_nv12(video, u_fwd, v_fwd, u_bwd, v_bwd, taus=(0.5,), siting: str = "left", alpha: float = 0.01,
                            beta: float = 0.5, refine: int = 2, return_status: bool = False):
    """interpolate_frames for NV12 frames, both planes in one launch: video (B+1, 3H/2, W) uint8 (nv12_from_planes), the flows
    (B, H, W) those of the Y planes.  new is (B, n, 3H/2, W): its Y plane is interpolate_frames' on the Y planes, a chroma
    sample solves from its luma position (`siting`: "left" or "center") and samples U and V there, clamped to the chroma
    plane; status (B, n, H, W) is the Y plane's."""
    cfg = _oflk.check_interp(alpha, beta, refine, taus)
    layout, arr, H, W = _interp_nv12(video, siting, "(B+1, 3H/2, W)")
    return _interpolate_frames(layout, arr, H, W, (u_fwd, v_fwd, u_bwd, v_bwd), cfg, return_status)


class SequenceInterpolated(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_interpolate on T frames and n times a pair; a frame is (H, W), (H, W, C) for
    colour or (3H/2, W) for NV12"""
    frames: np.ndarray   # ((T-1) * n + T,) + frame in the input type: the originals and the new frames in time order
    new: np.ndarray      # (T-1, n) + frame: new[t, j] at time taus[j] between frames t and t+1
    status: np.ndarray   # (T-1, n, H, W) uint8: bit 0 frame t's sample passed, bit 1 frame t+1's


def _sequence_interpolate(layout, arr, H, W, num_levels, window_size, num_iterations, cfg, flow_median=0) -> SequenceInterpolated:
    new, status = _oflk.interpolate_sequence_host(layout, arr, H, W, num_levels, window_size, num_iterations, cfg, flow_median)
    T, n = arr.shape[0], len(cfg.taus)
    both = np.empty((T - 1, n + 1) + arr.shape[1:], arr.dtype)   # frame t, then its n new frames
    both[:, 0], both[:, 1:] = arr[:-1], new
    return SequenceInterpolated(np.concatenate([both.reshape((-1,) + arr.shape[1:]), arr[-1:]]), new, status)


def lucas_kanade_pyramidal_sequence_interpolate(frames, factor: int = 2, taus=None, num_levels: int = 3, window_size: int = 5,
                                                num_iterations: int = 3, alpha: float = 0.01, beta: float = 0.5,
                                                refine: int = 2, order: str = "rgb", flow_median: int = 0) -> SequenceInterpolated:
    """Frame-rate conversion: frames in, the in-between frames of every consecutive pair out.

    factor=k inserts the k-1 frames at times j / k, j = 1 .. k-1 (formed in float64); explicit taus (ascending for `frames`
    to be in time order) override it.  The flows of lucas_kanade_pyramidal_sequence_fb and the interpolation of
    interpolate_frames run on the device: only the new frames and their status come back.
    A 4-D uint8 array (T, H, W, C), C = 3 or 4, is interleaved colour: the flows are tracked on its luma (rgb_to_luma, `order`
    "rgb" or "bgr"), formed on the device, and every channel is interpolated on them.
    flow_median = 3, 5, 7 or 9: the flows go through median_filter_flow of that size, on the device, before they are used.
    """
    cfg = _oflk.check_interp(alpha, beta, refine, taus, factor)
    k = _oflk.check_flow_median(flow_median)
    layout, arr, H, W = _interp_layout(frames, order, "(T, H, W, C)")
    return _sequence_interpolate(layout, arr, H, W, num_levels, window_size, num_iterations, cfg, k)


def lucas_kanade_pyramidal_sequence_interpolate_nv12(video, factor: int = 2, taus=None, num_levels: int = 3, window_size: int = 5,
                                                     num_iterations: int = 3, alpha: float = 0.01, beta: float = 0.5,
                                                     refine: int = 2, siting: str = "left",
                                                     flow_median: int = 0) -> SequenceInterpolated:
    """lucas_kanade_pyramidal_sequence_interpolate for NV12 video (T, 3H/2, W) uint8 (nv12_from_planes): the flows are tracked
    on the Y planes where they lie, and both planes of the new frames come from interpolate_frames_nv12's kernel."""
    cfg = _oflk.check_interp(alpha, beta, refine, taus, factor)
    k = _oflk.check_flow_median(flow_median)
    layout, arr, H, W = _interp_nv12(video, siting, "(T, 3H/2, W)")
    return _sequence_interpolate(layout, arr, H, W, num_levels, window_size, num_iterations, cfg, k)


def denoise_frames(frames, u_fwd, v_fwd, u_bwd, v_bwd, strength: float, radius: int = 2, alpha: float = 0.01, beta: float = 4.0,
                   return_count: bool = False):
    """Temporal noise reduction of a (B+1, H, W) frame sequence on given dense flows, motion compensated.

    frames: as lucas_kanade_pyramidal_sequence_fb (all uint8: the uint8 path); the flows are (B, H, W) float32 as that call
    returns them.  Returns the frames' shape and type: each pixel averaged with where it was in the `radius` frames before and
    after (fewer at the ends of the sequence).  A pixel is carried from frame to frame along the flows while every step
    passes the forward-backward test (alpha, beta) at the carried point; a chain ends at its first failure.  A neighbour v of
    the pixel c has the weight 1 - (v - c)^2 / strength^2 where that is positive and none otherwise, so a value `strength`
    grey levels or more away never enters; 3 x the noise's sigma is the suggested strength.  With return_count also count
    (B+1, H, W) uint8, the neighbours that entered each average (2 * radius at most).
    """
    cfg = _oflk.check_denoise(alpha, beta, radius, strength)
    arr, _ = _oflk.as_sequence(frames)
    out, count = _oflk.denoise_host(arr, (u_fwd, v_fwd, u_bwd, v_bwd), cfg, bool(return_count))
    return (out, count) if return_count else out


def lucas_kanade_pyramidal_sequence_denoise(frames, strength: float, radius: int = 2, alpha: float = 0.01, beta: float = 4.0,
                                            flow_median: int = 9, num_levels: int = 3, window_size: int = 5,
                                            num_iterations: int = 3, return_count: bool = False):
    """Temporal noise reduction of a frame sequence: frames in, the denoised frames out, (T, H, W) in the frames' type.

    The flows of lucas_kanade_pyramidal_sequence_fb (flow_median = 3, 5, 7 or 9: through median_filter_flow of that size; 0:
    as they are) and the average of denoise_frames run on the device: only the frames (and with return_count the counts)
    come back, and a long sequence goes in chunks whose cut does not show in the result.  The defaults are the ones the
    feature works with on this library's flows of noisy frames: the 9 x 9 median and a forward-backward test looser
    (beta = 4.0) than the other callers'.
    """
    cfg = _oflk.check_denoise(alpha, beta, radius, strength)
    k = _oflk.check_flow_median(flow_median)
    arr, _ = _oflk.as_sequence(frames)
    out, count = _oflk.denoise_sequence_host(arr, num_levels, window_size, num_iterations, cfg, k, bool(return_count))
    return (out, count) if return_count else out


class SequenceKLT(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_klt: n features of frame 0 and their tracks (row t is frame t)."""
    xy: np.ndarray        # (n, 2) float32 (x, y) in acceptance order
    tracks: np.ndarray    # (T, n, 2) float32 (x, y); NaN where not visible
    visible: np.ndarray   # (T, n) bool


def lucas_kanade_pyramidal_sequence_klt(frames, max_corners: int, quality_level: float = 0.01, min_distance: float = 10.0,
                                        num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                        alpha: float = 0.01, beta: float = 0.5) -> SequenceKLT:
    """Detect, then track (KLT): Shi-Tomasi features of frame 0 (lucas_kanade_core.good_features_to_track, with the LK
    window_size as the detection window, so it must be odd in [3, 11]) followed by lucas_kanade_pyramidal_sequence_tracks
    on them.  The features are born on the device; only they and the tracks come back.  frames: as
    lucas_kanade_pyramidal_sequence_fb (all uint8: the uint8 path).
    """
    a, b = _oflk.check_fb_params(alpha, beta)
    K, q, md, win = _oflk.check_feature_params(max_corners, quality_level, min_distance, window_size)
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    count = np.zeros(1, np.int32)
    xy, score = np.empty((K, 2), np.float32), np.empty(K, np.float32)
    tracks, visible = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_klt")
    _oflk.check(fn(src, T, H, W, int(num_levels), win, int(num_iterations), a, b, q, md, K, count.ctypes.data_as(_oflk._i32p),
                   _oflk.ptr(xy), _oflk.ptr(score), _oflk.ptr(tracks), visible.ctypes.data))
    n = int(count[0])
    return SequenceKLT(xy[:n], tracks[:, :n], visible[:, :n].astype(bool))


def lucas_kanade_sparse(frame_prev, frame_curr, points, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3):
    """Sparse pyramidal Lucas-Kanade of one pair (the shape of calcOpticalFlowPyrLK): points (N, 2) (x, y) of frame_prev ->
    (next_points (N, 2) float32, status (N,) bool, residual (N,) float32: the mean absolute difference of the two windows).

    Per point and pyramid level a (window_size + 2)^2 template patch and, per iteration, the patch around the displaced
    point are sampled bilinearly and solved with the reference's single-scale operations; the cost is proportional to
    N * window_size^2 * num_levels * num_iterations, and no flow field exists anywhere.  status is False where the last
    2x2 system had no solution or the point left the frame; a point outside the frame gives NaN.  Both frames uint8: the
    uint8 path."""
    p, c, _ = _pair(frame_prev, frame_curr)
    H, W = _oflk.same_shape(p, c)
    L, win, K, _ = _oflk.check_sparse_params((H, W), num_levels, window_size, num_iterations)
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1:
        raise ValueError(f"points must be an (N, 2) (x, y) array with N >= 1, got shape {pts.shape}")
    pts = np.ascontiguousarray(pts, np.float32)
    N = pts.shape[0]
    nxt, status, res = np.empty((N, 2), np.float32), np.empty(N, np.uint8), np.empty(N, np.float32)
    src, fn = _oflk.pixels(p, "oflk_sparse_lk")
    _oflk.check(fn(src, _oflk.pix(c), H, W, L, win, K, _oflk.ptr(pts), N, _oflk.ptr(nxt), status.ctypes.data, _oflk.ptr(res)))
    return nxt, status.astype(bool), res


def lucas_kanade_pyramidal_sequence_sparse_tracks(frames, queries, num_levels: int = 3, window_size: int = 5,
                                                  num_iterations: int = 3, alpha: float = 0.01, beta: float = 0.5,
                                                  max_residual: float = 4.0) -> SequenceTracks:
    """lucas_kanade_pyramidal_sequence_tracks with the sparse tracker: every step of a point is lucas_kanade_sparse forward,
    then backward from where it landed, and the point stays alive while both succeed, the two displacements pass the
    forward-backward test (alpha, beta) and the forward residual is at most max_residual (grey levels; inf: no such test).
    No dense flow is computed: only frames go up and rows come down.  frames, queries and the result as
    lucas_kanade_pyramidal_sequence_tracks."""
    a, b = _oflk.check_fb_params(alpha, beta)
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    L, win, K, r = _oflk.check_sparse_params((H, W), num_levels, window_size, num_iterations, max_residual)
    qt, qxy = _oflk.as_queries(queries, T)
    N = qxy.shape[0]
    tracks, visible = np.empty((T, N, 2), np.float32), np.empty((T, N), np.uint8)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_sparse_tracks")
    _oflk.check(fn(src, T, H, W, L, win, K, a, b, r, None if qt is None else qt.ctypes.data_as(_oflk._i32p), _oflk.ptr(qxy), N,
                   _oflk.ptr(tracks), visible.ctypes.data))
    return SequenceTracks(tracks, visible.astype(bool))


def _tracking(frames, num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level, min_distance,
              detect_every=None):
    """(the frames of a sequence as as_sequence gives them, their checked _oflk.Tracking), refused in the sparse sequence
    calls' order: alpha and beta, the frames, then check_tracking's"""
    _oflk.check_fb_params(alpha, beta)
    arr, _ = _oflk.as_sequence(frames)
    return arr, _oflk.check_tracking(arr.shape[1:], num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners,
                                     quality_level, min_distance, detect_every)


def lucas_kanade_pyramidal_sequence_klt_sparse(frames, max_corners: int, quality_level: float = 0.01, min_distance: float = 10.0,
                                               num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                               alpha: float = 0.01, beta: float = 0.5, max_residual: float = 4.0) -> SequenceKLT:
    """Detect, then track, sparsely: good_features_to_track on frame 0 (the LK window is the detection window), then
    lucas_kanade_pyramidal_sequence_sparse_tracks on those points, in one call: the features are born on the device,
    straight into the tracker's query buffer.  Result as lucas_kanade_pyramidal_sequence_klt."""
    arr, trk = _tracking(frames, num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level,
                         min_distance)
    (T, H, W), K = arr.shape, trk.max_corners
    count = np.zeros(1, np.int32)
    xy, score = np.empty((K, 2), np.float32), np.empty(K, np.float32)
    tracks, visible = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_klt_sparse")
    _oflk.check(fn(src, T, H, W, *trk.klt, count.ctypes.data_as(_oflk._i32p), _oflk.ptr(xy), _oflk.ptr(score), _oflk.ptr(tracks),
                   visible.ctypes.data))
    n = int(count[0])
    return SequenceKLT(xy[:n], tracks[:, :n], visible[:, :n].astype(bool))


class SequenceKLTReplenish(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_klt_replenish: K slots, row t is frame t.  A slot holds one track at a
    time; lucas_kanade_core.split_tracks(visible, born) lists them."""
    tracks: np.ndarray     # (T, K, 2) float32 (x, y); NaN where not visible
    visible: np.ndarray    # (T, K) bool
    born: np.ndarray       # (T, K) bool: a new track begins in this slot on this frame
    detected: np.ndarray   # (T,) int32: points born on each frame


def lucas_kanade_pyramidal_sequence_klt_replenish(frames, max_corners: int, detect_every: int, quality_level: float = 0.01,
                                                  min_distance: float = 10.0, num_levels: int = 3, window_size: int = 5,
                                                  num_iterations: int = 3, alpha: float = 0.01,
                                                  beta: float = 0.5) -> SequenceKLTReplenish:
    """KLT with replenishment: lucas_kanade_pyramidal_sequence_klt over max_corners slots, detecting again on every
    detect_every-th frame (0, D, 2D, .. below the last) away from the live tracks and starting the new points in the
    slots whose tracks have ended (lucas_kanade_core.replenish_features is one such detection).  Frames go up and the
    rows come down; the flows, the detections and the hand-over between them stay on the device.  With detect_every >=
    the number of frames the tracks are lucas_kanade_pyramidal_sequence_klt's, over all K slots.
    """
    a, b = _oflk.check_fb_params(alpha, beta)
    K, q, md, win = _oflk.check_feature_params(max_corners, quality_level, min_distance, window_size)
    every = _oflk.check_detect_every(detect_every)
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    tracks, visible = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    born, detected = np.empty((T, K), np.uint8), np.empty(T, np.int32)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_klt_replenish")
    _oflk.check(fn(src, T, H, W, int(num_levels), win, int(num_iterations), a, b, q, md, K, every, _oflk.ptr(tracks),
                   visible.ctypes.data, born.ctypes.data, detected.ctypes.data_as(_oflk._i32p)))
    return SequenceKLTReplenish(tracks, visible.astype(bool), born.astype(bool), detected)


class SequenceKLTSparseReplenish(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_klt_sparse_replenish: SequenceKLTReplenish's fields and the steps' residuals."""
    tracks: np.ndarray     # (T, K, 2) float32 (x, y); NaN where not visible
    visible: np.ndarray    # (T, K) bool
    born: np.ndarray       # (T, K) bool: a new track begins in this slot on this frame
    detected: np.ndarray   # (T,) int32: points born on each frame
    residual: np.ndarray   # (T, K) float32: the forward residual of the step into row t of a slot alive on row t-1; else NaN


def lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, max_corners: int, detect_every: int,
                                                         quality_level: float = 0.01, min_distance: float = 10.0,
                                                         num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                                         alpha: float = 0.01, beta: float = 0.5,
                                                         max_residual: float = 4.0) -> SequenceKLTSparseReplenish:
    """lucas_kanade_pyramidal_sequence_klt_replenish on the sparse tracker: max_corners slots, a detection on every
    detect_every-th frame away from the live tracks, and between them the steps of
    lucas_kanade_pyramidal_sequence_sparse_tracks -- no flow field anywhere.  residual[t, n] is the forward step's mean
    absolute window difference (what max_residual is compared with) for every slot that was alive on frame t-1 and whose
    forward step succeeded, also where the track ends on that step; NaN elsewhere.  lucas_kanade_core.split_tracks(visible,
    born) lists the tracks.  Frames go up; the rows come down."""
    arr, trk = _tracking(frames, num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level,
                         min_distance, detect_every)
    (T, H, W), K = arr.shape, trk.max_corners
    tracks, visible = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    born, detected = np.empty((T, K), np.uint8), np.empty(T, np.int32)
    residual = np.empty((T, K), np.float32)
    src, fn = _oflk.pixels(arr, "oflk_pyramidal_sequence_klt_sparse_replenish")
    _oflk.check(fn(src, T, H, W, *trk, _oflk.ptr(tracks), visible.ctypes.data, born.ctypes.data, detected.ctypes.data_as(_oflk._i32p),
                   _oflk.ptr(residual)))
    return SequenceKLTSparseReplenish(tracks, visible.astype(bool), born.astype(bool), detected, residual)


class SequenceStabilized(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_stabilize."""
    frames: np.ndarray      # (T, H, W) -- (T, H, W, C) for colour --, the input's type: the steadied frames, zero outside
    correction: np.ndarray  # (T, 2, 3) float32: where frame t's content was moved to (Trajectory.correction)
    model: np.ndarray       # (T-1, 2, 3) float32: the fitted motion of step t -> t+1; NaN where status is 0
    status: np.ndarray      # (T-1,) int32: 1 where a model was found
    held: np.ndarray        # (T-1,) bool: the step counted as no motion


def lucas_kanade_pyramidal_sequence_stabilize(frames, max_corners: int, detect_every: int, model: str = "similarity",
                                              radius: int = 15, sigma=None, hypotheses: int = 256, threshold: float = 1.0,
                                              seed: int = 0, quality_level: float = 0.01, min_distance: float = 10.0,
                                              num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                              alpha: float = 0.01, beta: float = 0.5, max_residual: float = 4.0,
                                              refine_iterations: int = 0, refine_levels: int = 3,
                                              order: str = "rgb", refine_photometric: bool = False,
                                              refine_robust_delta=None) -> SequenceStabilized:
    """Frames in, steadied frames out: lucas_kanade_pyramidal_sequence_klt_sparse_replenish on the frames, tracks_motion on
    its rows, stabilize_trajectory on the models and warp_affine of the frames under its maps, in one call whose
    intermediate rows stay in the library.  The frames go up twice, chunk by chunk (once to track, once to warp); nothing
    of the sequence's size is ever on the device.  The black border is not cropped (warp_affine's inside mask tells where
    it is).

    refine_iterations > 0: the same chain made of its public parts, with sequence_refine_alignment (kind "affine",
    refine_levels levels, refine_iterations iterations each) between the fit and the trajectory: every fitted step is refined
    on the pixels of its two frames, and a step that cannot be refined keeps the fitted model.  refine_photometric=True
    (needs refine_iterations > 0) refines every step together with a gain and a bias, for video whose exposure changes; the
    stabiliser only uses the better models, the frames keep their values.  refine_robust_delta (grey levels, e.g. 4.0; needs
    refine_iterations > 0) is sequence_refine_alignment's robust_delta: Huber weights, so that an object moving through the
    shot does not pull the refined steps.

    A 4-D uint8 array (T, H, W, C), C = 3 or 4, is interleaved colour video with R, G and B where `order` ("rgb" or "bgr")
    says: the motion is tracked, fitted and (with refine_iterations) refined on rgb_to_luma of the frames, exactly as this
    call does on that luma, and the colour frames are warped under the maps of that trajectory, every channel at one source
    position; .frames then has the input's shape."""
    refine = _oflk.check_refine(refine_iterations, refine_photometric, refine_robust_delta)
    code_order = _oflk.check_colour_order(order)
    if _oflk.is_packed(frames):
        packed = _oflk.as_packed(frames, "(T, H, W, C)")
        video = _Video(lambda: (packed,) + packed.shape[1:3], _oflk.FrameLayout("_packed", (packed.shape[3], code_order)),
                       lambda: rgb_to_luma(packed, order), lambda grey, maps: warp_affine(packed, maps))
    else:
        def grey_frames():
            arr, _ = _oflk.as_sequence(frames)
            return (arr,) + arr.shape[1:]
        video = _Video(grey_frames, _oflk.FrameLayout(), lambda: frames, warp_affine)
    return _sequence_stabilize(video, max_corners, detect_every, model, radius, sigma, hypotheses, threshold, seed, quality_level,
                               min_distance, num_levels, window_size, num_iterations, alpha, beta, max_residual, refine, refine_levels,
                               refine_photometric, refine_robust_delta)


class _Video(NamedTuple):
    """What differs between the grey, the interleaved colour and the NV12 form of the sequence stabiliser"""
    frames: Callable    # () -> (the contiguous frames as the C call takes them, H, W); called once alpha and beta are checked
    layout: "_oflk.FrameLayout"   # names the form of oflk_stabilize_sequence* and holds its arguments behind H, W
    luma: Callable      # () -> the grey frames that the refine chain tracks, fits and refines on
    warp: Callable      # (those grey frames as an array, maps (T, 2, 3)) -> the refined path's steadied frames


def _sequence_stabilize(video: _Video, max_corners, detect_every, model, radius, sigma, hypotheses, threshold, seed, quality_level,
                        min_distance, num_levels, window_size, num_iterations, alpha, beta, max_residual, refine: int, refine_levels,
                        refine_photometric, refine_robust_delta) -> SequenceStabilized:
    """the one body of lucas_kanade_pyramidal_sequence_stabilize and _stabilize_nv12, once the layout's own arguments are checked"""
    if refine > 0:
        grey = video.luma()
        rows = lucas_kanade_pyramidal_sequence_klt_sparse_replenish(grey, max_corners, detect_every, quality_level, min_distance,
                                                                    num_levels, window_size, num_iterations, alpha, beta, max_residual)
        fit = tracks_motion(rows.tracks, rows.visible, rows.born, model, hypotheses, threshold, seed)
        arr, _ = _oflk.as_sequence(grey)
        al = sequence_refine_alignment(arr, fit.model, fit.status, "affine", refine_levels, refine, photometric=bool(refine_photometric),
                                       robust_delta=refine_robust_delta)
        tr = stabilize_trajectory(al.model, fit.status, radius, sigma)
        return SequenceStabilized(video.warp(arr, tr.map), tr.correction, al.model, fit.status, tr.held)
    _oflk.check_fb_params(alpha, beta)
    arr, H, W = video.frames()
    T = arr.shape[0]
    if T < 2:
        raise ValueError(f"a sequence needs at least 2 frames, got {T}")
    trk = _oflk.check_tracking((H, W), num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level,
                               min_distance, detect_every)
    fit = _oflk.check_motion_params(model, hypotheses, threshold, seed)
    win = _oflk.check_window(radius, sigma)
    out = np.empty_like(arr)
    corr, mod = np.empty((T, 6), np.float32), np.empty((T - 1, 6), np.float32)
    cnt, held = np.empty((T - 1, 3), np.int32), np.empty(T - 1, np.uint8)
    if video.layout.suffix:
        src, fn = _oflk.pix(arr), getattr(_oflk.lib(), "oflk_stabilize_sequence" + video.layout.suffix)
    else:   # the grey form has the pixel type in its name
        src, fn = _oflk.pixels(arr, "oflk_stabilize_sequence")
    _oflk.check(fn(src, T, H, W, *video.layout.args, *trk, *fit, *win.args, _oflk.pix(out), _oflk.ptr(corr), _oflk.ptr(mod),
                   cnt.ctypes.data_as(_oflk._i32p), held.ctypes.data))
    return SequenceStabilized(out, corr.reshape(T, 2, 3), mod.reshape(T - 1, 2, 3), cnt[:, 2].copy(), held.astype(bool))


def nv12_planes(frames):
    """Views of the two planes of NV12 frames: an (F, 3H/2, W) or (3H/2, W) uint8 array -- rows 0 .. H-1 of a frame are its Y
    plane, the H/2 rows behind them its interleaved U, V pairs -- gives y (F, H, W) and uv (F, H/2, W/2, 2), or (H, W) and
    (H/2, W/2, 2).  H and W must be even and >= 4."""
    single = isinstance(frames, np.ndarray) and frames.ndim == 2
    arr = _oflk.as_nv12(frames[None] if single else frames, "(F, 3H/2, W) or (3H/2, W)")
    F, R, W = arr.shape
    H = 2 * R // 3
    y, uv = arr[:, :H, :], arr[:, H:, :].reshape(F, H // 2, W // 2, 2)
    return (y[0], uv[0]) if single else (y, uv)


def nv12_from_planes(y, uv):
    """NV12 frames from their planes, nv12_planes' inverse: y (F, H, W) and uv (F, H/2, W/2, 2) uint8 give (F, 3H/2, W);
    (H, W) and (H/2, W/2, 2) give (3H/2, W)."""
    y, uv = np.asarray(y), np.asarray(uv)
    if y.dtype != np.uint8 or uv.dtype != np.uint8:
        raise ValueError(f"NV12 planes must be uint8, got {y.dtype} and {uv.dtype}")
    single = y.ndim == 2
    if single:
        y, uv = y[None], uv[None]
    if y.ndim != 3 or uv.ndim != 4:
        raise ValueError(f"expected y (F, H, W) and uv (F, H/2, W/2, 2), got {y.shape} and {uv.shape}")
    F, H, W = y.shape
    if H % 2 or W % 2 or H < 4 or W < 4:
        raise ValueError(f"NV12 frames need even H and W >= 4, got {H} x {W}")
    if uv.shape != (F, H // 2, W // 2, 2):
        raise ValueError(f"expected uv of shape {(F, H // 2, W // 2, 2)} for y of shape {y.shape}, got {uv.shape}")
    out = np.concatenate([y, uv.reshape(F, H // 2, W)], axis=1)
    return out[0] if single else out


def _warp_nv12(frames, maps, siting, return_inside: bool, n: int):
    code = _oflk.check_nv12_siting(siting)
    single = isinstance(frames, np.ndarray) and frames.ndim == 2
    arr = _oflk.as_nv12(frames[None] if single else frames, "(F, 3H/2, W) or (3H/2, W)")
    F = arr.shape[0]
    out, ins = _oflk.warp_nv12_host(arr, _maps(maps, F, n), code, bool(return_inside))
    if single:
        out, ins = out[0], None if ins is None else ins[0]
    return (out, ins.astype(bool)) if return_inside else out


def warp_affine_nv12(frames, maps, siting: str = "left", return_inside: bool = False):
    """warp_affine for NV12 frames, both planes in one launch: frames (F, 3H/2, W) or (3H/2, W) uint8 (nv12_from_planes), maps
    as warp_affine's, in luma pixels.  The Y plane comes back as warp_affine returns it for that plane; U and V as
    warp_affine returns them for their H/2 x W/2 planes under the map restated in chroma coordinates, where chroma sample
    (i, j) sits at luma (2 i + sx, 2 j + sy): siting "left" is (0, 0.5), the H.264 / HEVC default, "center" (0.5, 0.5), as in
    JPEG.  Outside the frame Y is 0 and U = V = 128: black.  With return_inside also the (F, H, W) bool mask of the Y plane."""
    return _warp_nv12(frames, maps, siting, return_inside, 6)


def warp_perspective_nv12(frames, maps, siting: str = "left", return_inside: bool = False):
    """warp_perspective for NV12 frames, as warp_affine_nv12 under one 3 x 3 map each."""
    return _warp_nv12(frames, maps, siting, return_inside, 9)


def lucas_kanade_pyramidal_sequence_stabilize_nv12(frames, max_corners: int, detect_every: int, model: str = "similarity",
                                                   radius: int = 15, sigma=None, hypotheses: int = 256, threshold: float = 1.0,
                                                   seed: int = 0, quality_level: float = 0.01, min_distance: float = 10.0,
                                                   num_levels: int = 3, window_size: int = 5, num_iterations: int = 3,
                                                   alpha: float = 0.01, beta: float = 0.5, max_residual: float = 4.0,
                                                   refine_iterations: int = 0, refine_levels: int = 3,
                                                   siting: str = "left", refine_robust_delta=None) -> SequenceStabilized:
    """lucas_kanade_pyramidal_sequence_stabilize for NV12 video, frames (T, 3H/2, W) uint8 (nv12_from_planes): the motion is
    tracked, fitted and (with refine_iterations) refined on the Y planes, exactly as that call does on them, and the NV12
    frames are warped under the maps of that trajectory by warp_affine_nv12, the chroma sited as `siting` says.  .frames has
    the input's shape.  No conversion and no luma pass: the Y plane is the frame's first H W bytes.  refine_robust_delta (needs
    refine_iterations > 0) is sequence_refine_alignment's robust_delta, as in that call."""
    refine = _oflk.check_refine(refine_iterations, False, refine_robust_delta)
    code_siting = _oflk.check_nv12_siting(siting)
    arr = _oflk.as_nv12(frames, "(T, 3H/2, W)")
    T, R, W = arr.shape
    H = 2 * R // 3
    if T < 2:
        raise ValueError(f"a sequence needs at least 2 frames, got {T}")
    video = _Video(lambda: (arr, H, W), _oflk.FrameLayout("_nv12", (code_siting,)), lambda: np.ascontiguousarray(arr[:, :H, :]),
                   lambda grey, maps: warp_affine_nv12(arr, maps, siting))
    return _sequence_stabilize(video, max_corners, detect_every, model, radius, sigma, hypotheses, threshold, seed, quality_level,
                               min_distance, num_levels, window_size, num_iterations, alpha, beta, max_residual, refine, refine_levels,
                               False, refine_robust_delta)


class Mosaic(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_mosaic."""
    canvas: np.ndarray      # (Hc, Wc) -- (Hc, Wc, C) for colour --, the input's type: the blended frames in the anchor's coordinates
    count: np.ndarray       # (Hc, Wc) int32: the number of frames that cover each pixel
    origin: tuple           # (x0, y0): the anchor coordinates of canvas pixel (0, 0)
    to_anchor: np.ndarray   # (T, 3, 3) float64: frame t's coordinates to the anchor's (MosaicChain.to_anchor)
    held: np.ndarray        # (T-1,) bool: the step counted as no motion
    dropped: np.ndarray     # (T,) bool: the frame was left out
    model: np.ndarray       # (T-1, 3, 3) float32: the fitted homography of step t -> t+1; NaN where status is 0
    status: np.ndarray      # (T-1,) int32: 1 where a model was found


class PhotometricMosaic(NamedTuple):
    """Result of lucas_kanade_pyramidal_sequence_mosaic with refine_photometric=True: Mosaic's fields, then the exposure."""
    canvas: np.ndarray
    count: np.ndarray
    origin: tuple
    to_anchor: np.ndarray
    held: np.ndarray
    dropped: np.ndarray
    model: np.ndarray
    status: np.ndarray
    exposure: np.ndarray    # (T, 2) float64 (eg, eb): frame t's values entered the blend as eg[t] v + eb[t], the anchor's exposure


def lucas_kanade_pyramidal_sequence_mosaic(frames, max_corners: int = 1000, detect_every: int = 4, hypotheses: int = 256,
                                           threshold: float = 1.0, seed: int = 0, quality_level: float = 0.01,
                                           min_distance: float = 10.0, num_levels: int = 3, window_size: int = 5,
                                           num_iterations: int = 3, alpha: float = 0.01, beta: float = 0.5, max_residual: float = 4.0,
                                           anchor: int = 0, extent=None, blend: str = "feather", max_pixels=None,
                                           refine_iterations: int = 0, refine_levels: int = 3, order: str = "rgb",
                                           refine_photometric: bool = False, refine_robust_delta=None):
    """Frames in, one picture out: lucas_kanade_pyramidal_sequence_klt_sparse_replenish on the frames, tracks_homography on its
    rows, mosaic_chain from frame `anchor`, and mosaic_composite of every frame that is not dropped, in one call whose
    intermediate rows stay in the library.  The frames go up twice, chunk by chunk (once to track, once to blend).  The canvas
    is as large as the camera's path makes it; a canvas of more than max_pixels (default 16 H W) pixels raises OflkError with
    the size it needed in the message.

    refine_iterations > 0: the same chain made of its public parts, with sequence_refine_alignment (kind "homography",
    refine_levels levels, refine_iterations iterations each) between the fit and the chain, which answers the chain's drift: a
    product of steps fitted to at most max_corners tracks each.

    refine_photometric=True (needs refine_iterations > 0), for video whose exposure changes: every step is refined together
    with a gain and a bias (sequence_refine_alignment(..., photometric=True)), exposure_chain composes them from the anchor
    (a step that was not refined counts as no change), and every frame enters the blend at the anchor's exposure
    (mosaic_composite(..., exposure=...)).  Returns a PhotometricMosaic: Mosaic's fields and .exposure.  A uint8 canvas is
    rounded half to even and saturated to [0, 255]: a highlight that the anchor's exposure takes above 255 reads 255.

    refine_robust_delta (grey levels, e.g. 4.0; needs refine_iterations > 0) is sequence_refine_alignment's robust_delta, with
    or without refine_photometric: Huber weights, so that an object moving through the shot does not pull the refined steps.
    The blend itself is not masked by the weights.

    A 4-D uint8 array (T, H, W, C), C = 3 or 4, is interleaved colour video (`order`: "rgb" or "bgr"): this call runs on
    rgb_to_luma of the frames for everything but the canvas, and every channel's plane is then blended by mosaic_composite
    under the chain fitted on the luma; .canvas is (Hc, Wc, C), .count the grey call's."""
    refine = _oflk.check_refine(refine_iterations, refine_photometric, refine_robust_delta)
    _oflk.check_colour_order(order)
    if _oflk.is_packed(frames):
        packed = _oflk.as_packed(frames, "(T, H, W, C)")
        m = lucas_kanade_pyramidal_sequence_mosaic(rgb_to_luma(packed, order), max_corners, detect_every, hypotheses, threshold, seed,
                                                   quality_level, min_distance, num_levels, window_size, num_iterations, alpha, beta,
                                                   max_residual, anchor, extent, blend, max_pixels, refine_iterations, refine_levels,
                                                   refine_photometric=refine_photometric, refine_robust_delta=refine_robust_delta)
        ch = mosaic_chain(m.model, m.status, packed.shape[1:3], anchor, extent)
        canvas = mosaic_composite(packed, ch.from_anchor, m.canvas.shape, m.origin, ch.dropped, blend,
                                  exposure=m.exposure if refine_photometric else None)
        return m._replace(canvas=canvas)
    if refine > 0:
        rows = lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, max_corners, detect_every, quality_level, min_distance,
                                                                    num_levels, window_size, num_iterations, alpha, beta, max_residual)
        fit = tracks_homography(rows.tracks, rows.visible, rows.born, hypotheses, threshold, seed)
        arr, _ = _oflk.as_sequence(frames)
        al = sequence_refine_alignment(arr, fit.model, fit.status, "homography", refine_levels, refine,
                                       photometric=bool(refine_photometric), robust_delta=refine_robust_delta)
        ch = mosaic_chain(al.model, fit.status, arr.shape[1:], anchor, extent)
        Hc, Wc = ch.canvas_shape
        cap = _max_pixels(max_pixels, arr.shape[1], arr.shape[2])
        if Hc * Wc > cap:
            raise _oflk.OflkError(_oflk.OFLK_ERR_UNSUPPORTED,
                                  f"the canvas of {Wc} x {Hc} pixels at {ch.origin} exceeds the capacity of {cap} pixels")
        ex = exposure_chain(al.gain, al.bias, al.status == 1, anchor) if refine_photometric else None
        canvas, cnt = mosaic_composite(arr, ch.from_anchor, (Hc, Wc), ch.origin, ch.dropped, blend, True, exposure=ex)
        m = Mosaic(canvas, cnt, ch.origin, ch.to_anchor, ch.held, ch.dropped, al.model, fit.status)
        return PhotometricMosaic(*m, ex) if refine_photometric else m
    _oflk.check_fb_params(alpha, beta)
    arr, _ = _oflk.as_sequence(frames)
    T, H, W = arr.shape
    if H < 2 or W < 2:
        raise ValueError(f"frames must be at least 2 x 2, got {H} x {W}")
    trk = _oflk.check_tracking((H, W), num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level,
                               min_distance, detect_every)
    ransac = _oflk.check_ransac_params(hypotheses, threshold, seed)
    code = _oflk.check_mosaic_blend(blend)
    anchor = _oflk.check_int("anchor", anchor, 0, T - 1)
    extent = 8.0 * max(H, W) if extent is None else float(extent)
    if not (np.isfinite(extent) and extent > 0):
        raise ValueError(f"extent must be finite and > 0, got {extent!r}")
    cap = min(_max_pixels(max_pixels, H, W), 2 ** 30 - 1)
    out, cnt = np.empty(cap, arr.dtype), np.empty(cap, np.int32)
    canvas = np.zeros(4, np.int32)
    to, mod = np.empty((T, 9), np.float64), np.empty((T - 1, 9), np.float32)
    counts, held, drop = np.empty((T - 1, 3), np.int32), np.empty(T - 1, np.uint8), np.empty(T, np.uint8)
    src, fn = _oflk.pixels(arr, "oflk_mosaic_sequence")
    _oflk.check(fn(src, T, H, W, *trk, *ransac, anchor, extent, code, _oflk.pix(out), cap, canvas.ctypes.data_as(_oflk._i32p),
                   cnt.ctypes.data_as(_oflk._i32p), _oflk._f64(to), held.ctypes.data, drop.ctypes.data, _oflk.ptr(mod),
                   counts.ctypes.data_as(_oflk._i32p)))
    x0, y0, Wc, Hc = (int(v) for v in canvas)
    return Mosaic(out[:Hc * Wc].reshape(Hc, Wc).copy(), cnt[:Hc * Wc].reshape(Hc, Wc).copy(), (x0, y0), to.reshape(T, 3, 3),
                  held.astype(bool), drop.astype(bool), mod.reshape(T - 1, 3, 3), counts[:, 2].copy())


def lucas_kanade_pyramidal_sequence_mosaic_median(frames, max_corners: int = 1000, detect_every: int = 4, hypotheses: int = 256,
                                                  threshold: float = 1.0, seed: int = 0, quality_level: float = 0.01,
                                                  min_distance: float = 10.0, num_levels: int = 3, window_size: int = 5,
                                                  num_iterations: int = 3, alpha: float = 0.01, beta: float = 0.5,
                                                  max_residual: float = 4.0, anchor: int = 0, extent=None, max_pixels=None,
                                                  refine_iterations: int = 0, refine_levels: int = 3, order: str = "rgb",
                                                  refine_photometric: bool = False, refine_robust_delta=None):
    """lucas_kanade_pyramidal_sequence_mosaic with the temporal median for a blend: the clean plate of a panning shot, without
    the objects that move through it.  Made of the public parts and equal to their chain byte for byte:
    lucas_kanade_pyramidal_sequence_klt_sparse_replenish, tracks_homography, sequence_refine_alignment when refine_iterations >
    0, mosaic_chain from frame `anchor`, exposure_chain when refine_photometric, and mosaic_median of every frame that is not
    dropped.  The parameters are that call's without `blend`; a canvas of more than max_pixels (default 16 H W) pixels raises
    OflkError.  All frames are on the device at once for the median.  Returns a Mosaic, or a PhotometricMosaic with
    refine_photometric=True.

    A 4-D uint8 array (T, H, W, C), C = 3 or 4, is interleaved colour video: rgb_to_luma of the frames carries everything but
    the canvas, and every channel's plane then goes through mosaic_median under the chain fitted on the luma (a per-channel
    median); .canvas is (Hc, Wc, C)."""
    refine = _oflk.check_refine(refine_iterations, refine_photometric, refine_robust_delta)
    _oflk.check_colour_order(order)
    packed = _oflk.as_packed(frames, "(T, H, W, C)") if _oflk.is_packed(frames) else None
    arr, _ = _oflk.as_sequence(frames if packed is None else rgb_to_luma(packed, order))
    T, H, W = arr.shape
    if H < 2 or W < 2:
        raise ValueError(f"frames must be at least 2 x 2, got {H} x {W}")
    # what the parts below refuse, before the first of them runs
    _oflk.check_fb_params(alpha, beta)
    _oflk.check_tracking((H, W), num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level,
                         min_distance, detect_every)
    _oflk.check_ransac_params(hypotheses, threshold, seed)
    anchor = _oflk.check_int("anchor", anchor, 0, T - 1)
    if extent is not None and not (np.isfinite(float(extent)) and float(extent) > 0):
        raise ValueError(f"extent must be finite and > 0, got {extent!r}")
    cap = _max_pixels(max_pixels, H, W)
    rows = lucas_kanade_pyramidal_sequence_klt_sparse_replenish(arr, max_corners, detect_every, quality_level, min_distance, num_levels,
                                                                window_size, num_iterations, alpha, beta, max_residual)
    fit = tracks_homography(rows.tracks, rows.visible, rows.born, hypotheses, threshold, seed)
    model, al = fit.model, None
    if refine > 0:
        al = sequence_refine_alignment(arr, fit.model, fit.status, "homography", refine_levels, refine,
                                       photometric=bool(refine_photometric), robust_delta=refine_robust_delta)
        model = al.model
    ch = mosaic_chain(model, fit.status, (H, W), anchor, extent)
    Hc, Wc = ch.canvas_shape
    if Hc * Wc > cap:
        raise _oflk.OflkError(_oflk.OFLK_ERR_UNSUPPORTED,
                              f"the canvas of {Wc} x {Hc} pixels at {ch.origin} exceeds the capacity of {cap} pixels")
    ex = exposure_chain(al.gain, al.bias, al.status == 1, anchor) if refine_photometric else None
    canvas, cnt = mosaic_median(arr if packed is None else packed, ch.from_anchor, (Hc, Wc), ch.origin, ch.dropped, True, ex)
    m = Mosaic(canvas, cnt, ch.origin, ch.to_anchor, ch.held, ch.dropped, model, fit.status)
    return PhotometricMosaic(*m, ex) if refine_photometric else m


def _max_pixels(max_pixels, H: int, W: int) -> int:
    """the mosaic's canvas capacity: max_pixels, by default 16 H W"""
    return _oflk.check_int("max_pixels", 16 * H * W if max_pixels is None else max_pixels, 1)


class TrackerRow(NamedTuple):
    """One frame's row of a SparseKltTracker: K slots."""
    xy: np.ndarray         # (K, 2) float32 (x, y); NaN where not visible
    visible: np.ndarray    # (K,) bool
    born: np.ndarray       # (K,) bool: a new track began in this slot on this frame
    birth: np.ndarray      # (K,) int32: the frame on which the slot's current track began (meaningful where visible)
    residual: np.ndarray   # (K,) float32: the forward residual of the step into this frame of a slot alive before it; else NaN
    detected: int          # points accepted by this frame's detection


class SparseKltTracker:
    """lucas_kanade_pyramidal_sequence_klt_sparse_replenish for video that arrives frame by frame: the state stays on the
    device and push(frame) returns that frame's row (with motion=, also that step's global motion: motion()).  Frame t detects when t % detect_every == 0 (0: never; hand it points
    with add_points), at once, so a point born on frame t is in row t.  The rows of T pushes are rows 0 .. T-1 of the
    sequence call on those frames followed by any one more.

        with SparseKltTracker(frame.shape, 1000) as tracker:
            for frame in video:                     # uint8 (H, W)
                row = tracker.push(frame)
    """

    def __init__(self, shape, max_corners: int, detect_every: int = 4, quality_level: float = 0.01, min_distance: float = 10.0,
                 num_levels: int = 3, window_size: int = 5, num_iterations: int = 3, alpha: float = 0.01, beta: float = 0.5,
                 max_residual: float = 4.0, dtype=np.uint8, device: int = 0, motion=None):
        if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
            raise ValueError(f"shape must be (H, W), got {shape!r}")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise ValueError(f"dtype must be uint8 or float32, got {dtype!r}")
        H, W = int(shape[0]), int(shape[1])
        trk = _oflk.check_tracking((H, W), num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners,
                                   quality_level, min_distance, detect_every, min_every=0)
        self.shape, self.max_corners, self.detect_every = (H, W), trk.max_corners, trk.detect_every
        self._t = _oflk.Tracker(device, H, W, self.dtype == np.uint8, **trk._asdict())
        if motion is not None:
            self.set_motion(**motion) if isinstance(motion, dict) else self.set_motion(motion)

    @staticmethod
    def _row(r) -> TrackerRow:
        return TrackerRow(r[0], r[1].astype(bool), r[2].astype(bool), r[3], r[4], r[5])

    def push(self, frame) -> TrackerRow:
        """the next frame (H, W) in, its row out (synchronous)"""
        f = np.ascontiguousarray(frame, self.dtype)
        if f.shape != self.shape:
            raise ValueError(f"expected a frame of shape {self.shape}, got {f.shape}")
        return self._row(self._t.push(f))

    def push_device(self, ptr: int, stream: int = 0) -> None:
        """the next frame at a device address, asynchronous on `stream`; read_row or row_device gives its row"""
        self._t.push_device(ptr, stream)

    def read_row(self, stream: int = 0) -> TrackerRow:
        """the row of the last pushed frame, points of add_points included (synchronises `stream`)"""
        return self._row(self._t.read_row(stream))

    def row_device(self):
        """device addresses (xy, visible, born, birth, residual, detected) of the last pushed frame's row, valid until the
        next push, add_points or reset"""
        return self._t.row_device()

    def add_points(self, pts, stream: int = 0) -> None:
        """(n, 2) points (x, y) start tracks on the last pushed frame in the dead slots, ascending; points outside the frame
        or not finite, and those for which no dead slot is left, are dropped"""
        self._t.add_points(pts, stream)

    def reset(self) -> None:
        """every slot dead; the next push is frame 0"""
        self._t.reset()

    def set_motion(self, model="similarity", hypotheses: int = 256, threshold: float = 1.0, seed: int = 0) -> None:
        """From the next push on, every push also fits the global motion of its step (lucas_kanade_core.estimate_motion on
        the slots visible on both frames and not born on the new one, hash index t-1 for the push of frame t) on the
        device; motion() returns it.  model None turns it off.  The constructor's motion= takes a model name or a dict of
        these arguments."""
        if model is None:
            self._t.set_motion(-1)
        else:
            self._t.set_motion(*_oflk.check_motion_params(model, hypotheses, threshold, seed))

    def motion(self, stream: int = 0) -> Motion:
        """the last push's Motion: rows t-1 -> t; status 0 after frame 0 (synchronises `stream`)"""
        m, inl, cnt = self._t.read_motion(stream)
        return Motion(m.reshape(2, 3), inl.astype(bool), int(cnt[0]), int(cnt[1]), int(cnt[2]))

    def motion_device(self):
        """device addresses (model [6], inlier [K], counts [3]) of the last push's motion, valid until the next push"""
        return self._t.motion_device()

    @property
    def frame_index(self) -> int:
        """index of the last pushed frame, -1 before the first"""
        return self._t.frame_index

    def close(self) -> None:
        self._t.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class StabilizedFrame(NamedTuple):
    """One steadied frame of an OnlineStabilizer."""
    index: int                     # the frame's index in the stream
    frame: np.ndarray              # (H, W) -- (H, W, C) for colour --, the input's type; zero where the source lies outside
    correction: np.ndarray         # (2, 3) float32: where the frame's content was moved to
    inside: Optional[np.ndarray]   # (H, W) bool: the source lay inside the frame; None unless asked for


class OnlineStabilizer:
    """lucas_kanade_pyramidal_sequence_stabilize for video that arrives frame by frame: a SparseKltTracker with its motion on,
    a delay line of radius + 1 frames and the last 2 radius step models stay on the device.  The window of frame f reaches
    radius frames ahead, so push(frame t) returns frame t - radius (None while t < radius) and flush() returns the last
    radius frames once the stream has ended.  The frames and corrections of T pushes and a flush are those of the sequence
    call on the same T frames, byte for byte.  After flush() the stabiliser takes no frame until reset().  The black border
    is not cropped (inside=True returns the mask).  shape = (H, W, C) with C = 3 or 4 and order = "rgb" or "bgr" (required:
    without it a three-entry shape is refused, as it always was) makes a colour stabiliser: it takes and returns interleaved
    uint8 frames (H, W, C), tracks their luma, which the push forms on the device, and equals the sequence call on the same
    colour frames; the device forms then take [H][W][C] frames too.  layout = "nv12" with shape = (H, W), H and W even, makes
    an NV12 stabiliser: it takes and returns (3H/2, W) uint8 frames (nv12_from_planes), tracks their Y plane where it lies,
    warps both planes in one launch with the chroma sited as `siting` says ("left" or "center"), and equals
    lucas_kanade_pyramidal_sequence_stabilize_nv12 on the same frames; inside stays (H, W).  An NV12 frame is never guessed
    from a shape.

        with OnlineStabilizer(frame.shape, 1000, radius=15) as stab:
            for frame in video:                     # uint8 (H, W)
                s = stab.push(frame)
                if s is not None:
                    show(s.index, s.frame)
            for s in stab.flush():
                show(s.index, s.frame)
    """

    def __init__(self, shape, max_corners: int, detect_every: int = 4, model="similarity", radius: int = 15, sigma=None,
                 hypotheses: int = 256, threshold: float = 1.0, seed: int = 0, quality_level: float = 0.01,
                 min_distance: float = 10.0, num_levels: int = 3, window_size: int = 5, num_iterations: int = 3, alpha: float = 0.01,
                 beta: float = 0.5, max_residual: float = 4.0, dtype=np.uint8, device: int = 0, inside: bool = False,
                 order: Optional[str] = None, layout: Optional[str] = None, siting: str = "left"):
        if layout is not None and layout != "nv12":
            raise ValueError(f"layout must be None or 'nv12', got {layout!r}")
        nv12 = layout == "nv12"
        code_siting = _oflk.check_nv12_siting(siting)
        if nv12 and (len(shape) != 2 or int(shape[0]) < 4 or int(shape[1]) < 4 or int(shape[0]) % 2 or int(shape[1]) % 2):
            raise ValueError(f"an NV12 stabiliser needs shape (H, W) with H, W even and >= 4, got {shape!r}")
        if nv12 and order is not None:
            raise ValueError("NV12 frames have no channel order")
        if len(shape) not in (2, 3) or int(shape[0]) < 2 or int(shape[1]) < 2:
            raise ValueError(f"shape must be (H, W) or (H, W, C) with H, W >= 2, got {shape!r}")
        channels = 0
        if len(shape) == 3:   # interleaved colour frames: the tracker sees their luma
            channels = int(shape[2])
            if channels not in (3, 4):
                raise ValueError(f"colour frames must have 3 or 4 interleaved channels, got shape {shape!r}")
            if order is None:   # a decoder hands over RGB or BGR: there is no safe guess, and (H, W, 3) was refused before colour
                raise ValueError(f"a colour stabiliser (shape {shape!r}) needs order='rgb' or order='bgr'")
        code_order = 0 if order is None else _oflk.check_colour_order(order)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise ValueError(f"dtype must be uint8 or float32, got {dtype!r}")
        if channels and self.dtype != np.dtype(np.uint8):
            raise ValueError("colour frames must be uint8 (float32 colour is not offered)")
        if nv12 and self.dtype != np.dtype(np.uint8):
            raise ValueError("NV12 frames must be uint8")
        H, W = int(shape[0]), int(shape[1])
        trk = _oflk.check_tracking((H, W), num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners,
                                   quality_level, min_distance, detect_every, min_every=0)
        fit = _oflk.check_motion_params(model, hypotheses, threshold, seed)
        win = _oflk.check_window(radius, sigma)
        self.max_corners, self.detect_every, self.radius, self.inside = trk.max_corners, trk.detect_every, win.radius, bool(inside)
        self._s = _oflk.Stabilizer(device, H, W, self.dtype == np.uint8, **trk._asdict(), **fit._asdict(), weights=win.weights,
                                   channels=channels, order=code_order, nv12=nv12, siting=code_siting)
        self.shape = self._s.layout.frame_shape(H, W)

    def _frame(self, index, frame, corr, ins) -> StabilizedFrame:
        return StabilizedFrame(int(index), frame, corr.reshape(2, 3), None if ins is None else ins.astype(bool))

    def push(self, frame) -> Optional[StabilizedFrame]:
        """the next frame (H, W) -- (H, W, C) for a colour stabiliser, (3H/2, W) for an NV12 one -- in; frame t - radius
        steadied, or None while t < radius (synchronous)"""
        f = np.ascontiguousarray(frame, self.dtype)
        if f.shape != self.shape:
            raise ValueError(f"expected a frame of shape {self.shape}, got {f.shape}")
        e, out, corr, ins = self._s.push(f, self.inside)
        return None if e < 0 else self._frame(e, out, corr, ins)

    def flush(self) -> List[StabilizedFrame]:
        """the stream has ended: the min(radius, T) frames not yet returned, ascending (synchronous)"""
        first, out, corr, ins = self._s.flush(self.inside)
        return [self._frame(first + i, out[i], corr[i], None if ins is None else ins[i]) for i in range(len(out))]

    def push_device(self, ptr: int, out_ptr: int, inside_ptr: int = 0, stream: int = 0) -> int:
        """the next frame at a device address, asynchronous on `stream`: returns the index of the frame written to out_ptr
        [H][W] (and inside_ptr [H][W] uint8), or -1 when nothing was written"""
        return self._s.push_device(ptr, out_ptr, inside_ptr, stream)

    def flush_device(self, out_ptr: int, inside_ptr: int = 0, stream: int = 0) -> Tuple[int, int]:
        """the stream has ended: (first, count) of the frames written to out_ptr [radius][H][W] (and inside_ptr)"""
        return self._s.flush_device(out_ptr, inside_ptr, stream)

    def correction_device(self) -> Tuple[int, int]:
        """device addresses (correction [rows][6] float32, map [rows][6] float64) of the last emission, valid until the next
        push, flush or reset"""
        return self._s.correction_device()

    def row(self, stream: int = 0) -> TrackerRow:
        """the tracker's row of the last pushed frame (not of the returned one; synchronises `stream`)"""
        return SparseKltTracker._row(self._s.tracker.read_row(stream))

    def motion(self, stream: int = 0) -> Motion:
        """the fitted motion of the step into the last pushed frame; status 0 after frame 0 (synchronises `stream`)"""
        m, inl, cnt = self._s.tracker.read_motion(stream)
        return Motion(m.reshape(2, 3), inl.astype(bool), int(cnt[0]), int(cnt[1]), int(cnt[2]))

    def add_points(self, pts, stream: int = 0) -> None:
        """SparseKltTracker.add_points on the last pushed frame"""
        self._s.tracker.add_points(pts, stream)

    @property
    def lag(self) -> int:
        """frames between a push and the frame it returns: the radius"""
        return self._s.lag

    @property
    def frame_index(self) -> int:
        """index of the last pushed frame, -1 before the first"""
        return self._s.frame_index

    def reset(self) -> None:
        """forget the stream: the next push is frame 0"""
        self._s.reset()

    def close(self) -> None:
        self._s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _dump_levels(key, shapes, u, v) -> None:
    """The reference's per-level PNG side effect (:226), after the call, best-effort."""
    num_levels = key[3]
    out_dir = os.environ.get("OFLK_DUMP_DIR", "python/output")
    try:
        for level in range(num_levels):
            if level == num_levels - 1:
                lu, lv = u, v
            else:
                lu = np.empty(shapes[level], np.float32)
                lv = np.empty(shapes[level], np.float32)
                _oflk.check(_oflk.lib().oflk_pyramidal_last_level_flow(*key, level, 0, _oflk.ptr(lu), _oflk.ptr(lv)))
            visualize_pyramid_level(lu, lv, level, num_levels, out_dir)
    except ImportError:
        pass  # no matplotlib on this box


# ---------------------------------------------------------------------------
# host-side plotting and CLI (names kept for drop-in use; not GPU work)
# ---------------------------------------------------------------------------
def _quiver_panel(ax, u, v, title: str, step: int, scale: float) -> None:
    h, w = u.shape
    ys, xs = np.mgrid[step:h:step, step:w:step]
    us, vs = u[step:h:step, step:w:step], v[step:h:step, step:w:step]
    ax.quiver(xs, ys, us, vs, np.hypot(us, vs), angles="xy", scale_units="xy",
              scale=1.0 / scale, cmap="jet", width=0.003)
    ax.set_aspect("equal")
    ax.set_xlim(0, w)
    ax.set_ylim(h, 0)
    ax.set_title(title)
    ax.set_xlabel("X (pixels)")
    ax.set_ylabel("Y (pixels)")


def visualize_flow_comparison(flow_u_single, flow_v_single, flow_u_pyr, flow_v_pyr,
                              output_path: Path, scale: float = 1.0) -> None:
    """Side-by-side quiver plots, single-scale vs pyramidal (reference :231-310)."""
    import matplotlib

    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt

    fig, axes = plt.subplots(1, 2, figsize=(20, 9))
    _quiver_panel(axes[0], flow_u_single, flow_v_single, "Single-Scale Lucas-Kanade", 10, scale)
    _quiver_panel(axes[1], flow_u_pyr, flow_v_pyr, "Pyramidal Lucas-Kanade", 10, scale)
    fig.tight_layout()
    fig.savefig(output_path, dpi=100)
    plt.close(fig)
    print(f"Comparison visualization saved: {output_path}")


def visualize_pyramid_level(flow_u, flow_v, level: int, num_levels: int = 3,
                            output_dir: str = "python/output") -> None:
    """U / V / magnitude images of one level's flow (reference :313-351)."""
    import matplotlib

    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    from matplotlib.colors import Normalize

    os.makedirs(output_dir, exist_ok=True)
    panels = [
        (flow_u, "RdBu_r", Normalize(vmin=-20, vmax=20), f"Level {level}: U (horizontal)"),
        (flow_v, "RdBu_r", Normalize(vmin=-20, vmax=20), f"Level {level}: V (vertical)"),
        (np.sqrt(flow_u**2 + flow_v**2), "viridis", Normalize(vmin=0, vmax=20), f"Level {level}: Magnitude"),
    ]
    fig, axes = plt.subplots(1, 3, figsize=(15, 4))
    for ax, (img, cmap, norm, title) in zip(axes, panels):
        im = ax.imshow(img, cmap=cmap, norm=norm)
        ax.set_title(title)
        ax.axis("off")
        fig.colorbar(im, ax=ax, label="pixels")
    fig.tight_layout()
    fig.savefig(f"{output_dir}/pyramid_level_{level}.png", dpi=100, bbox_inches="tight")
    plt.close(fig)


def _load_pair(frame_dir: Path, height: int, width: int):
    prev = np.fromfile(frame_dir / "frame_00.bin", dtype=np.uint8).reshape(height, width)
    curr = np.fromfile(frame_dir / "frame_01.bin", dtype=np.uint8).reshape(height, width)
    return prev.astype(np.float32), curr.astype(np.float32)


def main() -> None:
    """CLI with the reference's options (reference :354-475)."""
    ap = argparse.ArgumentParser(description="Pyramidal Lucas-Kanade optical flow (MI355X)")
    ap.add_argument("--frame-dir", type=str, default=str(DEFAULT_FRAME_DIR),
                    help="Directory containing frame_00.bin and frame_01.bin")
    ap.add_argument("--width", type=int, default=320, help="Frame width")
    ap.add_argument("--height", type=int, default=240, help="Frame height")
    ap.add_argument("--num-levels", type=int, default=3, help="Number of pyramid levels")
    ap.add_argument("--window-size", type=int, default=5, help="Window size")
    ap.add_argument("--num-iterations", type=int, default=3, help="Iterations per pyramid level")
    ap.add_argument("--output-dir", type=str, default="python/output", help="Output directory")
    ap.add_argument("--compare", action="store_true", help="Compare with single-scale implementation")
    args = ap.parse_args()

    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    frame_prev, frame_curr = _load_pair(Path(args.frame_dir), args.height, args.width)

    bar = "=" * 60
    print(bar + "\nPyramidal Lucas-Kanade Optical Flow\n" + bar)
    print(f"Loaded frames: {args.width}x{args.height}")
    print(f"Pyramid levels: {args.num_levels}")
    print(f"Window size: {args.window_size}x{args.window_size}")
    print(f"Iterations per level: {args.num_iterations}")
    print("\n" + bar + "\nRunning Pyramidal Lucas-Kanade...\n" + bar)
    u_pyr, v_pyr = lucas_kanade_pyramidal(frame_prev, frame_curr, num_levels=args.num_levels,
                                          window_size=args.window_size,
                                          num_iterations=args.num_iterations)

    region = np.s_[105:135, 55:85]
    u_mean, v_mean = np.mean(u_pyr[region]), np.mean(v_pyr[region])
    print("\n" + bar + "\nPyramidal Results\n" + bar)
    print(f"Mean flow in test region: u={u_mean:.3f}, v={v_mean:.3f}")
    print(f"Std dev in test region:   u={np.std(u_pyr[region]):.3f}, v={np.std(v_pyr[region]):.3f}")
    u_pyr.tofile(out_dir / "flow_u_pyramidal.bin")
    v_pyr.tofile(out_dir / "flow_v_pyramidal.bin")
    print(f"\nPyramidal flow fields saved to {out_dir}")

    if args.compare:
        print("\n" + bar + "\nRunning Single-Scale for Comparison...\n" + bar)
        u_s, v_s = lucas_kanade_single_scale(frame_prev, frame_curr, window_size=args.window_size)
        us_mean, vs_mean = np.mean(u_s[region]), np.mean(v_s[region])
        print("\n" + bar + "\nComparison\n" + bar)
        print(f"Single-scale: u={us_mean:.3f}, v={vs_mean:.3f}")
        print(f"Pyramidal:    u={u_mean:.3f}, v={v_mean:.3f}")
        print(f"Difference:   u={abs(u_mean - us_mean):.3f}, v={abs(v_mean - vs_mean):.3f}")
        try:
            visualize_flow_comparison(u_s, v_s, u_pyr, v_pyr, out_dir / "flow_comparison.png")
        except ImportError:
            print("Matplotlib not available, skipping visualization")
    print("\n" + bar + "\nComplete!\n" + bar)


if __name__ == "__main__":
    main()
