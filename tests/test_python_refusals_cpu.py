"""The refusals of the Python tier above the C ABI -- every public entry point of lucas_kanade_pyramidal and lucas_kanade_core
that takes tracking, fit, trajectory-window, refine or alignment settings -- and which refusal wins when two arguments are
wrong.  The counterpart of tests/test_config_refusals_cpu.py one tier up.

Every row is refused before the call's first library call; the library is replaced by the recording stub of
tests/test_python_marshalling_cpu.py all the same, so a fault that were accepted would show as "did not raise", with or
without a GPU.

CALLS gives each call with arguments that it accepts; FAULTS names a fault and the arguments it sets; ORDER lists, per call,
one fault per check in the order the checks are made, EXTRA further faults that are only tried alone.  EXPECTED pins the
exception type and the exact message of every fault alone (EXCEPT where a call words it differently); it was recorded from
the modules before their settings became records (`python tests/test_python_refusals_cpu.py` prints the tables of the
modules it imports).  Precedence: each fault of ORDER together with the next one that sets other arguments raises the
earlier fault's message, and so do the pairs of MORE_PAIRS.  ACCEPTED lists edge values that are normalised, not refused.

Raises that have no row, because they can only be reached after a library call: in the refined
lucas_kanade_pyramidal_sequence_mosaic (refine_iterations > 0) the max_pixels ValueError and the canvas-capacity OflkError,
both made after the tracking, fit and alignment calls; in the refined and the colour paths of
lucas_kanade_pyramidal_sequence_stabilize[_nv12] and _mosaic everything that tracks_motion / tracks_homography,
sequence_refine_alignment, stabilize_trajectory, mosaic_chain, exposure_chain, warp_affine[_nv12] and mosaic_composite refuse
(their own calls have the rows, the warps and composites in their grey, colour and NV12 forms); and the frame checks of the push
methods.  replenish_features has its rows because its integer check shares check_int."""
import numpy as np
import pytest

from test_python_marshalling_cpu import StubLib

T, H, W, K = 3, 24, 32, 4
GREY = {"f32": np.zeros((T, H, W), np.float32), "u8": np.zeros((T, H, W), np.uint8)}
COLOUR = np.zeros((T, H, W, 3), np.uint8)
NV12 = np.zeros((T, 3 * H // 2, W), np.uint8)
TRACKS, VISIBLE, BORN = np.zeros((T, K, 2), np.float32), np.ones((T, K), bool), np.zeros((T, K), bool)
WEIGHTS = np.array([1.0, 0.5, 0.25])

_KLT = dict(num_levels=2, window_size=5, num_iterations=3, alpha=0.01, beta=0.5)
_RES = dict(max_residual=4.0)
_SEL = dict(max_corners=K, quality_level=0.01, min_distance=3.0)
_FIT = dict(hypotheses=64, threshold=1.5, seed=7)
_WIN = dict(radius=2, sigma=None)
_REF = dict(refine_iterations=0, refine_levels=2, refine_photometric=False, refine_robust_delta=None)
_STAB = dict(**_SEL, detect_every=2, model="similarity", **_WIN, **_FIT, **_KLT, **_RES)
_MOS = dict(**_SEL, detect_every=2, **_FIT, **_KLT, **_RES, anchor=1, extent=None, blend="feather", max_pixels=None, order="rgb", **_REF)
_ALIGN = dict(model=np.zeros((T, 9), np.float32), status=None, kind="homography", levels=2, iterations=2, min_share=0.25,
              photometric=False, robust_delta=None)


def _p():
    import lucas_kanade_pyramidal
    return lucas_kanade_pyramidal


def _c():
    import lucas_kanade_core
    return lucas_kanade_core


def _set_motion(**kw):
    _p().SparseKltTracker((H, W), K).set_motion(**kw)


def _raw_stabilizer(**kw):
    import _oflk
    _oflk.Stabilizer(**kw)


def _both(name, make):
    return {f"{name}-{px}": make(f) for px, f in GREY.items()}


# call -> (the function, arguments that it accepts)
CALLS = {
    **_both("klt", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_klt(**kw), dict(frames=f, **_SEL, **_KLT))),
    **_both("klt_replenish", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_klt_replenish(**kw),
                                        dict(frames=f, **_SEL, detect_every=2, **_KLT))),
    **_both("sparse_tracks", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_sparse_tracks(**kw),
                                        dict(frames=f, queries=np.float32([[0, 5, 6]]), **_KLT, **_RES))),
    **_both("klt_sparse", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_klt_sparse(**kw),
                                     dict(frames=f, **_SEL, **_KLT, **_RES))),
    **_both("klt_sparse_replenish", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_klt_sparse_replenish(**kw),
                                               dict(frames=f, **_SEL, detect_every=2, **_KLT, **_RES))),
    **_both("stabilize", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_stabilize(**kw),
                                    dict(frames=f, **_STAB, order="rgb", **_REF))),
    "stabilize-colour": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_stabilize(**kw), dict(frames=COLOUR, **_STAB, order="rgb", **_REF)),
    "stabilize-refine-u8": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_stabilize(**kw),
                            dict(frames=GREY["u8"], **_STAB, order="rgb", **{**_REF, "refine_iterations": 2})),
    "stabilize-refine-colour": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_stabilize(**kw),
                                dict(frames=COLOUR, **_STAB, order="rgb", **{**_REF, "refine_iterations": 2})),
    "stabilize_nv12": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_stabilize_nv12(**kw),
                       dict(frames=NV12, **_STAB, refine_iterations=0, refine_levels=2, siting="left", refine_robust_delta=None)),
    "stabilize_nv12-refine": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_stabilize_nv12(**kw),
                              dict(frames=NV12, **_STAB, refine_iterations=2, refine_levels=2, siting="left", refine_robust_delta=None)),
    **_both("mosaic", lambda f: (lambda **kw: _p().lucas_kanade_pyramidal_sequence_mosaic(**kw), dict(frames=f, **_MOS))),
    "mosaic-colour": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_mosaic(**kw), dict(frames=COLOUR, **_MOS)),
    "mosaic-refine-u8": (lambda **kw: _p().lucas_kanade_pyramidal_sequence_mosaic(**kw),
                         dict(frames=GREY["u8"], **{**_MOS, "refine_iterations": 2})),
    **_both("sparse", lambda f: (lambda **kw: _p().lucas_kanade_sparse(**kw),
                                 dict(frame_prev=f[0], frame_curr=f[1], points=np.float32([[5, 6]]), num_levels=2, window_size=5,
                                      num_iterations=3))),
    "tracker": (lambda **kw: _p().SparseKltTracker(**kw), dict(shape=(H, W), **_SEL, detect_every=2, **_KLT, **_RES, dtype=np.uint8)),
    "set_motion": (_set_motion, dict(model="similarity", **_FIT)),
    "online": (lambda **kw: _p().OnlineStabilizer(**kw), dict(shape=(H, W), **_STAB, dtype=np.uint8, order=None, layout=None, siting="left")),
    "online-colour": (lambda **kw: _p().OnlineStabilizer(**kw),
                      dict(shape=(H, W, 3), **_STAB, dtype=np.uint8, order="rgb", layout=None, siting="left")),
    "online-nv12": (lambda **kw: _p().OnlineStabilizer(**kw),
                    dict(shape=(H, W), **_STAB, dtype=np.uint8, order=None, layout="nv12", siting="left")),
    "_oflk.Stabilizer": (_raw_stabilizer, dict(device=0, H=H, W=W, u8=True, max_corners=K, detect_every=2, model=1, weights=WEIGHTS,
                                               channels=0, nv12=False)),
    "tracks_motion": (lambda **kw: _c().tracks_motion(**kw), dict(tracks=TRACKS, visible=VISIBLE, born=BORN, model="similarity", **_FIT, t0=0)),
    "estimate_motion": (lambda **kw: _c().estimate_motion(**kw),
                        dict(src=TRACKS[0], dst=TRACKS[1], valid=VISIBLE[0], model="similarity", **_FIT, step0=0)),
    "tracks_homography": (lambda **kw: _c().tracks_homography(**kw), dict(tracks=TRACKS, visible=VISIBLE, born=BORN, **_FIT, t0=0)),
    "estimate_homography": (lambda **kw: _c().estimate_homography(**kw), dict(src=TRACKS[0], dst=TRACKS[1], valid=VISIBLE[0], **_FIT, step0=0)),
    "stabilize_trajectory": (lambda **kw: _c().stabilize_trajectory(**kw),
                             dict(models=np.zeros((T - 1, 6), np.float32), status=np.ones(T - 1, np.int32), **_WIN)),
    **_both("refine_alignment", lambda f: (lambda **kw: _c().refine_alignment(**kw), dict(a=f, b=f, **_ALIGN))),
    **_both("sequence_refine_alignment", lambda f: (lambda **kw: _c().sequence_refine_alignment(**kw),
                                                    dict(frames=f, **{**_ALIGN, "model": np.zeros((T - 1, 9), np.float32)}))),
    **_both("alignment_weights", lambda f: (lambda **kw: _c().alignment_weights(**kw),
                                            dict(a=f, b=f, model=np.zeros((T, 9), np.float32), kind="homography", robust_delta=4.0,
                                                 gain=None, bias=None))),
    "warp_affine-grey": (lambda **kw: _c().warp_affine(**kw), dict(frames=GREY["u8"], maps=np.zeros((T, 2, 3)), return_inside=False)),
    "warp_affine-colour": (lambda **kw: _c().warp_affine(**kw), dict(frames=COLOUR, maps=np.zeros((T, 2, 3)), return_inside=False)),
    "warp_affine-nv12": (lambda **kw: _p().warp_affine_nv12(**kw), dict(frames=NV12, maps=np.zeros((T, 2, 3)), siting="left")),
    "warp_perspective-grey": (lambda **kw: _c().warp_perspective(**kw), dict(frames=GREY["u8"], maps=np.zeros((T, 3, 3)), return_inside=True)),
    "warp_perspective-colour": (lambda **kw: _c().warp_perspective(**kw), dict(frames=COLOUR, maps=np.zeros((T, 3, 3)), return_inside=True)),
    "warp_perspective-nv12": (lambda **kw: _p().warp_perspective_nv12(**kw), dict(frames=NV12, maps=np.zeros((T, 3, 3)), siting="left")),
    "mosaic_composite-grey": (lambda **kw: _c().mosaic_composite(**kw),
                              dict(frames=GREY["u8"], maps=np.zeros((T, 3, 3)), canvas_shape=(8, 8), origin=(0, 0), skip=None, blend="mean",
                                   return_count=False, exposure=None)),
    "mosaic_composite-colour": (lambda **kw: _c().mosaic_composite(**kw),
                                dict(frames=COLOUR, maps=np.zeros((T, 3, 3)), canvas_shape=(8, 8), origin=(0, 0), skip=None, blend="mean",
                                     return_count=False, exposure=None)),
    "mosaic_chain": (lambda **kw: _c().mosaic_chain(**kw),
                     dict(model=np.zeros((T - 1, 9), np.float32), status=np.ones(T - 1, np.int32), shape=(H, W), anchor=1, extent=None)),
    "exposure_chain": (lambda **kw: _c().exposure_chain(**kw),
                       dict(gain=np.ones(T - 1, np.float32), bias=np.zeros(T - 1, np.float32), status=np.ones(T - 1, np.int32), anchor=1)),
    "replenish_features": (lambda **kw: _c().replenish_features(**kw),
                           dict(frame=GREY["u8"][0], xy=np.zeros((K, 2), np.float32), visible=np.zeros(K, bool), max_corners=K,
                                quality_level=0.01, min_distance=3.0, window_size=5, t=0, qt=None, qxy=None)),
}

# fault -> the arguments it sets
FAULTS = {
    "alpha=-1": {"alpha": -1.0}, "beta=inf": {"beta": np.inf}, "alpha=1e40": {"alpha": 1e40},
    "max_corners=0": {"max_corners": 0}, "max_corners=True": {"max_corners": True}, "max_corners=1.5": {"max_corners": 1.5},
    "quality_level=2": {"quality_level": 2.0}, "quality_level=nan": {"quality_level": np.nan},
    "min_distance=-1": {"min_distance": -1.0}, "min_distance=inf": {"min_distance": np.inf},
    "window_size=4": {"window_size": 4}, "window_size=13": {"window_size": 13},
    "num_levels=0": {"num_levels": 0}, "num_levels=True": {"num_levels": True}, "num_levels=5": {"num_levels": 5},
    "num_iterations=0": {"num_iterations": 0}, "num_iterations=1.5": {"num_iterations": 1.5},
    "max_residual=nan": {"max_residual": np.nan}, "max_residual=-1": {"max_residual": -1.0},
    "detect_every=0": {"detect_every": 0}, "detect_every=-1": {"detect_every": -1}, "detect_every=True": {"detect_every": True},
    "detect_every=1.5": {"detect_every": 1.5},
    "T=1": {"frames": np.zeros((1, H, W), np.uint8)}, "frames 2-D": {"frames": np.zeros((H, W), np.uint8)},
    "frames empty": {"frames": np.zeros((T, 0, W), np.uint8)}, "frames item 3-D": {"frames": [np.zeros((1, H, W)), np.zeros((1, H, W))]},
    "frames mixed shapes": {"frames": [np.zeros((H, W)), np.zeros((H, W + 1))]},
    "frames mixed dtypes": {"frames": [np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)]},
    "frames H=1": {"frames": np.zeros((T, 1, W), np.uint8)},
    "colour float32": {"frames": np.zeros((T, H, W, 3), np.float32)}, "colour C=5": {"frames": np.zeros((T, H, W, 5), np.uint8)},
    "colour H=1": {"frames": np.zeros((T, 1, W, 3), np.uint8)}, "colour T=1": {"frames": np.zeros((1, H, W, 3), np.uint8)},
    "nv12 4-D": {"frames": np.zeros((T, 36, W, 1), np.uint8)}, "nv12 float32": {"frames": np.zeros((T, 36, W), np.float32)},
    "nv12 rows=35": {"frames": np.zeros((T, 35, W), np.uint8)}, "nv12 W=31": {"frames": np.zeros((T, 36, 31), np.uint8)},
    "nv12 tiny": {"frames": np.zeros((T, 3, W), np.uint8)}, "nv12 T=1": {"frames": np.zeros((1, 36, W), np.uint8)},
    "queries 1-D": {"queries": np.zeros(3, np.float32)}, "queries t=9": {"queries": np.float32([[9, 5, 6]])},
    "queries t=0.5": {"queries": np.float32([[0.5, 5, 6]])},
    "refine_iterations=-1": {"refine_iterations": -1}, "refine_iterations=True": {"refine_iterations": True},
    "refine_iterations=1.5": {"refine_iterations": 1.5}, "refine_photometric alone": {"refine_photometric": True},
    "refine_robust_delta alone": {"refine_robust_delta": 4.0},
    "order=xyz": {"order": "xyz"}, "order=0": {"order": 0}, "order=None": {"order": None}, "order=rgb": {"order": "rgb"},
    "siting=x": {"siting": "x"},
    "model=x": {"model": "x"}, "model=7": {"model": 7}, "model=True": {"model": True},
    "hypotheses=0": {"hypotheses": 0}, "hypotheses=65537": {"hypotheses": 65537}, "hypotheses=True": {"hypotheses": True},
    "threshold=nan": {"threshold": np.nan}, "threshold=0": {"threshold": 0.0},
    "seed=-1": {"seed": -1}, "seed=2^32": {"seed": 2 ** 32}, "seed=1.5": {"seed": 1.5},
    "radius=-1": {"radius": -1}, "radius=65": {"radius": 65}, "radius=True": {"radius": True},
    "sigma=0": {"sigma": 0.0}, "sigma=nan": {"sigma": np.nan}, "sigma=0.01": {"sigma": 0.01},
    "blend=x": {"blend": "x"}, "anchor=3": {"anchor": 3}, "anchor=-1": {"anchor": -1}, "anchor=True": {"anchor": True},
    "extent=0": {"extent": 0.0}, "extent=nan": {"extent": np.nan},
    "max_pixels=0": {"max_pixels": 0}, "max_pixels=True": {"max_pixels": True}, "max_pixels=1.5": {"max_pixels": 1.5},
    "prev 3-D": {"frame_prev": np.zeros((1, H, W), np.float32)}, "curr other shape": {"frame_curr": np.zeros((H, W + 1), np.float32)},
    "points 1-D": {"points": np.zeros(2, np.float32)}, "points empty": {"points": np.zeros((0, 2), np.float32)},
    "shape 1-D": {"shape": (H,)}, "shape H=0": {"shape": (0, W)}, "shape H=1": {"shape": (1, W)}, "shape 4-D": {"shape": (H, W, 3, 1)},
    "shape 3-D": {"shape": (H, W, 3)}, "channels=5": {"shape": (H, W, 5)}, "shape H=25": {"shape": (25, W)}, "shape H=2": {"shape": (2, W)},
    "dtype=int16": {"dtype": np.int16}, "dtype=float32": {"dtype": np.float32},
    "layout=x": {"layout": "x"},
    "nv12 float": {"nv12": True, "u8": False}, "nv12 channels": {"nv12": True, "channels": 3}, "channels float": {"channels": 3, "u8": False},
    "tracks 2-D": {"tracks": np.zeros((T, K), np.float32)}, "tracks T=1": {"tracks": np.zeros((1, K, 2), np.float32)},
    "visible other shape": {"visible": np.ones((T, K + 1), bool)}, "born other shape": {"born": np.zeros((T, K + 1), bool)},
    "t0=-1": {"t0": -1}, "t0=True": {"t0": True}, "step0=-1": {"step0": -1}, "step0=2^31": {"step0": 2 ** 31},
    "dst other shape": {"dst": np.zeros((K + 1, 2), np.float32)}, "src 1-D": {"src": np.zeros(2, np.float32)},
    "valid other shape": {"valid": np.ones(K + 1, bool)},
    "models (2, 5)": {"models": np.zeros((T - 1, 5), np.float32)}, "status other shape": {"status": np.ones(T + 3, np.int32)},
    "kind=x": {"kind": "x"}, "kind=0": {"kind": 0},
    "levels=0": {"levels": 0}, "levels=True": {"levels": True}, "iterations=0": {"iterations": 0}, "iterations=1.5": {"iterations": 1.5},
    "min_share=0": {"min_share": 0.0}, "min_share=2": {"min_share": 2.0}, "min_share=nan": {"min_share": np.nan},
    "robust_delta=0": {"robust_delta": 0.0}, "robust_delta=nan": {"robust_delta": np.nan}, "robust_delta=x": {"robust_delta": "4"},
    "robust_delta=True": {"robust_delta": True}, "robust_delta=1e40": {"robust_delta": 1e40}, "robust_delta=None": {"robust_delta": None},
    "a 4-D": {"a": np.zeros((1, T, H, W), np.float32)}, "a empty": {"a": np.zeros((T, 0, W), np.float32)},
    "b other shape": {"b": np.zeros((T, H, W + 1), np.float32)},
    "frames 4-D": {"frames": np.zeros((1, T, H, W), np.float32)}, "align T=1": {"frames": np.zeros((1, H, W), np.float32)},
    "model size": {"model": np.zeros((T, 5), np.float32)},
    "maps (T, 5)": {"maps": np.zeros((T, 5))}, "maps (T, 2, 3)": {"maps": np.zeros((T, 2, 3))}, "maps (9, 3)": {"maps": np.zeros((9, 3))},
    "maps 4-D": {"maps": np.zeros((1, T, 3, 3))},
    "canvas_shape 1-D": {"canvas_shape": (8,)}, "canvas_shape Hc=0": {"canvas_shape": (0, 8)}, "canvas 2^30": {"canvas_shape": (2 ** 15, 2 ** 15)},
    "origin=True": {"origin": (True, 0)}, "origin 1-D": {"origin": (0,)}, "origin=2^31": {"origin": (0, 2 ** 31)},
    "skip other shape": {"skip": np.zeros(T + 1, bool)}, "exposure other shape": {"exposure": np.zeros((T, 3))},
    "model (2, 5)": {"model": np.zeros((T - 1, 5), np.float32)}, "bias other shape": {"bias": np.zeros(T, np.float32)},
    "frame 3-D": {"frame": np.zeros((1, H, W), np.uint8)}, "xy 1-D": {"xy": np.zeros(K, np.float32)},
    "visible other length": {"visible": np.zeros(K + 1, bool)}, "max_corners=5": {"max_corners": K + 1},
    "t=-1": {"t": -1}, "t=True": {"t": True}, "t=1.5": {"t": 1.5},
    "qt other shape": {"qt": np.zeros(K + 1, np.int32)}, "qxy other shape": {"qxy": np.zeros((K, 3), np.float32)},
    "gain alone": {"gain": 1.0}, "gain shape": {"gain": np.ones(T + 1, np.float32), "bias": np.zeros(T + 1, np.float32)},
}

# the checks in the order they are made, one fault each
_FB = ["alpha=-1"]
_SELECT = ["max_corners=0", "quality_level=2", "min_distance=-1"]
_SPARSE = ["num_levels=0", "num_iterations=0", "window_size=4", "num_levels=5"]
_SPARSE_R = _SPARSE + ["max_residual=nan"]
_TRACKING = _FB + ["T=1"] + _SPARSE_R + _SELECT
_RANSAC = ["hypotheses=0", "threshold=nan", "seed=-1"]
_MOTION = ["model=x"] + _RANSAC
_WINDOW = ["radius=-1", "sigma=0"]
_REFINE = ["refine_iterations=-1", "refine_photometric alone", "refine_robust_delta alone"]
_ALIGN_O = ["kind=x", "levels=0", "iterations=0", "min_share=0", "robust_delta=0"]
_X_FB = ["beta=inf", "alpha=1e40"]
_X_SELECT = ["max_corners=True", "max_corners=1.5", "quality_level=nan", "min_distance=inf"]
_X_SPARSE = ["num_levels=True", "num_iterations=1.5", "window_size=13"]
_X_SEQ = ["frames 2-D", "frames empty", "frames item 3-D", "frames mixed shapes", "frames mixed dtypes"]
_X_EVERY = ["detect_every=True", "detect_every=1.5", "detect_every=-1"]
_X_RANSAC = ["hypotheses=65537", "hypotheses=True", "threshold=0", "seed=2^32", "seed=1.5"]
_X_MOTION = ["model=7", "model=True"] + _X_RANSAC
_X_WINDOW = ["radius=65", "radius=True", "sigma=nan", "sigma=0.01"]
_X_REFINE = ["refine_iterations=True", "refine_iterations=1.5"]
_X_TRACKING = _X_FB + _X_SELECT + _X_SPARSE + ["max_residual=-1"]
_X_ALIGN = ["kind=0", "levels=True", "iterations=1.5", "min_share=2", "min_share=nan", "robust_delta=nan", "robust_delta=x",
            "robust_delta=True", "robust_delta=1e40"]
_X_NV12 = ["nv12 4-D", "nv12 float32", "nv12 W=31", "nv12 tiny"]
_X_PACKED = ["colour float32", "colour H=1"]

ORDER = {
    "klt": _FB + _SELECT + ["window_size=4", "T=1"],
    "klt_replenish": _FB + _SELECT + ["window_size=4", "detect_every=0", "T=1"],
    "sparse_tracks": _FB + ["T=1"] + _SPARSE_R + ["queries 1-D"],
    "klt_sparse": _TRACKING,
    "klt_sparse_replenish": _TRACKING + ["detect_every=0"],
    "stabilize": _REFINE + ["order=xyz"] + _TRACKING + ["detect_every=0"] + _MOTION + _WINDOW,
    "stabilize-colour": _REFINE + ["order=xyz", "colour C=5", "alpha=-1", "colour T=1"] + _SPARSE_R + _SELECT + ["detect_every=0"] + _MOTION + _WINDOW,
    "stabilize-refine-u8": ["order=xyz"] + _TRACKING + ["detect_every=0"],
    "stabilize-refine-colour": ["order=xyz", "colour C=5"],
    "stabilize_nv12": ["refine_iterations=-1", "refine_robust_delta alone", "siting=x", "nv12 rows=35", "alpha=-1"] + _SPARSE_R + _SELECT
                      + ["detect_every=0"] + _MOTION + _WINDOW,
    "stabilize_nv12-refine": ["siting=x", "nv12 rows=35", "alpha=-1"] + _SPARSE_R + _SELECT + ["detect_every=0"],
    "mosaic": _REFINE + ["order=xyz"] + _TRACKING + ["detect_every=0"] + _RANSAC + ["blend=x", "anchor=3", "extent=0", "max_pixels=0"],
    "mosaic-colour": _REFINE + ["order=xyz", "colour C=5"],
    "mosaic-refine-u8": ["order=xyz"] + _TRACKING + ["detect_every=0"],
    "sparse": ["prev 3-D", "curr other shape"] + _SPARSE + ["points 1-D"],
    "tracker": ["shape 1-D", "dtype=int16", "alpha=-1"] + _SPARSE_R + _SELECT + ["detect_every=-1"],
    "set_motion": _MOTION,
    "online": ["layout=x", "siting=x", "shape 1-D", "order=xyz", "dtype=int16", "alpha=-1"] + _SPARSE_R + _SELECT + ["detect_every=-1"]
              + _MOTION + _WINDOW,
    "online-colour": ["layout=x", "siting=x", "channels=5", "order=xyz", "dtype=float32", "alpha=-1"] + _SPARSE_R + _SELECT
                     + ["detect_every=-1"] + _MOTION + _WINDOW,
    "online-nv12": ["siting=x", "shape H=25", "order=rgb", "dtype=float32", "alpha=-1"] + _SPARSE_R + _SELECT + ["detect_every=-1"]
                   + _MOTION + _WINDOW,
    "_oflk.Stabilizer": [],
    "tracks_motion": ["tracks 2-D", "born other shape"] + _MOTION + ["t0=-1"],
    "estimate_motion": _MOTION + ["dst other shape", "valid other shape", "step0=-1"],
    "tracks_homography": ["tracks 2-D", "born other shape"] + _RANSAC + ["t0=-1"],
    "estimate_homography": _RANSAC + ["dst other shape", "valid other shape", "step0=-1"],
    "stabilize_trajectory": _WINDOW + ["models (2, 5)", "status other shape"],
    "refine_alignment": _ALIGN_O + ["a 4-D", "b other shape", "model size", "status other shape"],
    "sequence_refine_alignment": _ALIGN_O + ["frames 4-D", "model size", "status other shape"],
    "alignment_weights": ["kind=x", "robust_delta=0", "a 4-D", "b other shape", "model size", "gain alone"],
    "warp_affine-grey": ["frames H=1", "maps (T, 5)"],
    "warp_affine-colour": ["colour C=5", "maps (T, 5)"],
    "warp_affine-nv12": ["siting=x", "nv12 rows=35", "maps (T, 5)"],
    "warp_perspective-grey": ["frames H=1", "maps (T, 5)"],
    "warp_perspective-colour": ["colour C=5", "maps (T, 5)"],
    "warp_perspective-nv12": ["siting=x", "nv12 rows=35", "maps (T, 5)"],
    "mosaic_composite-grey": ["frames H=1", "blend=x", "canvas_shape 1-D", "origin=True", "maps (T, 5)", "skip other shape",
                              "exposure other shape"],
    "mosaic_composite-colour": ["colour C=5", "blend=x", "canvas_shape 1-D", "origin=True", "maps (T, 5)", "skip other shape",
                                "exposure other shape"],
    "mosaic_chain": ["shape 1-D", "model (2, 5)", "anchor=3", "extent=0", "status other shape"],
    "exposure_chain": ["bias other shape", "anchor=3", "status other shape"],
    "replenish_features": ["frame 3-D", "xy 1-D", "max_corners=5", "quality_level=2", "min_distance=-1", "window_size=4", "t=-1",
                           "qt other shape"],
}
EXTRA = {
    "klt": _X_FB + _X_SELECT + ["window_size=13"] + _X_SEQ,
    "klt_replenish": _X_FB + _X_SELECT + _X_EVERY + _X_SEQ,
    "sparse_tracks": _X_FB + _X_SPARSE + ["max_residual=-1", "queries t=9", "queries t=0.5"] + _X_SEQ,
    "klt_sparse": _X_TRACKING + _X_SEQ,
    "klt_sparse_replenish": _X_TRACKING + _X_EVERY + _X_SEQ,
    "stabilize": _X_REFINE + ["order=0"] + _X_TRACKING + _X_EVERY + _X_MOTION + _X_WINDOW + _X_SEQ,
    "stabilize-colour": _X_REFINE + _X_PACKED + _X_TRACKING + _X_EVERY + _X_MOTION + _X_WINDOW,
    "stabilize-refine-u8": _X_TRACKING + _X_EVERY + _X_SEQ,
    "stabilize-refine-colour": _X_PACKED,
    "stabilize_nv12": _X_REFINE + _X_NV12 + ["nv12 T=1"] + _X_TRACKING + _X_EVERY + _X_MOTION + _X_WINDOW,
    "stabilize_nv12-refine": _X_NV12 + ["nv12 T=1"] + _X_TRACKING + _X_EVERY,
    "mosaic": _X_REFINE + _X_TRACKING + _X_EVERY + _X_RANSAC + ["frames H=1", "anchor=-1", "anchor=True", "extent=nan", "max_pixels=True",
                                                                "max_pixels=1.5"] + _X_SEQ,
    "mosaic-colour": _X_REFINE + _X_PACKED,
    "mosaic-refine-u8": _X_TRACKING + _X_EVERY + _X_SEQ,
    "sparse": _X_SPARSE + ["points empty"],
    "tracker": ["shape H=0", "shape 3-D"] + _X_TRACKING + ["detect_every=True", "detect_every=1.5"],
    "set_motion": _X_MOTION,
    "online": ["shape H=1", "shape 4-D", "shape 3-D"] + _X_TRACKING + ["detect_every=True", "detect_every=1.5"] + _X_MOTION + _X_WINDOW,
    "online-colour": ["order=None", "dtype=int16", "shape H=1"] + _X_TRACKING + _X_MOTION + _X_WINDOW,
    "online-nv12": ["layout=x", "shape H=2", "shape 3-D", "dtype=int16"] + _X_TRACKING + _X_MOTION + _X_WINDOW,
    "_oflk.Stabilizer": ["nv12 float", "nv12 channels", "channels float"],
    "tracks_motion": ["tracks T=1", "visible other shape", "t0=True"] + _X_MOTION,
    "estimate_motion": ["src 1-D", "step0=2^31"] + _X_MOTION,
    "tracks_homography": ["tracks T=1", "visible other shape", "t0=True"] + _X_RANSAC,
    "estimate_homography": ["src 1-D", "step0=2^31"] + _X_RANSAC,
    "stabilize_trajectory": _X_WINDOW,
    "refine_alignment": _X_ALIGN + ["a empty"],
    "sequence_refine_alignment": _X_ALIGN + ["align T=1", "frames empty"],
    "alignment_weights": ["kind=0", "robust_delta=nan", "robust_delta=x", "robust_delta=True", "robust_delta=None", "gain shape"],
    "warp_affine-grey": ["maps (9, 3)", "maps 4-D", "frames empty"],
    "warp_affine-colour": ["colour float32", "colour H=1", "maps (9, 3)"],
    "warp_affine-nv12": _X_NV12 + ["maps (9, 3)"],
    "warp_perspective-grey": ["maps (T, 2, 3)", "maps (9, 3)", "maps 4-D", "frames empty"],
    "warp_perspective-colour": ["colour float32", "colour H=1", "maps (T, 2, 3)", "maps (9, 3)"],
    "warp_perspective-nv12": _X_NV12 + ["maps (T, 2, 3)", "maps (9, 3)"],
    "mosaic_composite-grey": ["frames empty", "canvas_shape Hc=0", "canvas 2^30", "origin 1-D", "origin=2^31", "maps (T, 2, 3)", "maps (9, 3)"],
    "mosaic_composite-colour": ["colour float32", "colour H=1", "canvas 2^30", "origin=2^31", "maps (9, 3)"],
    "mosaic_chain": ["shape H=1", "anchor=-1", "anchor=True", "extent=nan"],
    "exposure_chain": ["anchor=-1", "anchor=True"],
    "replenish_features": ["visible other length", "max_corners=True", "max_corners=0", "quality_level=nan", "min_distance=inf",
                           "window_size=13", "t=True", "t=1.5", "qxy other shape"],
}

# pairs that are not neighbours in ORDER: (call, the fault that wins, the other)
MORE_PAIRS = [
    ("mosaic", "frames H=1", "num_levels=0"), ("mosaic", "alpha=-1", "max_pixels=0"), ("mosaic", "refine_iterations=-1", "order=xyz"),
    ("stabilize", "refine_iterations=-1", "order=xyz"), ("stabilize", "alpha=-1", "radius=-1"), ("stabilize", "num_levels=0", "detect_every=0"),
    ("stabilize-colour", "order=xyz", "alpha=-1"), ("stabilize-colour", "colour C=5", "alpha=-1"), ("stabilize-colour", "alpha=-1", "num_levels=0"),
    ("stabilize_nv12", "refine_iterations=-1", "siting=x"), ("stabilize_nv12", "nv12 T=1", "alpha=-1"), ("stabilize_nv12", "nv12 T=1", "num_levels=0"),
    ("klt", "max_corners=0", "T=1"), ("klt_replenish", "detect_every=0", "T=1"), ("klt_sparse", "T=1", "max_corners=0"),
    ("klt_sparse_replenish", "max_residual=nan", "detect_every=0"), ("tracker", "dtype=int16", "max_corners=0"),
    ("online", "layout=x", "radius=-1"), ("online-colour", "order=None", "dtype=float32"), ("online-nv12", "shape H=25", "dtype=float32"),
    ("refine_alignment", "kind=x", "status other shape"), ("refine_alignment", "robust_delta=x", "a 4-D"),
    ("alignment_weights", "model size", "gain shape"),
    ("mosaic_composite-grey", "canvas 2^30", "origin=True"), ("mosaic_chain", "anchor=3", "status other shape"),
    ("replenish_features", "max_corners=5", "t=-1"), ("warp_perspective-grey", "frames H=1", "maps (9, 3)"),
]

# accepted edge values, normalised rather than refused (what goes to the library: tests/test_python_marshalling_cpu.py)
ACCEPTED = [
    ("klt_replenish", {"detect_every": 2 ** 40}), ("klt_sparse_replenish", {"detect_every": 2 ** 40}), ("stabilize", {"detect_every": 2 ** 40}),
    ("stabilize-colour", {"detect_every": 2 ** 40}), ("stabilize_nv12", {"detect_every": 2 ** 40}), ("mosaic", {"detect_every": 2 ** 40}),
    ("tracker", {"detect_every": 2 ** 40}), ("online", {"detect_every": 2 ** 40}), ("tracker", {"detect_every": 0}), ("online", {"detect_every": 0}),
    ("klt_sparse_replenish", {"detect_every": np.int64(2), "max_corners": np.int64(K), "num_levels": 2.0, "num_iterations": np.int64(3)}),
    ("stabilize", {"detect_every": 2.0, "radius": np.int64(2), "hypotheses": 64.0, "seed": np.int64(7), "refine_iterations": 0.0}),
    ("mosaic", {"anchor": np.int64(1), "max_pixels": 4096.0, "refine_iterations": np.int64(0)}),
    ("refine_alignment", {"levels": 2.0, "iterations": np.int64(2), "robust_delta": np.float32(4.0)}),
    ("refine_alignment", {"robust_delta": 4}), ("set_motion", {"model": None}), ("set_motion", {"model": 2}),
    ("klt_sparse", {"max_residual": np.inf}), ("stabilize", {"refine_iterations": 2, "refine_photometric": True, "refine_robust_delta": 4.0}),
]

MESSAGES = [   # (exception type's name, message); EXPECTED's and EXCEPT's values are indices into this list
    ('ValueError', 'alpha and beta must be finite and >= 0, got -1.0, 0.5'),   # 0
    ('ValueError', 'max_corners must be an integer >= 1, got 0'),
    ('ValueError', 'quality_level must be in [0, 1], got 2.0'),
    ('ValueError', 'min_distance must be finite and >= 0, got -1.0'),
    ('ValueError', 'window_size must be one of (3, 5, 7, 9, 11), got 4'),
    ('ValueError', 'a sequence needs at least 2 frames, got 1'),   # 5
    ('ValueError', 'alpha and beta must be finite and >= 0, got 0.01, inf'),
    ('ValueError', 'alpha and beta must be finite and >= 0, got 1e+40, 0.5'),
    ('ValueError', 'max_corners must be an integer >= 1, got True'),
    ('ValueError', 'max_corners must be an integer >= 1, got 1.5'),
    ('ValueError', 'quality_level must be in [0, 1], got nan'),   # 10
    ('ValueError', 'min_distance must be finite and >= 0, got inf'),
    ('ValueError', 'window_size must be one of (3, 5, 7, 9, 11), got 13'),
    ('ValueError', 'expected a (T, H, W) array of frames, got shape (24, 32)'),
    ('ValueError', 'empty frames: shape (3, 0, 32)'),
    ('ValueError', 'every frame must be a 2-D array, got shape (1, 24, 32)'),   # 15
    ('ValueError', 'frames of mixed shapes: [(24, 32), (24, 33)]'),
    ('ValueError', "frames of mixed dtypes: ['float32', 'uint8']"),
    ('ValueError', 'detect_every must be an integer >= 1, got 0'),
    ('ValueError', 'detect_every must be an integer >= 1, got True'),
    ('ValueError', 'detect_every must be an integer >= 1, got 1.5'),   # 20
    ('ValueError', 'detect_every must be an integer >= 1, got -1'),
    ('ValueError', 'num_levels must be an integer >= 1, got 0'),
    ('ValueError', 'num_iterations must be an integer >= 1, got 0'),
    ('ValueError', 'pyramid level 0 of 24 x 32 frames would be 1 x 2: the sparse tracker needs 2 x 2'),
    ('ValueError', 'max_residual must be >= 0 (inf: no residual test), got nan'),   # 25
    ('ValueError', 'queries must be an (N, 3) (t, x, y) or (N, 2) (x, y) array with N >= 1, got shape (3,)'),
    ('ValueError', 'num_levels must be an integer >= 1, got True'),
    ('ValueError', 'num_iterations must be an integer >= 1, got 1.5'),
    ('ValueError', 'max_residual must be >= 0 (inf: no residual test), got -1.0'),
    ('ValueError', 'query frames must be integers in [0, 2]'),   # 30
    ('ValueError', 'refine_iterations must be an integer >= 0, got -1'),
    ('ValueError', 'refine_photometric needs refine_iterations > 0'),
    ('ValueError', 'refine_robust_delta needs refine_iterations > 0'),
    ('ValueError', "order must be one of ['bgr', 'rgb'], got 'xyz'"),
    ('ValueError', "model must be one of ['affine', 'similarity', 'translation'], got 'x'"),   # 35
    ('ValueError', 'hypotheses must be an integer in [1, 65536], got 0'),
    ('ValueError', 'threshold must be finite and > 0, got nan'),
    ('ValueError', 'seed must be an integer in [0, 2^32), got -1'),
    ('ValueError', 'radius must be an integer in [0, 64], got -1'),
    ('ValueError', 'sigma must be finite and > 0, got 0.0'),   # 40
    ('ValueError', 'refine_iterations must be an integer >= 0, got True'),
    ('ValueError', 'refine_iterations must be an integer >= 0, got 1.5'),
    ('ValueError', "order must be one of ['bgr', 'rgb'], got 0"),
    ('ValueError', "model must be one of ['affine', 'similarity', 'translation'], got 7"),
    ('ValueError', "model must be one of ['affine', 'similarity', 'translation'], got True"),   # 45
    ('ValueError', 'hypotheses must be an integer in [1, 65536], got 65537'),
    ('ValueError', 'hypotheses must be an integer in [1, 65536], got True'),
    ('ValueError', 'threshold must be finite and > 0, got 0.0'),
    ('ValueError', 'seed must be an integer in [0, 2^32), got 4294967296'),
    ('ValueError', 'seed must be an integer in [0, 2^32), got 1.5'),   # 50
    ('ValueError', 'radius must be an integer in [0, 64], got 65'),
    ('ValueError', 'radius must be an integer in [0, 64], got True'),
    ('ValueError', 'sigma must be finite and > 0, got nan'),
    ('ValueError', 'sigma 0.01 is too small for radius 2: a weight underflows to 0'),
    ('ValueError', 'colour frames must have 3 or 4 interleaved channels, got 5'),   # 55
    ('ValueError', 'colour frames must be uint8 (float32 colour is not offered), got float32'),
    ('ValueError', 'expected at least one frame of at least 2 x 2 pixels, got shape (3, 1, 32, 3)'),
    ('ValueError', "siting must be one of ['center', 'left'], got 'x'"),
    ('ValueError', 'an NV12 frame has 3H/2 rows with H even, got 35 rows'),
    ('ValueError', 'expected a (T, 3H/2, W) array of NV12 frames, got shape (3, 36, 32, 1)'),   # 60
    ('ValueError', 'NV12 frames must be uint8, got float32'),
    ('ValueError', 'NV12 frames need an even W, got 31'),
    ('ValueError', 'expected at least one NV12 frame of at least 4 x 4 pixels, got shape (3, 3, 32)'),
    ('ValueError', "blend must be one of ['feather', 'first', 'last', 'mean'], got 'x'"),
    ('ValueError', 'anchor must be an integer in [0, 2], got 3'),   # 65
    ('ValueError', 'extent must be finite and > 0, got 0.0'),
    ('ValueError', 'max_pixels must be an integer >= 1, got 0'),
    ('ValueError', 'frames must be at least 2 x 2, got 1 x 32'),
    ('ValueError', 'anchor must be an integer in [0, 2], got -1'),
    ('ValueError', 'anchor must be an integer in [0, 2], got True'),   # 70
    ('ValueError', 'extent must be finite and > 0, got nan'),
    ('ValueError', 'max_pixels must be an integer >= 1, got True'),
    ('ValueError', 'max_pixels must be an integer >= 1, got 1.5'),
    ('ValueError', 'expected a 2-D array, got shape (1, 24, 32)'),
    ('ValueError', 'shape mismatch: (24, 32) vs (24, 33)'),   # 75
    ('ValueError', 'points must be an (N, 2) (x, y) array with N >= 1, got shape (2,)'),
    ('ValueError', 'points must be an (N, 2) (x, y) array with N >= 1, got shape (0, 2)'),
    ('ValueError', 'shape must be (H, W), got (24,)'),
    ('ValueError', "dtype must be uint8 or float32, got <class 'numpy.int16'>"),
    ('ValueError', 'detect_every must be an integer >= 0, got -1'),   # 80
    ('ValueError', 'shape must be (H, W), got (0, 32)'),
    ('ValueError', 'shape must be (H, W), got (24, 32, 3)'),
    ('ValueError', 'detect_every must be an integer >= 0, got True'),
    ('ValueError', 'detect_every must be an integer >= 0, got 1.5'),
    ('ValueError', "layout must be None or 'nv12', got 'x'"),   # 85
    ('ValueError', 'shape must be (H, W) or (H, W, C) with H, W >= 2, got (24,)'),
    ('ValueError', 'shape must be (H, W) or (H, W, C) with H, W >= 2, got (1, 32)'),
    ('ValueError', 'shape must be (H, W) or (H, W, C) with H, W >= 2, got (24, 32, 3, 1)'),
    ('ValueError', "a colour stabiliser (shape (24, 32, 3)) needs order='rgb' or order='bgr'"),
    ('ValueError', 'colour frames must have 3 or 4 interleaved channels, got shape (24, 32, 5)'),   # 90
    ('ValueError', 'colour frames must be uint8 (float32 colour is not offered)'),
    ('ValueError', 'an NV12 stabiliser needs shape (H, W) with H, W even and >= 4, got (25, 32)'),
    ('ValueError', 'NV12 frames have no channel order'),
    ('ValueError', 'NV12 frames must be uint8'),
    ('ValueError', 'an NV12 stabiliser needs shape (H, W) with H, W even and >= 4, got (2, 32)'),   # 95
    ('ValueError', 'an NV12 stabiliser needs shape (H, W) with H, W even and >= 4, got (24, 32, 3)'),
    ('ValueError', 'NV12 frames are uint8 and have no channel axis'),
    ('ValueError', 'expected tracks (T, K, 2) with T >= 2 and visible (T, K), got (3, 4) and (3, 4)'),
    ('ValueError', 'born must have shape (3, 4), got (3, 5)'),
    ('ValueError', 'step0 must be an integer in [0, 2^31), got -1'),   # 100
    ('ValueError', 'expected tracks (T, K, 2) with T >= 2 and visible (T, K), got (1, 4, 2) and (3, 4)'),
    ('ValueError', 'expected tracks (T, K, 2) with T >= 2 and visible (T, K), got (3, 4, 2) and (3, 5)'),
    ('ValueError', 'step0 must be an integer in [0, 2^31), got True'),
    ('ValueError', 'expected src and dst of one shape (N, 2) or (S, N, 2), got (4, 2) and (5, 2)'),
    ('ValueError', 'valid must have shape (4,), got (5,)'),   # 105
    ('ValueError', 'expected src and dst of one shape (N, 2) or (S, N, 2), got (2,) and (4, 2)'),
    ('ValueError', 'step0 must be an integer in [0, 2^31), got 2147483648'),
    ('ValueError', 'expected models of shape (T-1, 2, 3) or (T-1, 6), got (2, 5)'),
    ('ValueError', 'status must have shape (2,), got (6,)'),
    ('ValueError', "kind must be one of ['affine', 'homography'], got 'x'"),   # 110
    ('ValueError', 'levels must be an integer >= 1, got 0'),
    ('ValueError', 'iterations must be an integer >= 1, got 0'),
    ('ValueError', 'min_share must be in (0, 1], got 0.0'),
    ('ValueError', 'robust_delta must be finite and > 0 as float32, got 0.0'),
    ('ValueError', 'expected an (H, W) frame or an (F, H, W) batch, got shape (1, 3, 24, 32)'),   # 115
    ('ValueError', 'a and b must have one shape and type, got (3, 24, 32) float32 and (3, 24, 33) float32'),
    ('ValueError', 'expected 3 homography models of 9 coefficients, got (3, 5)'),
    ('ValueError', 'status must have shape (3,), got (6,)'),
    ('ValueError', "kind must be one of ['affine', 'homography'], got 0"),
    ('ValueError', 'levels must be an integer >= 1, got True'),   # 120
    ('ValueError', 'iterations must be an integer >= 1, got 1.5'),
    ('ValueError', 'min_share must be in (0, 1], got 2.0'),
    ('ValueError', 'min_share must be in (0, 1], got nan'),
    ('ValueError', 'robust_delta must be finite and > 0 as float32, got nan'),
    ('ValueError', "robust_delta must be a number, got '4'"),   # 125
    ('ValueError', 'robust_delta must be a number, got True'),
    ('ValueError', 'robust_delta must be finite and > 0 as float32, got 1e+40'),
    ('ValueError', 'no frames, or empty frames'),
    ('ValueError', 'a and b must have one shape and type, got (3, 24, 32) uint8 and (3, 24, 33) float32'),
    ('ValueError', 'expected 2 homography models of 9 coefficients, got (3, 5)'),   # 130
    ('ValueError', 'a sequence needs at least two frames, got 1'),
    ('ValueError', 'gain and bias go together'),
    ('ValueError', 'robust_delta must be a number, got None'),
    ('ValueError', 'gain and bias must be scalars or have shape (3,), got (4,) and (4,)'),
    ('ValueError', 'expected 3 maps of shape (2, 3) or (6,), got (3, 5)'),   # 135
    ('ValueError', 'expected 3 maps of shape (2, 3) or (6,), got (9, 3)'),
    ('ValueError', 'expected 3 maps of shape (2, 3) or (6,), got (1, 3, 3, 3)'),
    ('ValueError', 'expected a (F, 3H/2, W) or (3H/2, W) array of NV12 frames, got shape (3, 36, 32, 1)'),
    ('ValueError', 'expected 3 maps of shape (3, 3) or (9,), got (3, 5)'),
    ('ValueError', 'expected 3 maps of shape (3, 3) or (9,), got (3, 2, 3)'),   # 140
    ('ValueError', 'expected 3 maps of shape (3, 3) or (9,), got (9, 3)'),
    ('ValueError', 'expected 3 maps of shape (3, 3) or (9,), got (1, 3, 3, 3)'),
    ('ValueError', 'canvas_shape must be (Hc, Wc) with Hc, Wc >= 1, got (8,)'),
    ('ValueError', 'origin must be two integers (x0, y0), got (True, 0)'),
    ('ValueError', 'skip must have shape (3,), got (4,)'),   # 145
    ('ValueError', 'exposure must have shape (3, 2), got (3, 3)'),
    ('ValueError', 'canvas_shape must be (Hc, Wc) with Hc, Wc >= 1, got (0, 8)'),
    ('ValueError', 'a canvas of 2^30 pixels or more is not supported, got 32768 x 32768'),
    ('ValueError', 'origin must be two integers (x0, y0), got (0,)'),
    ('ValueError', 'origin must be two integers (x0, y0), got (0, 2147483648)'),   # 150
    ('ValueError', 'shape must be (H, W) with H, W >= 2, got (24,)'),
    ('ValueError', 'expected models of shape (T-1, 3, 3) or (T-1, 9), got (2, 5)'),
    ('ValueError', 'shape must be (H, W) with H, W >= 2, got (1, 32)'),
    ('ValueError', 'gain and bias must have one shape, got (2,) and (3,)'),
    ('ValueError', 'expected one (H, W) frame, got shape (1, 24, 32)'),   # 155
    ('ValueError', 'expected xy (K, 2) and visible (K,), got (4,) and (4,)'),
    ('ValueError', 'max_corners 5 is not the number of slots 4'),
    ('ValueError', 't must be an integer >= 0, got -1'),
    ('ValueError', 'expected qt (4,) and qxy (4, 2), got (5,) and (4, 2)'),
    ('ValueError', 'expected xy (K, 2) and visible (K,), got (4, 2) and (5,)'),   # 160
    ('ValueError', 'max_corners True is not the number of slots 4'),
    ('ValueError', 'max_corners 0 is not the number of slots 4'),
    ('ValueError', 't must be an integer >= 0, got True'),
    ('ValueError', 't must be an integer >= 0, got 1.5'),
    ('ValueError', 'expected qt (4,) and qxy (4, 2), got (4,) and (4, 3)'),   # 165
]
EXPECTED = {   # fault -> message
    'alpha=-1': 0, 'beta=inf': 6, 'alpha=1e40': 7, 'max_corners=0': 1, 'max_corners=True': 8, 'max_corners=1.5': 9,
    'quality_level=2': 2, 'quality_level=nan': 10, 'min_distance=-1': 3, 'min_distance=inf': 11, 'window_size=4': 4,
    'window_size=13': 12, 'num_levels=0': 22, 'num_levels=True': 27, 'num_levels=5': 24, 'num_iterations=0': 23,
    'num_iterations=1.5': 28, 'max_residual=nan': 25, 'max_residual=-1': 29, 'detect_every=0': 18, 'detect_every=-1': 21,
    'detect_every=True': 19, 'detect_every=1.5': 20, 'T=1': 5, 'frames 2-D': 13, 'frames empty': 14, 'frames item 3-D': 15,
    'frames mixed shapes': 16, 'frames mixed dtypes': 17, 'frames H=1': 68, 'colour float32': 56, 'colour C=5': 55,
    'colour H=1': 57, 'colour T=1': 5, 'nv12 4-D': 60, 'nv12 float32': 61, 'nv12 rows=35': 59, 'nv12 W=31': 62, 'nv12 tiny': 63,
    'nv12 T=1': 5, 'queries 1-D': 26, 'queries t=9': 30, 'queries t=0.5': 30, 'refine_iterations=-1': 31,
    'refine_iterations=True': 41, 'refine_iterations=1.5': 42, 'refine_photometric alone': 32, 'refine_robust_delta alone': 33,
    'order=xyz': 34, 'order=0': 43, 'order=None': 89, 'order=rgb': 93, 'siting=x': 58, 'model=x': 35, 'model=7': 44,
    'model=True': 45, 'hypotheses=0': 36, 'hypotheses=65537': 46, 'hypotheses=True': 47, 'threshold=nan': 37, 'threshold=0': 48,
    'seed=-1': 38, 'seed=2^32': 49, 'seed=1.5': 50, 'radius=-1': 39, 'radius=65': 51, 'radius=True': 52, 'sigma=0': 40,
    'sigma=nan': 53, 'sigma=0.01': 54, 'blend=x': 64, 'anchor=3': 65, 'anchor=-1': 69, 'anchor=True': 70, 'extent=0': 66,
    'extent=nan': 71, 'max_pixels=0': 67, 'max_pixels=True': 72, 'max_pixels=1.5': 73, 'prev 3-D': 74, 'curr other shape': 75,
    'points 1-D': 76, 'points empty': 77, 'shape 1-D': 78, 'shape H=0': 81, 'shape H=1': 87, 'shape 4-D': 88, 'shape 3-D': 82,
    'channels=5': 90, 'shape H=25': 92, 'shape H=2': 95, 'dtype=int16': 79, 'dtype=float32': 91, 'layout=x': 85,
    'nv12 float': 97, 'nv12 channels': 97, 'channels float': 91, 'tracks 2-D': 98, 'tracks T=1': 101,
    'visible other shape': 102, 'born other shape': 99, 't0=-1': 100, 't0=True': 103, 'step0=-1': 100, 'step0=2^31': 107,
    'dst other shape': 104, 'src 1-D': 106, 'valid other shape': 105, 'models (2, 5)': 108, 'status other shape': 109,
    'kind=x': 110, 'kind=0': 119, 'levels=0': 111, 'levels=True': 120, 'iterations=0': 112, 'iterations=1.5': 121,
    'min_share=0': 113, 'min_share=2': 122, 'min_share=nan': 123, 'robust_delta=0': 114, 'robust_delta=nan': 124,
    'robust_delta=x': 125, 'robust_delta=True': 126, 'robust_delta=1e40': 127, 'robust_delta=None': 133, 'a 4-D': 115,
    'a empty': 128, 'b other shape': 116, 'frames 4-D': 115, 'align T=1': 131, 'model size': 117, 'gain alone': 132,
    'gain shape': 134, 'maps (T, 5)': 139, 'maps (T, 2, 3)': 140, 'maps (9, 3)': 141, 'maps 4-D': 137, 'canvas_shape 1-D': 143,
    'canvas_shape Hc=0': 147, 'canvas 2^30': 148, 'origin=True': 144, 'origin 1-D': 149, 'origin=2^31': 150,
    'skip other shape': 145, 'exposure other shape': 146, 'model (2, 5)': 152, 'bias other shape': 154, 'frame 3-D': 155,
    'xy 1-D': 156, 'visible other length': 160, 'max_corners=5': 157, 't=-1': 158, 't=True': 163, 't=1.5': 164,
    'qt other shape': 159, 'qxy other shape': 165,
}
EXCEPT = {   # (call, fault) -> message, where a call words the fault differently
    ('tracker', 'detect_every=-1'): 80, ('tracker', 'detect_every=True'): 83, ('tracker', 'detect_every=1.5'): 84,
    ('online', 'shape 1-D'): 86, ('online', 'detect_every=-1'): 80, ('online', 'shape 3-D'): 89,
    ('online', 'detect_every=True'): 83, ('online', 'detect_every=1.5'): 84, ('online-colour', 'detect_every=-1'): 80,
    ('online-nv12', 'dtype=float32'): 94, ('online-nv12', 'detect_every=-1'): 80, ('online-nv12', 'shape 3-D'): 96,
    ('refine_alignment-f32', 'status other shape'): 118, ('refine_alignment-u8', 'b other shape'): 129,
    ('refine_alignment-u8', 'status other shape'): 118, ('sequence_refine_alignment-f32', 'model size'): 130,
    ('sequence_refine_alignment-f32', 'frames empty'): 128, ('sequence_refine_alignment-u8', 'model size'): 130,
    ('sequence_refine_alignment-u8', 'frames empty'): 128, ('alignment_weights-u8', 'b other shape'): 129,
    ('warp_affine-grey', 'maps (T, 5)'): 135, ('warp_affine-grey', 'maps (9, 3)'): 136, ('warp_affine-grey', 'frames empty'): 128,
    ('warp_affine-colour', 'maps (T, 5)'): 135, ('warp_affine-colour', 'maps (9, 3)'): 136, ('warp_affine-nv12', 'maps (T, 5)'): 135,
    ('warp_affine-nv12', 'nv12 4-D'): 138, ('warp_affine-nv12', 'maps (9, 3)'): 136, ('warp_perspective-grey', 'maps 4-D'): 142,
    ('warp_perspective-grey', 'frames empty'): 128, ('warp_perspective-nv12', 'nv12 4-D'): 138,
    ('mosaic_composite-grey', 'frames empty'): 128, ('mosaic_chain', 'shape 1-D'): 151, ('mosaic_chain', 'shape H=1'): 153,
    ('replenish_features', 'max_corners=True'): 161, ('replenish_features', 'max_corners=0'): 162,
}


def family(call):
    """the call's name in ORDER: the float32 and the uint8 form of a call share one"""
    return call if call in ORDER else call.rsplit("-", 1)[0]


def outcome(call, faults, monkeypatch):
    """(exception type's name, message) of `call` with the named faults put into its accepted arguments; None if it returns"""
    import _oflk

    fn, args = CALLS[call]
    args = dict(args)
    for f in faults:
        for name, value in (FAULTS[f] if isinstance(f, str) else f).items():
            assert name in args, (call, f)
            args[name] = value
    monkeypatch.setattr(_oflk, "_lib", StubLib())
    try:
        fn(**args)
    except Exception as e:   # noqa: BLE001 -- the type is part of what is pinned
        return type(e).__name__, str(e)
    return None


def expected(call, fault):
    return MESSAGES[EXCEPT.get((call, fault), EXPECTED[fault])]


def pairs(call):
    """each fault of ORDER with the next one that sets other arguments, then MORE_PAIRS'"""
    order = ORDER[family(call)]
    for i, a in enumerate(order):
        b = next((b for b in order[i + 1:] if not set(FAULTS[a]) & set(FAULTS[b])), None)
        if b:
            yield a, b
    yield from ((a, b) for f, a, b in MORE_PAIRS if f == family(call))


ONE = [(call, fault) for call in CALLS for fault in ORDER[family(call)] + EXTRA[family(call)]]
TWO = [(call, a, b) for call in CALLS for a, b in pairs(call)]


@pytest.mark.parametrize("call,fault", ONE, ids=[f"{c}-{x.replace(' ', '_')}" for c, x in ONE])
def test_one_wrong_argument_is_refused_with_its_type_and_message(call, fault, monkeypatch):
    assert outcome(call, [fault], monkeypatch) == expected(call, fault)


@pytest.mark.parametrize("call,a,b", TWO, ids=[f"{c}-{a.replace(' ', '_')}-{b.replace(' ', '_')}" for c, a, b in TWO])
def test_of_two_wrong_arguments_the_earlier_check_refuses(call, a, b, monkeypatch):
    assert outcome(call, [a, b], monkeypatch) == expected(call, a)


@pytest.mark.parametrize("call,values", ACCEPTED, ids=[f"{c}-{'-'.join(f'{k}={v!r}' for k, v in x.items())}" for c, x in ACCEPTED])
def test_edge_values_that_are_normalised_are_accepted(call, values, monkeypatch):
    for c in [c for c in CALLS if family(c) == call]:
        assert outcome(c, [values], monkeypatch) is None


def test_the_tables_go_together():
    assert {family(c) for c in CALLS} == set(ORDER) == set(EXTRA)
    for call in ORDER:
        faults = ORDER[call] + EXTRA[call]
        assert len(set(faults)) == len(faults), call
    assert {f for call in ORDER for f in ORDER[call] + EXTRA[call]} == set(EXPECTED) == set(FAULTS)
    assert all(name in ("ValueError", "TypeError") for name, _ in MESSAGES)


if __name__ == "__main__":   # the tables of the modules that are importable
    import os
    import sys
    from collections import Counter

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "optical-flow-fpga_amd", "python"))
    mp = pytest.MonkeyPatch()
    seen, messages = {}, []
    for call, fault in ONE:
        row = outcome(call, [fault], mp)
        assert row is not None, (call, fault, "was accepted")
        if row not in messages:
            messages.append(row)
        seen[call, fault] = messages.index(row)
    mp.undo()
    usual = {f: Counter(i for (c, g), i in seen.items() if g == f).most_common(1)[0][0] for f in FAULTS}
    print("MESSAGES = [")
    for i, row in enumerate(messages):
        print(f"    {row!r},{'   # ' + str(i) if i % 5 == 0 else ''}")
    print("]\nEXPECTED = {")
    for f in FAULTS:
        print(f"    {f!r}: {usual[f]},")
    print("}\nEXCEPT = {")
    for (c, f), i in seen.items():
        if i != usual[f]:
            print(f"    ({c!r}, {f!r}): {i},")
    print("}")
