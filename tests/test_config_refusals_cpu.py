"""The refusals of the entry points that take the tracking, fit, trajectory-window and alignment settings, and which refusal
wins when two arguments are wrong, through ctypes: oflk_tracker_create, oflk_tracker_set_motion, the three
oflk_stabilizer_create*, the four oflk_stabilize_sequence*, oflk_mosaic_sequence[_u8], the three alignment workspace calls,
the six alignment device calls, the twelve alignment host calls and the three oflk_align_weights*.

Every case is refused before the first device call, so the rows hold with or without a GPU; the device entry points get
dummy aligned integers as pointers, which no refused call reads.  A case that would reach the device has no row (an
accepted NULL such as d_status_in or d_photo, a robust call without its photometric part and no d_photo_out).

ORDER lists, per family of calls with one argument list, one fault per check in the order the checks are made.  EXPECTED
pins the return code and the exact oflk_last_error text of every fault alone (ORDER's and EXTRA's); it was recorded from the
library before the settings were passed as structs (`python tests/test_config_refusals_cpu.py` prints the table of the
library it loads).  Precedence: each fault of ORDER together with the next one that it can be combined with (another
argument) is refused with the earlier fault's code and text, and so are the pairs of MORE_PAIRS."""
import ctypes
import math

import numpy as np
import pytest

T, H, W, K = 3, 24, 32, 4
INVALID, UNSUPPORTED = -1, -4
PTR = 0x100000                                    # a dummy device pointer, 256-byte aligned; never read
BUF = np.zeros(T * H * W * 4, np.float32)         # host frames of every layout; never read either
OUT, BYTES, TRACKER = "out", "bytes", "tracker"   # a handle to receive, a size_t to receive, a tracker made for the call

_KLT = [("levels", 2), ("window_size", 5), ("iters", 3), ("alpha", 0.01), ("beta", 0.5), ("max_residual", math.inf),
        ("quality_level", 0.01), ("min_distance", 3.0), ("max_corners", K)]
_FIT = [("model", 2), ("hypotheses", 64), ("threshold", 1.5), ("seed", 7)]
_WINDOW = [("weights", np.array([1.0, 1.0, 1.0])), ("radius", 2)]
_ONLINE = _KLT + [("detect_every", 2)] + _FIT + _WINDOW
_STAB_OUT = [("out", BUF), ("correction", np.zeros((T, 6), np.float32)), ("model_out", np.zeros((T - 1, 6), np.float32)),
             ("counts_out", np.zeros((T - 1, 3), np.int32)), ("held", np.zeros(T - 1, np.uint8))]
_SHAPE = [("H", H), ("W", W)]
_ALIGN = _SHAPE + [("levels", 2), ("iterations", 2), ("model", 0), ("min_share", 0.25)]
_ROBUST = [("robust_delta", 4.0), ("photometric", 1)]
_D_IO = [("d_model_in", PTR + 0x1000), ("d_status_in", PTR + 0x2000), ("d_workspace", PTR + 0x10000), ("workspace_bytes", 1 << 30),
         ("d_model_out", PTR + 0x3000), ("d_status_out", PTR + 0x4000), ("d_stats", PTR + 0x5000)]
_D_PHOTO = [("d_photo_out", PTR + 0x6000)]
_H_IO = [("model_in", np.zeros((T, 9), np.float32)), ("status_in", np.zeros(T, np.int32)), ("model_out", np.zeros((T, 9), np.float32)),
         ("status_out", np.zeros(T, np.int32)), ("stats", np.zeros((T, 8), np.float64))]
_H_PHOTO = [("photo_out", np.zeros((T, 2), np.float32))]
_D_PAIR = [("d_a", PTR + 0x20000), ("d_b", PTR + 0x40000), ("u8", 0), ("S", 2)]
_D_SEQ = [("d_frames", PTR + 0x20000), ("u8", 0), ("T", T)]
_H_PAIR = [("a", BUF), ("b", BUF), ("S", 2)]
_H_SEQ = [("frames", BUF), ("T", T)]

# fault -> the arguments it sets
FAULTS = {
    "out NULL": {"out": None}, "tr NULL": {"tr": None}, "bytes NULL": {"bytes": None}, "canvas NULL": {"canvas": None},
    "frames NULL": {"frames": None}, "a NULL": {"a": None}, "b NULL": {"b": None}, "model_in NULL": {"model_in": None},
    "model_out NULL": {"model_out": None}, "status_out NULL": {"status_out": None}, "stats NULL": {"stats": None},
    "photo_out NULL": {"photo_out": None}, "weights NULL": {"weights": None},
    "d_a NULL": {"d_a": None}, "d_b NULL": {"d_b": None}, "d_frames NULL": {"d_frames": None}, "d_model_in NULL": {"d_model_in": None},
    "d_workspace NULL": {"d_workspace": None}, "d_model_out NULL": {"d_model_out": None}, "d_status_out NULL": {"d_status_out": None},
    "d_stats NULL": {"d_stats": None}, "d_photo_out NULL": {"d_photo_out": None}, "d_model NULL": {"d_model": None},
    "d_weights NULL": {"d_weights": None},
    "d_a misaligned": {"d_a": PTR + 0x20002}, "d_frames misaligned": {"d_frames": PTR + 0x20002},
    "d_workspace misaligned": {"d_workspace": PTR + 0x10010}, "d_stats misaligned": {"d_stats": PTR + 0x5004},
    "d_photo_out misaligned": {"d_photo_out": PTR + 0x6002}, "d_model misaligned": {"d_model": PTR + 0x1002},
    "d_photo misaligned": {"d_photo": PTR + 0x6002}, "workspace_bytes=16": {"workspace_bytes": 16},
    "T=1": {"T": 1}, "S=0": {"S": 0}, "H=0": {"H": 0}, "H=1": {"H": 1}, "W=1": {"W": 1}, "H=5": {"H": 5}, "H=2^23": {"H": 1 << 23},
    "2^29 pixels": {"H": 1 << 14, "W": 1 << 15}, "2^30 pixels": {"H": 1 << 15, "W": 1 << 15},
    "2^31 packed bytes": {"H": 30000, "W": 30000}, "device=-1": {"device": -1},
    "channels=5": {"channels": 5}, "order=9": {"order": 9}, "siting=9": {"siting": 9},
    "levels=0": {"levels": 0}, "levels=17": {"levels": 17}, "levels=3": {"levels": 3}, "levels=5": {"levels": 5},
    "window_size=4": {"window_size": 4}, "iters=0": {"iters": 0}, "alpha=-1": {"alpha": -1.0}, "beta=inf": {"beta": math.inf},
    "max_residual=nan": {"max_residual": math.nan}, "quality_level=2": {"quality_level": 2.0}, "min_distance=-1": {"min_distance": -1.0},
    "max_corners=0": {"max_corners": 0}, "detect_every=0": {"detect_every": 0}, "detect_every=-1": {"detect_every": -1},
    "model=7": {"model": 7}, "hypotheses=0": {"hypotheses": 0}, "threshold=nan": {"threshold": math.nan},
    "radius=-1": {"radius": -1}, "weights[1]=nan": {"weights": np.array([1.0, math.nan, 1.0])},
    "weights[0]=0": {"weights": np.array([0.0, 1.0, 1.0])},
    "blend=9": {"blend": 9}, "anchor=3": {"anchor": 3}, "anchor=-1": {"anchor": -1}, "extent=0": {"extent": 0.0},
    "iterations=0": {"iterations": 0}, "min_share=0": {"min_share": 0.0}, "min_share=2": {"min_share": 2.0},
    "robust_delta=0": {"robust_delta": 0.0}, "robust_delta=nan": {"robust_delta": math.nan},
}

# the checks in the order they are made, one fault each
_SPARSE_TEST = ["alpha=-1", "max_residual=nan"]
_SPARSE_CONFIG = ["levels=0", "iters=0", "window_size=4", "levels=5"]
_SELECT = ["quality_level=2", "min_distance=-1", "max_corners=0"]
_RANSAC = ["hypotheses=0", "threshold=nan"]
_MOTION = ["model=7"] + _RANSAC
_STAB_WINDOW = ["radius=-1", "weights NULL", "weights[1]=nan"]
_TRACKER = ["2^29 pixels", "H=2^23"] + _SPARSE_TEST + _SPARSE_CONFIG + _SELECT + ["detect_every=-1", "device=-1"]
_SEQ_CONFIG = _MOTION + _STAB_WINDOW + ["detect_every=0"] + _SELECT + _SPARSE_TEST + _SPARSE_CONFIG
_FRAMES = ["H=1", "frames NULL", "2^30 pixels", "H=2^23"]
_ALIGN_SHAPE = ["H=0", "2^30 pixels", "H=2^23", "model=7"]
_ALIGN_CONFIG = _ALIGN_SHAPE + ["iterations=0", "min_share=0", "levels=0", "levels=3"]
_ALIGN_DEVICE = ["workspace_bytes=16", "d_workspace misaligned"]
_KLT_EXTRA = ["beta=inf", "levels=17"]
_D_NULLS = ["d_model_in NULL", "d_workspace NULL", "d_model_out NULL", "d_status_out NULL", "d_stats NULL", "d_stats misaligned",
            "min_share=2", "levels=17"]
_H_NULLS = ["model_in NULL", "model_out NULL", "status_out NULL", "stats NULL", "min_share=2", "levels=17"]

# family -> (its calls, the arguments in the order of include/oflk.h with values that the call accepts, ORDER, EXTRA)
FAMILIES = {
    "tracker_create": (["oflk_tracker_create"], [("out", OUT), ("device", 0)] + _SHAPE + [("u8", 1)] + _KLT + [("detect_every", 2)],
                       ["out NULL", "H=0"] + _TRACKER, _KLT_EXTRA),
    "tracker_set_motion": (["oflk_tracker_set_motion"], [("tr", TRACKER)] + _FIT, ["tr NULL"] + _MOTION, []),
    "stabilizer_create": (["oflk_stabilizer_create"], [("out", OUT), ("device", 0)] + _SHAPE + [("u8", 1)] + _ONLINE,
                          ["out NULL", "H=1"] + _MOTION + _STAB_WINDOW + _TRACKER, _KLT_EXTRA + ["W=1", "weights[0]=0"]),
    "stabilizer_create_packed": (["oflk_stabilizer_create_packed"],
                                 [("out", OUT), ("device", 0)] + _SHAPE + [("channels", 3), ("order", 0)] + _ONLINE,
                                 ["out NULL", "channels=5", "order=9", "H=1", "2^31 packed bytes"] + _MOTION + _STAB_WINDOW + _TRACKER,
                                 _KLT_EXTRA),
    "stabilizer_create_nv12": (["oflk_stabilizer_create_nv12"], [("out", OUT), ("device", 0)] + _SHAPE + [("siting", 0)] + _ONLINE,
                               ["out NULL", "H=5", "siting=9"] + _MOTION + _STAB_WINDOW + _TRACKER, _KLT_EXTRA + ["H=1"]),
    "stabilize_sequence": (["oflk_stabilize_sequence", "oflk_stabilize_sequence_u8"], _H_SEQ + _SHAPE + _ONLINE + _STAB_OUT,
                           ["T=1"] + _FRAMES + _SEQ_CONFIG, _KLT_EXTRA + ["out NULL", "W=1", "weights[0]=0"]),
    "stabilize_sequence_packed": (["oflk_stabilize_sequence_packed"],
                                  _H_SEQ + _SHAPE + [("channels", 3), ("order", 0)] + _ONLINE + _STAB_OUT,
                                  ["channels=5", "order=9", "T=1"] + _FRAMES + ["2^31 packed bytes"] + _SEQ_CONFIG,
                                  _KLT_EXTRA + ["out NULL"]),
    "stabilize_sequence_nv12": (["oflk_stabilize_sequence_nv12"], _H_SEQ + _SHAPE + [("siting", 0)] + _ONLINE + _STAB_OUT,
                                ["H=5", "siting=9", "T=1", "frames NULL", "2^30 pixels", "H=2^23"] + _SEQ_CONFIG,
                                _KLT_EXTRA + ["out NULL", "H=1"]),
    "mosaic_sequence": (["oflk_mosaic_sequence", "oflk_mosaic_sequence_u8"],
                        _H_SEQ + _SHAPE + _KLT + [("detect_every", 2)] + _FIT[1:]
                        + [("anchor", 1), ("extent", 8.0), ("blend", 0), ("out", BUF), ("capacity", 1 << 20), ("canvas", np.zeros(4, np.int32)),
                           ("count", np.zeros(1 << 12, np.int32)), ("to_anchor", np.zeros((T, 9), np.float64)), ("held", np.zeros(T, np.uint8)),
                           ("dropped", np.zeros(T, np.uint8)), ("model_out", np.zeros((T, 9), np.float32)),
                           ("counts_out", np.zeros((T, 3), np.int32))],
                        ["T=1", "canvas NULL"] + _FRAMES + _RANSAC + ["blend=9", "anchor=3", "extent=0", "detect_every=0"] + _SELECT
                        + _SPARSE_TEST + _SPARSE_CONFIG, _KLT_EXTRA + ["out NULL", "W=1", "anchor=-1"]),
    "align_workspace": (["oflk_align_workspace", "oflk_align_photo_workspace"],
                        [("S", 2)] + _SHAPE + [("levels", 2), ("model", 0), ("bytes", BYTES)],
                        ["bytes NULL", "S=0"] + _ALIGN_SHAPE + ["levels=0", "levels=3"], ["levels=17"]),
    "align_robust_workspace": (["oflk_align_robust_workspace"],
                               [("S", 2)] + _SHAPE + [("levels", 2), ("model", 0), ("photometric", 1), ("bytes", BYTES)],
                               ["bytes NULL", "S=0"] + _ALIGN_SHAPE + ["levels=0", "levels=3"], ["levels=17"]),
    "align_refine": (["oflk_align_refine"], _D_PAIR + _ALIGN + _D_IO + [("stream", None)],
                     ["S=0"] + _ALIGN_CONFIG + ["d_a NULL"] + _ALIGN_DEVICE + ["d_a misaligned"], _D_NULLS + ["d_b NULL"]),
    "align_refine_photo": (["oflk_align_refine_photo"], _D_PAIR + _ALIGN + _D_IO + _D_PHOTO + [("stream", None)],
                           ["S=0"] + _ALIGN_CONFIG + ["d_a NULL"] + _ALIGN_DEVICE + ["d_a misaligned", "d_photo_out NULL"],
                           _D_NULLS + ["d_b NULL", "d_photo_out misaligned"]),
    "align_refine_robust": (["oflk_align_refine_robust"], _D_PAIR + _ALIGN + _ROBUST + _D_IO + _D_PHOTO + [("stream", None)],
                            ["S=0"] + _ALIGN_CONFIG + ["robust_delta=0", "d_a NULL"] + _ALIGN_DEVICE + ["d_a misaligned", "d_photo_out NULL"],
                            _D_NULLS + ["d_b NULL", "d_photo_out misaligned", "robust_delta=nan"]),
    "align_sequence": (["oflk_align_sequence"], _D_SEQ + _ALIGN + _D_IO + [("stream", None)],
                       ["T=1"] + _ALIGN_CONFIG + ["d_frames NULL"] + _ALIGN_DEVICE + ["d_frames misaligned"], _D_NULLS),
    "align_sequence_photo": (["oflk_align_sequence_photo"], _D_SEQ + _ALIGN + _D_IO + _D_PHOTO + [("stream", None)],
                             ["T=1"] + _ALIGN_CONFIG + ["d_frames NULL"] + _ALIGN_DEVICE + ["d_frames misaligned", "d_photo_out NULL"],
                             _D_NULLS + ["d_photo_out misaligned"]),
    "align_sequence_robust": (["oflk_align_sequence_robust"], _D_SEQ + _ALIGN + _ROBUST + _D_IO + _D_PHOTO + [("stream", None)],
                              ["T=1"] + _ALIGN_CONFIG + ["robust_delta=0", "d_frames NULL"] + _ALIGN_DEVICE
                              + ["d_frames misaligned", "d_photo_out NULL"], _D_NULLS + ["d_photo_out misaligned", "robust_delta=nan"]),
    "align_refine_host": (["oflk_align_refine_host", "oflk_align_refine_host_u8"], _H_PAIR + _ALIGN + _H_IO,
                          ["S=0"] + _ALIGN_CONFIG + ["a NULL"], _H_NULLS + ["b NULL"]),
    "align_refine_photo_host": (["oflk_align_refine_photo_host", "oflk_align_refine_photo_host_u8"], _H_PAIR + _ALIGN + _H_IO + _H_PHOTO,
                                ["S=0"] + _ALIGN_CONFIG + ["a NULL"], _H_NULLS + ["b NULL", "photo_out NULL"]),
    "align_refine_robust_host": (["oflk_align_refine_robust_host", "oflk_align_refine_robust_host_u8"],
                                 _H_PAIR + _ALIGN + _ROBUST + _H_IO + _H_PHOTO, ["S=0"] + _ALIGN_CONFIG + ["robust_delta=0", "a NULL"],
                                 _H_NULLS + ["b NULL", "photo_out NULL", "robust_delta=nan"]),
    "align_sequence_host": (["oflk_align_sequence_host", "oflk_align_sequence_host_u8"], _H_SEQ + _ALIGN + _H_IO,
                            ["T=1"] + _ALIGN_CONFIG + ["frames NULL"], _H_NULLS),
    "align_sequence_photo_host": (["oflk_align_sequence_photo_host", "oflk_align_sequence_photo_host_u8"],
                                  _H_SEQ + _ALIGN + _H_IO + _H_PHOTO, ["T=1"] + _ALIGN_CONFIG + ["frames NULL"],
                                  _H_NULLS + ["photo_out NULL"]),
    "align_sequence_robust_host": (["oflk_align_sequence_robust_host", "oflk_align_sequence_robust_host_u8"],
                                   _H_SEQ + _ALIGN + _ROBUST + _H_IO + _H_PHOTO,
                                   ["T=1"] + _ALIGN_CONFIG + ["robust_delta=0", "frames NULL"],
                                   _H_NULLS + ["photo_out NULL", "robust_delta=nan"]),
    "align_weights": (["oflk_align_weights"],
                      _D_PAIR + _SHAPE + [("model", 0), ("robust_delta", 4.0), ("d_model", PTR + 0x1000), ("d_photo", PTR + 0x6000),
                                          ("d_weights", PTR + 0x80000), ("stream", None)],
                      ["S=0"] + _ALIGN_SHAPE + ["robust_delta=0", "d_a NULL", "d_a misaligned"],
                      ["d_b NULL", "d_model NULL", "d_weights NULL", "d_model misaligned", "d_photo misaligned", "robust_delta=nan"]),
    "align_weights_host": (["oflk_align_weights_host", "oflk_align_weights_host_u8"],
                           _H_PAIR + _SHAPE + [("model", 0), ("robust_delta", 4.0), ("model_in", np.zeros((T, 9), np.float32)),
                                               ("photo", np.zeros((T, 2), np.float32)), ("weights", BUF)],
                           ["S=0"] + _ALIGN_SHAPE + ["robust_delta=0", "a NULL"], ["b NULL", "model_in NULL", "weights NULL", "robust_delta=nan"]),
}

# pairs that are not neighbours in ORDER: (family, the fault that wins, the other)
MORE_PAIRS = [(f, "model=7", "radius=-1") for f in FAMILIES if f.startswith("stabiliz")] + [
    ("align_refine", "S=0", "model=7"), ("align_refine_host", "S=0", "model=7"), ("align_workspace", "S=0", "model=7"),
    ("align_refine_robust", "robust_delta=0", "d_photo_out NULL"), ("align_sequence_robust", "robust_delta=0", "d_photo_out NULL"),
    ("align_refine_robust_host", "robust_delta=0", "photo_out NULL"), ("align_sequence_robust_host", "robust_delta=0", "photo_out NULL"),
    ("align_refine", "min_share=0", "levels=0"), ("align_sequence_photo", "min_share=0", "levels=0"),
    ("align_refine_robust_host", "min_share=0", "levels=0"), ("align_sequence_host", "min_share=0", "levels=0"),
    ("mosaic_sequence", "hypotheses=0", "max_corners=0"), ("tracker_create", "alpha=-1", "max_corners=0"),
]

MESSAGES = [   # EXPECTED's values are indices into this list
    (-1, 'tracker pointer is NULL'),                                                                   # 0
    (-1, 'H and W must be >= 1 (got 0 x 32)'),
    (-4, 'frames of 2^29 pixels or more are not supported'),
    (-4, 'frames of 2^23 rows or columns or more are not supported (got 8388608 x 32)'),
    (-1, 'alpha and beta must be finite and >= 0 (got -1, 0.5)'),
    (-1, 'max_residual must be >= 0 (+inf disables the test)'),                                        # 5
    (-1, 'levels must be in [1,16] (got 0)'),
    (-1, 'the sparse tracker needs iters >= 1 (got 0)'),
    (-4, 'the sparse tracker is built for the odd windows 3 ... 11 (got 4)'),
    (-4, 'pyramid level 0 of 32x24 would be 2x1: the sparse tracker needs 2 x 2'),
    (-1, 'quality_level must be in [0,1] (got 2)'),                                                    # 10
    (-1, 'min_distance must be finite and >= 0 (got -1)'),
    (-1, 'max_corners must be >= 1 (got 0)'),
    (-1, 'detect_every must be >= 0 (0: never detect; got -1)'),
    (-1, 'device -1 out of range'),
    (-1, 'alpha and beta must be finite and >= 0 (got 0.01, inf)'),                                    # 15
    (-1, 'levels must be in [1,16] (got 17)'),
    (-1, 'NULL tracker'),
    (-1, 'unknown motion model 7'),
    (-1, 'hypotheses must be in [1, 65536] (got 0)'),
    (-1, 'threshold must be finite and > 0 (got nan)'),                                                # 20
    (-1, 'stabiliser pointer is NULL'),
    (-1, 'H and W must be >= 2 (got 1 x 32)'),
    (-1, 'radius must be in [0, 64] (got -1)'),
    (-1, 'NULL weights'),
    (-1, 'weights[1] must be finite and > 0 (got nan)'),                                               # 25
    (-1, 'H and W must be >= 2 (got 24 x 1)'),
    (-1, 'weights[0] must be finite and > 0 (got 0)'),
    (-1, 'channels must be 3 or 4 (got 5)'),
    (-1, 'order must be OFLK_ORDER_RGB or OFLK_ORDER_BGR (got 9)'),
    (-4, 'packed frames of 2^31 bytes or more are not supported'),                                     # 30
    (-1, 'NV12 frames need even H and W >= 4 (got 5 x 32)'),
    (-1, 'siting must be OFLK_SITING_LEFT or OFLK_SITING_CENTER (got 9)'),
    (-1, 'NV12 frames need even H and W >= 4 (got 1 x 32)'),
    (-1, 'a sequence needs T >= 2 frames (got 1)'),
    (-1, 'NULL input or output argument'),                                                             # 35
    (-4, 'frames of 2^30 pixels or more are not supported'),
    (-1, 'detect_every must be >= 1 (got 0)'),
    (-1, 'NULL canvas'),
    (-1, 'unknown blend 9'),
    (-1, 'anchor must be in [0, 2] (got 3)'),                                                          # 40
    (-1, 'extent must be finite and > 0 (got 0)'),
    (-1, 'anchor must be in [0, 2] (got -1)'),
    (-1, 'bytes is NULL'),
    (-1, 'S must be >= 1 (got 0)'),
    (-1, 'unknown model 7'),                                                                           # 45
    (-4, 'pyramid level 0 of 32x24 would be 8x6: the alignment needs 8 x 8'),
    (-1, 'iterations must be >= 1 (got 0)'),
    (-1, 'min_share must be in (0, 1] (got 0)'),
    (-1, 'NULL input, workspace or output argument'),
    (-1, 'workspace of 16 bytes, 3840 needed (oflk_align_workspace)'),                                 # 50
    (-1, 'd_workspace must be 256-byte aligned, d_stats 8-byte aligned'),
    (-1, 'float32 frames must be 4-byte aligned'),
    (-1, 'min_share must be in (0, 1] (got 2)'),
    (-1, 'workspace of 16 bytes, 4352 needed (oflk_align_workspace)'),
    (-1, 'NULL d_photo_out'),                                                                          # 55
    (-1, 'd_photo_out must be 4-byte aligned'),
    (-1, 'robust_delta must be finite and > 0 (got 0)'),
    (-1, 'workspace of 16 bytes, 4608 needed (oflk_align_workspace)'),
    (-1, 'robust_delta must be finite and > 0 (got nan)'),
    (-1, 'float32 arguments must be 4-byte aligned'),                                                  # 60
]
_E_KLT = {'alpha=-1': 4, 'max_residual=nan': 5, 'levels=0': 6, 'iters=0': 7, 'window_size=4': 8, 'levels=5': 9, 'quality_level=2': 10,
          'min_distance=-1': 11, 'max_corners=0': 12, 'beta=inf': 15, 'levels=17': 16}
_E_TRACKER = {**_E_KLT, '2^29 pixels': 2, 'H=2^23': 3, 'detect_every=-1': 13, 'device=-1': 14}
_E_MOTION = {'model=7': 18, 'hypotheses=0': 19, 'threshold=nan': 20}
_E_WINDOW = {'radius=-1': 23, 'weights NULL': 24, 'weights[1]=nan': 25}
_E_CREATE = {**_E_TRACKER, **_E_MOTION, **_E_WINDOW, 'out NULL': 21}
_E_SEQ = {**_E_KLT, **_E_MOTION, **_E_WINDOW, 'T=1': 34, 'frames NULL': 35, '2^30 pixels': 36, 'H=2^23': 3, 'detect_every=0': 37,
          'out NULL': 35}
_E_ALIGN_SHAPE = {'H=0': 1, '2^30 pixels': 36, 'H=2^23': 3, 'model=7': 45}
_E_ALIGN_WS = {**_E_ALIGN_SHAPE, 'bytes NULL': 43, 'S=0': 44, 'levels=0': 6, 'levels=3': 46, 'levels=17': 16}
_E_ALIGN = {**_E_ALIGN_SHAPE, 'iterations=0': 47, 'min_share=0': 48, 'levels=0': 6, 'levels=3': 46, 'min_share=2': 53, 'levels=17': 16}
_E_ALIGN_D = {**_E_ALIGN, 'd_workspace misaligned': 51, 'd_model_in NULL': 49, 'd_workspace NULL': 49, 'd_model_out NULL': 49,
              'd_status_out NULL': 49, 'd_stats NULL': 49, 'd_stats misaligned': 51}
_E_ALIGN_H = {**_E_ALIGN, 'model_in NULL': 35, 'model_out NULL': 35, 'status_out NULL': 35, 'stats NULL': 35}
_E_PAIR_D = {'S=0': 44, 'd_a NULL': 49, 'd_b NULL': 49, 'd_a misaligned': 52}
_E_SEQ_D = {'T=1': 34, 'd_frames NULL': 49, 'd_frames misaligned': 52}
_E_PAIR_H = {'S=0': 44, 'a NULL': 35, 'b NULL': 35}
_E_SEQ_H = {'T=1': 34, 'frames NULL': 35}
_E_PHOTO_D = {'workspace_bytes=16': 54, 'd_photo_out NULL': 55, 'd_photo_out misaligned': 56}
_E_ROBUST_D = {**_E_PHOTO_D, 'workspace_bytes=16': 58, 'robust_delta=0': 57, 'robust_delta=nan': 59}
_E_ROBUST_H = {'photo_out NULL': 35, 'robust_delta=0': 57, 'robust_delta=nan': 59}
EXPECTED = {
    'tracker_create': {**_E_TRACKER, 'out NULL': 0, 'H=0': 1},
    'tracker_set_motion': {**_E_MOTION, 'tr NULL': 17},
    'stabilizer_create': {**_E_CREATE, 'H=1': 22, 'W=1': 26, 'weights[0]=0': 27},
    'stabilizer_create_packed': {**_E_CREATE, 'channels=5': 28, 'order=9': 29, 'H=1': 22, '2^31 packed bytes': 30},
    'stabilizer_create_nv12': {**_E_CREATE, 'H=5': 31, 'siting=9': 32, 'H=1': 33},
    'stabilize_sequence': {**_E_SEQ, 'H=1': 22, 'W=1': 26, 'weights[0]=0': 27},
    'stabilize_sequence_packed': {**_E_SEQ, 'channels=5': 28, 'order=9': 29, 'H=1': 22, '2^31 packed bytes': 30},
    'stabilize_sequence_nv12': {**_E_SEQ, 'H=5': 31, 'siting=9': 32, 'H=1': 33},
    'mosaic_sequence': {**_E_KLT, 'T=1': 34, 'canvas NULL': 38, 'H=1': 22, 'frames NULL': 35, '2^30 pixels': 36, 'H=2^23': 3,
                        'hypotheses=0': 19, 'threshold=nan': 20, 'blend=9': 39, 'anchor=3': 40, 'extent=0': 41, 'detect_every=0': 37,
                        'out NULL': 35, 'W=1': 26, 'anchor=-1': 42},
    'align_workspace': _E_ALIGN_WS,
    'align_robust_workspace': _E_ALIGN_WS,
    'align_refine': {**_E_ALIGN_D, **_E_PAIR_D, 'workspace_bytes=16': 50},
    'align_refine_photo': {**_E_ALIGN_D, **_E_PAIR_D, **_E_PHOTO_D},
    'align_refine_robust': {**_E_ALIGN_D, **_E_PAIR_D, **_E_ROBUST_D},
    'align_sequence': {**_E_ALIGN_D, **_E_SEQ_D, 'workspace_bytes=16': 50},
    'align_sequence_photo': {**_E_ALIGN_D, **_E_SEQ_D, **_E_PHOTO_D},
    'align_sequence_robust': {**_E_ALIGN_D, **_E_SEQ_D, **_E_ROBUST_D},
    'align_refine_host': {**_E_ALIGN_H, **_E_PAIR_H},
    'align_refine_photo_host': {**_E_ALIGN_H, **_E_PAIR_H, 'photo_out NULL': 35},
    'align_refine_robust_host': {**_E_ALIGN_H, **_E_PAIR_H, **_E_ROBUST_H},
    'align_sequence_host': {**_E_ALIGN_H, **_E_SEQ_H},
    'align_sequence_photo_host': {**_E_ALIGN_H, **_E_SEQ_H, 'photo_out NULL': 35},
    'align_sequence_robust_host': {**_E_ALIGN_H, **_E_SEQ_H, **_E_ROBUST_H},
    'align_weights': {**_E_ALIGN_SHAPE, 'S=0': 44, 'robust_delta=0': 57, 'robust_delta=nan': 59, 'd_a NULL': 35, 'd_b NULL': 35,
                      'd_model NULL': 35, 'd_weights NULL': 35, 'd_a misaligned': 60, 'd_model misaligned': 60, 'd_photo misaligned': 60},
    'align_weights_host': {**_E_ALIGN_SHAPE, 'S=0': 44, 'robust_delta=0': 57, 'robust_delta=nan': 59, 'a NULL': 35, 'b NULL': 35,
                           'model_in NULL': 35, 'weights NULL': 35},
}


def refusal(call, args, faults):
    """(return code, oflk_last_error text) of `call` with the named faults put into its accepted arguments"""
    import _oflk

    L = _oflk.lib()
    fn = getattr(L, call)
    args = dict(args)
    for f in faults:
        for name, value in FAULTS[f].items():
            assert name in args, (call, f)
            args[name] = value
    assert len(args) == len(fn.argtypes), call
    handle, tracker, c_args = ctypes.c_void_p(), ctypes.c_void_p(), []
    for value, ctype in zip(args.values(), fn.argtypes):
        if value is OUT:
            value = ctypes.byref(handle)
        elif value is BYTES:
            value = ctypes.byref(ctypes.c_size_t())
        elif value is TRACKER:   # creation makes no device call
            assert L.oflk_tracker_create(ctypes.byref(tracker), 0, H, W, 1, 2, 5, 3, 0.01, 0.5, math.inf, 0.01, 3.0, K, 2) == 0
            value = tracker
        elif isinstance(value, np.ndarray):
            value = value.ctypes.data if ctype is ctypes.c_void_p else value.ctypes.data_as(ctype)
        c_args.append(value)
    rc = fn(*c_args)
    text = L.oflk_last_error().decode()
    if tracker:
        L.oflk_tracker_destroy(tracker)
    assert not handle, (call, faults, "was accepted")
    return rc, text


def pairs(family):
    """each fault of ORDER with the next one that sets other arguments, then MORE_PAIRS'"""
    order = FAMILIES[family][2]
    for i, a in enumerate(order):
        b = next((b for b in order[i + 1:] if not set(FAULTS[a]) & set(FAULTS[b])), None)
        if b:
            yield a, b
    yield from ((a, b) for f, a, b in MORE_PAIRS if f == family)


ONE = [(f, call, fault) for f, (calls, _, order, extra) in FAMILIES.items() for call in calls for fault in order + extra]
TWO = [(f, call, a, b) for f, (calls, _, _, _) in FAMILIES.items() for call in calls for a, b in pairs(f)]


@pytest.mark.parametrize("family,call,fault", ONE, ids=[f"{c}-{x.replace(' ', '_')}" for _, c, x in ONE])
def test_one_wrong_argument_is_refused_with_its_code_and_text(family, call, fault):
    assert refusal(call, FAMILIES[family][1], [fault]) == MESSAGES[EXPECTED[family][fault]]


@pytest.mark.parametrize("family,call,a,b", TWO, ids=[f"{c}-{a.replace(' ', '_')}-{b.replace(' ', '_')}" for _, c, a, b in TWO])
def test_of_two_wrong_arguments_the_earlier_check_refuses(family, call, a, b):
    assert refusal(call, FAMILIES[family][1], [a, b]) == MESSAGES[EXPECTED[family][a]]


def test_the_table_holds_every_fault_of_every_family_and_only_refusals():
    for family, (_, args, order, extra) in FAMILIES.items():
        assert sorted(EXPECTED[family]) == sorted(order + extra), family
        assert len(set(order + extra)) == len(order + extra), family
    assert all(rc in (INVALID, UNSUPPORTED) for rc, _ in MESSAGES)


if __name__ == "__main__":   # the table of the library that OFLK_LIB names
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "optical-flow-fpga_amd", "python"))
    messages, table = [], {}
    for family, (calls, args, order, extra) in FAMILIES.items():
        table[family] = {}
        for fault in order + extra:
            got = {refusal(call, args, [fault]) for call in calls}
            assert len(got) == 1 and next(iter(got))[0] in (INVALID, UNSUPPORTED), (family, fault, got)
            row = got.pop()
            if row not in messages:
                messages.append(row)
            table[family][fault] = messages.index(row)
    print("MESSAGES = [")
    for row in messages:
        print(f"    {row!r},")
    print("]\nEXPECTED = {")
    for family, rows in table.items():
        print(f"    {family!r}: {rows!r},")
    print("}")
