"""The refusals of the twelve host sequence track entry points (six calls, float32 and uint8 frames) and the NULL-plan
refusal of oflk_plan_sparse_klt_replenish, through ctypes.  Every one is made before the first device call, so the
rows hold with or without a GPU.  Each row of EXPECTED has exactly one wrong argument and pins the return code and the
exact oflk_last_error text; the table was recorded from the library before the six calls were given one driver, and a
case that reaches the device there (OFLK_ERR_NO_DEVICE without a GPU: the dense calls' window and iteration checks sit
in oflk_plan_create) is no refusal before the device and has no row."""
import ctypes
import math

import numpy as np
import pytest

T, H, W, N = 3, 24, 32, 4
INVALID, UNSUPPORTED = -1, -4

_CONFIG = [("T", T), ("H", H), ("W", W), ("levels", 2), ("window_size", 5), ("iters", 3), ("alpha", 0.01), ("beta", 0.5)]
_SELECT = [("quality_level", 0.01), ("min_distance", 3.0), ("max_corners", N)]
_QUERIES = [("qt", np.zeros(N, np.int32)), ("qxy", np.full((N, 2), 8.0, np.float32)), ("N", N)]
_ROWS = [("tracks", np.zeros((T, N, 2), np.float32)), ("visible", np.zeros((T, N), np.uint8))]
_FOUND = [("count", np.zeros(1, np.int32)), ("xy", np.zeros((N, 2), np.float32)), ("score", np.zeros(N, np.float32))]
_SLOTS = [("born", np.zeros((T, N), np.uint8)), ("detected", np.zeros(T, np.int32))]
_RES = [("max_residual", math.inf)]

# call -> its arguments after `frames`, in the order of include/oflk.h, with a value that the call accepts
CALLS = {
    "tracks": _CONFIG + _QUERIES + _ROWS,
    "klt": _CONFIG + _SELECT + _FOUND + _ROWS,
    "klt_replenish": _CONFIG + _SELECT + [("detect_every", 2)] + _ROWS + _SLOTS,
    "sparse_tracks": _CONFIG + _RES + _QUERIES + _ROWS,
    "klt_sparse": _CONFIG + _RES + _SELECT + _FOUND + _ROWS,
    "klt_sparse_replenish": _CONFIG + _RES + _SELECT + [("detect_every", 2)] + _ROWS + _SLOTS
                            + [("residual", np.zeros((T, N), np.float32))],
}

# fault -> (argument, wrong value)
FAULTS = {
    "T=1": ("T", 1), "H=0": ("H", 0), "levels=0": ("levels", 0), "alpha=-1": ("alpha", -1.0), "beta=inf": ("beta", math.inf),
    "max_residual=nan": ("max_residual", math.nan), "N=0": ("N", 0), "max_corners=0": ("max_corners", 0),
    "quality_level=2": ("quality_level", 2.0), "min_distance=-1": ("min_distance", -1.0), "detect_every=0": ("detect_every", 0),
    "qt outside": ("qt", np.array([0, 0, T, 0], np.int32)), "window_size=4": ("window_size", 4), "iters=0": ("iters", 0),
    "qxy NULL": ("qxy", None), "tracks NULL": ("tracks", None), "visible NULL": ("visible", None), "count NULL": ("count", None),
    "xy NULL": ("xy", None), "score NULL": ("score", None), "born NULL": ("born", None), "detected NULL": ("detected", None),
}

_T1 = (INVALID, "a sequence needs T >= 2 frames (got 1)")
_H0 = (INVALID, "H and W must be >= 1 (got 0 x 32)")
_LEVELS = (INVALID, "levels must be in [1,16] (got 0)")
_ALPHA = (INVALID, "alpha and beta must be finite and >= 0 (got -1, 0.5)")
_BETA = (INVALID, "alpha and beta must be finite and >= 0 (got 0.01, inf)")
_MAXRES = (INVALID, "max_residual must be >= 0 (+inf disables the test)")
_N0 = (INVALID, "N must be >= 1 (got 0)")
_K0 = (INVALID, "max_corners must be >= 1 (got 0)")
_Q2 = (INVALID, "quality_level must be in [0,1] (got 2)")
_MD = (INVALID, "min_distance must be finite and >= 0 (got -1)")
_EVERY = (INVALID, "detect_every must be >= 1 (got 0)")
_QT = (INVALID, "query 2: frame 3 outside [0,2]")
_NULLQ = (INVALID, "NULL query or output argument")
_NULLO = (INVALID, "NULL output argument")
_CORNERW = (UNSUPPORTED, "corner windows are odd sizes in [3,11] (got 4)")
_SPARSEW = (UNSUPPORTED, "the sparse tracker is built for the odd windows 3 ... 11 (got 4)")
_ITERS = (INVALID, "the sparse tracker needs iters >= 1 (got 0)")

EXPECTED = {
    "tracks": {"T=1": _T1, "H=0": _H0, "levels=0": _LEVELS, "alpha=-1": _ALPHA, "beta=inf": _BETA, "N=0": _N0, "qt outside": _QT,
               "qxy NULL": _NULLQ, "tracks NULL": _NULLQ, "visible NULL": _NULLQ},
    "klt": {"T=1": _T1, "H=0": _H0, "levels=0": _LEVELS, "alpha=-1": _ALPHA, "beta=inf": _BETA, "max_corners=0": _K0,
            "quality_level=2": _Q2, "min_distance=-1": _MD, "window_size=4": _CORNERW, "count NULL": _NULLO, "xy NULL": _NULLO,
            "score NULL": _NULLO, "tracks NULL": _NULLO, "visible NULL": _NULLO},
    "klt_replenish": {"T=1": _T1, "H=0": _H0, "levels=0": _LEVELS, "alpha=-1": _ALPHA, "beta=inf": _BETA, "max_corners=0": _K0,
                      "quality_level=2": _Q2, "min_distance=-1": _MD, "detect_every=0": _EVERY, "window_size=4": _CORNERW,
                      "tracks NULL": _NULLO, "visible NULL": _NULLO, "born NULL": _NULLO, "detected NULL": _NULLO},
    "sparse_tracks": {"T=1": _T1, "H=0": _H0, "levels=0": _LEVELS, "alpha=-1": _ALPHA, "beta=inf": _BETA,
                      "max_residual=nan": _MAXRES, "N=0": _N0, "qt outside": _QT, "window_size=4": _SPARSEW, "iters=0": _ITERS,
                      "qxy NULL": _NULLQ, "tracks NULL": _NULLQ, "visible NULL": _NULLQ},
    "klt_sparse": {"T=1": _T1, "H=0": _H0, "levels=0": _LEVELS, "alpha=-1": _ALPHA, "beta=inf": _BETA, "max_residual=nan": _MAXRES,
                   "max_corners=0": _K0, "quality_level=2": _Q2, "min_distance=-1": _MD, "window_size=4": _SPARSEW,
                   "iters=0": _ITERS, "count NULL": _NULLO, "xy NULL": _NULLO, "score NULL": _NULLO, "tracks NULL": _NULLO,
                   "visible NULL": _NULLO},
    "klt_sparse_replenish": {"T=1": _T1, "H=0": _H0, "levels=0": _LEVELS, "alpha=-1": _ALPHA, "beta=inf": _BETA,
                             "max_residual=nan": _MAXRES, "max_corners=0": _K0, "quality_level=2": _Q2, "min_distance=-1": _MD,
                             "detect_every=0": _EVERY, "window_size=4": _SPARSEW, "iters=0": _ITERS, "tracks NULL": _NULLO,
                             "visible NULL": _NULLO, "born NULL": _NULLO, "detected NULL": _NULLO},
}

# two faults at once: the call is refused with the code and text of one of them (which one is not promised)
PAIRS = [("tracks", "levels=0", "alpha=-1"), ("sparse_tracks", "levels=0", "alpha=-1"), ("klt_sparse", "T=1", "max_corners=0"),
         ("klt_replenish", "detect_every=0", "quality_level=2")]


def refusal(call, u8, faults):
    """(return code, oflk_last_error text) of `call` on 3 x 24 x 32 zero frames with the named faults put in"""
    import _oflk

    L = _oflk.lib()
    fn = getattr(L, f"oflk_pyramidal_sequence_{call}" + ("_u8" if u8 else ""))
    args = dict(CALLS[call])
    for f in faults:
        name, value = FAULTS[f]
        assert name in args, (call, f)
        args[name] = value
    frames = np.zeros((T, H, W), np.uint8 if u8 else np.float32)
    keep = [frames] + list(args.values())   # the arrays outlive the call
    c_args = []
    for value, ctype in zip(keep, fn.argtypes):
        if isinstance(value, np.ndarray):
            value = value.ctypes.data if ctype is ctypes.c_void_p else value.ctypes.data_as(ctype)
        c_args.append(value)
    rc = fn(*c_args)
    return rc, L.oflk_last_error().decode()


ROWS = [(call, fault) for call, faults in EXPECTED.items() for fault in faults]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("call,fault", ROWS, ids=[f"{c}-{f.replace(' ', '_')}" for c, f in ROWS])
def test_one_wrong_argument_is_refused_with_its_code_and_text(call, fault, u8):
    assert refusal(call, u8, [fault]) == EXPECTED[call][fault]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("call,a,b", PAIRS, ids=[f"{c}-{a}-{b}" for c, a, b in PAIRS])
def test_two_wrong_arguments_are_refused_with_one_of_their_own(call, a, b, u8):
    assert refusal(call, u8, [a, b]) in (EXPECTED[call][a], EXPECTED[call][b])


def test_the_table_covers_every_fault_that_applies_to_a_call():
    """a fault whose argument a call has is either in its table or one of the dense calls' two that reach the device"""
    reach_the_device = {("tracks", "window_size=4"), ("tracks", "iters=0"), ("klt", "iters=0"), ("klt_replenish", "iters=0")}
    for call, args in CALLS.items():
        names = dict(args)
        for fault, (name, _) in FAULTS.items():
            if name in names:
                assert (fault in EXPECTED[call]) != ((call, fault) in reach_the_device), (call, fault)


def test_the_plan_level_replenished_pass_refuses_a_null_plan():
    import _oflk

    L = _oflk.lib()
    rc = L.oflk_plan_sparse_klt_replenish(None, None, 0, 0.01, 0.5, math.inf, 0.01, 3.0, N, 2, 0, None, 0, *([None] * 8))
    assert (rc, L.oflk_last_error().decode()) == (INVALID, "NULL argument")
