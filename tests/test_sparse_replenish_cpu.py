"""CPU tests of the replenished-KLT statement on the sparse tracker (tests/sparse_replenish_model.py), of the new entry
points' refusals and of their Python shims' argument checks.  Nothing here touches a device."""
import ctypes

import numpy as np
import pytest

import feature_model as FM
import sparse_model as S
import sparse_replenish_model as M
from test_replenish_cpu import check_invariants
from test_sparse_cpu import INVALID, UNSUPPORTED, _drifting

SYMBOLS = ["oflk_pyramidal_sequence_klt_sparse", "oflk_pyramidal_sequence_klt_sparse_u8",
           "oflk_pyramidal_sequence_klt_sparse_replenish", "oflk_pyramidal_sequence_klt_sparse_replenish_u8",
           "oflk_plan_sparse_klt_replenish"]


# ---------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    """seven noisy drifting frames, their pyramids and the statement at D = 2, computed once"""
    T, H, W, K, md, q = 7, 40, 52, 40, 4.0, 0.05
    frames = _drifting(T, H, W, 3)
    pyr = [S.pyramid(f, 3) for f in frames]
    kw = dict(quality_level=q, min_distance=md)
    return dict(frames=frames, pyr=pyr, K=K, md=md, q=q, kw=kw, whole={D: M.sequence(frames, K, D, pyramids=pyr, **kw) for D in (1, 2, 3)})


def test_without_replenishing_it_is_detection_then_sparse_tracks(clip):
    frames, pyr, K = clip["frames"], clip["pyr"], clip["K"]
    T = frames.shape[0]
    n, xy, _ = FM.select(FM.score(frames[0], 5), clip["q"], clip["md"], K)
    assert 10 < n <= K
    wtr, wvis = S.track(frames, None, xy, 3, 5, 3, pyramids=pyr)   # the NaN rows from n on are never-visible tracks
    assert not wvis[-1].all() and wvis[-1].any(), "some tracks should end on this clip"
    for D in (T - 1, T, T + 1, 2 ** 31 - 1):   # T-1: the last frame never detects
        tr, vis, born, det, res = M.sequence(frames, K, D, pyramids=pyr, **clip["kw"])
        M.same((tr, vis), (wtr, wvis), f"D={D}")
        assert np.array_equal(born[0], vis[0]) and not born[1:].any() and det.tolist() == [n] + [0] * (T - 1)
        # the residual: NaN on row 0 and wherever the slot was dead on the row before; finite where the track goes on
        assert np.isnan(res[0]).all() and np.isnan(res[1:][vis[:-1] == 0]).all()
        assert np.isfinite(res[1:][vis[1:] == 1]).all() and (res[1:][vis[1:] == 1] <= np.float32(4.0)).all()


@pytest.mark.parametrize("D", [1, 2, 3])
def test_two_calls_cut_at_every_frame_equal_one(clip, D):
    frames, pyr, K = clip["frames"], clip["pyr"], clip["K"]
    whole = clip["whole"][D]
    for cut in range(1, frames.shape[0] - 1):
        M.same(M.sequence_in_two(frames, K, D, cut, pyramids=pyr, **clip["kw"]), whole, f"D={D} cut={cut}")


@pytest.mark.parametrize("D", [1, 2, 3])
def test_invariants_births_and_residuals(clip, D):
    tr, vis, born, det, res = clip["whole"][D]
    check_invariants(tr, vis, born, det, D, clip["md"])
    assert born[1:].any(), "ended tracks should be replaced on this clip"
    alive_before = np.vstack([np.zeros((1, vis.shape[1]), bool), vis[:-1].astype(bool)])
    assert np.isnan(res[~alive_before]).all(), "a slot dead on the row before has no step"
    cont = vis.astype(bool) & alive_before & ~born.astype(bool)
    assert np.isfinite(res[cont]).all() and (res[cont] <= np.float32(4.0)).all(), "a surviving step passed the residual test"
    ended = alive_before & ~cont
    assert ended.any() and (res[ended] > np.float32(4.0)).any(), "some track should end by the residual test"


def test_uint8_frames_are_their_float32_values():
    frames = np.rint(_drifting(4, 40, 52, 5)).astype(np.uint8)
    M.same(M.sequence(frames, 30, 2, 0.05, 4.0), M.sequence(frames.astype(np.float32), 30, 2, 0.05, 4.0), "uint8")


# ---------------------------------------------------------------------------------------------------------------
# refusals, before any device call
# ---------------------------------------------------------------------------------------------------------------
def _c_call(name, T=4, H=24, W=32, L=3, w=5, it=3, alpha=0.01, beta=0.5, mr=4.0, q=0.01, md=3.0, K=8, D=2, null=None, u8=False):
    """one of the host forms on zero frames; null: the name of a pointer argument to pass as NULL"""
    import _oflk

    Lb = _oflk.lib()
    Tn = max(T, 1)
    frames = np.zeros((Tn, H, W), np.uint8 if u8 else np.float32)
    tr, vis, born = np.empty((Tn, K if K > 0 else 1, 2), np.float32), np.empty((Tn, max(K, 1)), np.uint8), np.empty((Tn, max(K, 1)), np.uint8)
    det, res = np.empty(Tn, np.int32), np.empty((Tn, max(K, 1)), np.float32)
    cnt, xy, sc = np.zeros(1, np.int32), np.empty((max(K, 1), 2), np.float32), np.empty(max(K, 1), np.float32)
    a = dict(frames=frames.ctypes.data if u8 else _oflk.ptr(frames), tracks=_oflk.ptr(tr), visible=vis.ctypes.data, born=born.ctypes.data,
             detected=det.ctypes.data_as(_oflk._i32p), residual=_oflk.ptr(res), count=cnt.ctypes.data_as(_oflk._i32p), xy=_oflk.ptr(xy),
             score=_oflk.ptr(sc))
    if null:
        a[null] = None
    fn = getattr(Lb, name + ("_u8" if u8 else ""))
    if name.endswith("replenish"):
        return fn(a["frames"], T, H, W, L, w, it, alpha, beta, mr, q, md, K, D, a["tracks"], a["visible"], a["born"], a["detected"],
                  a["residual"])
    return fn(a["frames"], T, H, W, L, w, it, alpha, beta, mr, q, md, K, a["count"], a["xy"], a["score"], a["tracks"], a["visible"])


HOST = ["oflk_pyramidal_sequence_klt_sparse", "oflk_pyramidal_sequence_klt_sparse_replenish"]
REFUSALS = [
    (dict(T=1), INVALID), (dict(T=0), INVALID), (dict(w=4), UNSUPPORTED), (dict(w=13), UNSUPPORTED), (dict(w=1), UNSUPPORTED),
    (dict(H=7, W=9), UNSUPPORTED), (dict(H=1, W=40, L=1), UNSUPPORTED), (dict(it=0), INVALID), (dict(L=0), INVALID),
    (dict(alpha=-1.0), INVALID), (dict(beta=float("nan")), INVALID), (dict(alpha=float("inf")), INVALID), (dict(mr=-0.5), INVALID),
    (dict(mr=float("nan")), INVALID), (dict(q=2.0), INVALID), (dict(q=float("nan")), INVALID), (dict(md=-1.0), INVALID),
    (dict(md=float("inf")), INVALID), (dict(K=0), INVALID), (dict(K=-3), INVALID), (dict(null="frames"), INVALID),
    (dict(null="tracks"), INVALID), (dict(null="visible"), INVALID),
]


def test_symbols_and_signatures_exist():
    import _oflk

    for name in SYMBOLS:
        assert hasattr(_oflk.lib(), name) and name in _oflk.SIGNATURES, name
    assert callable(_oflk.sparse_klt_replenish)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("name", HOST)
@pytest.mark.parametrize("kw,code", REFUSALS, ids=lambda v: str(v))
def test_host_entry_points_refuse_without_a_device(kw, code, name, u8):
    assert _c_call(name, u8=u8, **kw) == code


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_host_entry_points_refuse_their_own_arguments(u8):
    import _oflk

    rep, klt = HOST[1], HOST[0]
    for D in (0, -1):
        assert _c_call(rep, D=D, u8=u8) == INVALID and b"detect_every" in _oflk.lib().oflk_last_error()
    for null in ("born", "detected"):
        assert _c_call(rep, null=null, u8=u8) == INVALID
    for null in ("count", "xy", "score"):
        assert _c_call(klt, null=null, u8=u8) == INVALID


def test_device_form_refuses_before_any_device_call():
    """a plan handle cannot exist without a device, so what answers here is the NULL plan; the other refusals of the device
    form are exercised on the GPU"""
    import _oflk

    fn = _oflk.lib().oflk_plan_sparse_klt_replenish
    assert fn(None, None, 0, 0.01, 0.5, 4.0, 0.01, 3.0, 8, 2, 0, None, 0, None, None, None, None, None, None, None, None) == INVALID
    assert fn(None, ctypes.c_void_p(256), 0, 0.01, 0.5, 4.0, 0.01, 3.0, 8, 2, 0, ctypes.c_void_p(256), 1 << 20, *([ctypes.c_void_p(256)] * 7),
              None) == INVALID


def test_shims_raise_value_error_before_any_device_call():
    import lucas_kanade_pyramidal as P

    seq = np.zeros((3, 24, 32), np.float32)
    fn = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            fn(seq, 10, bad)
    for kw in (dict(num_levels=0), dict(num_iterations=0), dict(window_size=4), dict(window_size=13), dict(window_size=1),
               dict(max_residual=-1.0), dict(max_residual=float("nan")), dict(alpha=-0.1), dict(beta=float("inf")),
               dict(quality_level=1.5), dict(min_distance=-1.0), dict(min_distance=float("inf"))):
        with pytest.raises(ValueError):
            fn(seq, 10, 2, **kw)
    for K in (0, -1, 2.5):
        with pytest.raises(ValueError):
            fn(seq, K, 2)
    with pytest.raises(ValueError):
        fn(seq[:1], 10, 2)
    with pytest.raises(ValueError):
        fn(np.zeros((3, 7, 9), np.float32), 10, 2)   # 7 x 9 at 3 levels: a level of width 1
    assert P.SequenceKLTSparseReplenish._fields == P.SequenceKLTReplenish._fields + ("residual",)
