"""CPU tests of the online sparse KLT tracker: its statement (tests/tracker_model.py) against the sequence statement, the
add_points rule, the new entry points' refusals and the Python shims' argument checks.  Nothing here touches a device."""
import ctypes

import numpy as np
import pytest

import feature_model as FM
import sparse_model as S
import sparse_replenish_model as M
import tracker_model as TM
from test_sparse_cpu import INVALID, UNSUPPORTED, _drifting

SYMBOLS = ["oflk_tracker_create", "oflk_tracker_destroy", "oflk_tracker_reset", "oflk_tracker_workspace_bytes",
           "oflk_tracker_frame_index", "oflk_tracker_push_device", "oflk_tracker_row_device", "oflk_tracker_read_row",
           "oflk_tracker_push", "oflk_tracker_add_points"]

CLIP = dict(T=8, H=40, W=52, seed=3, K=40, q=0.05, md=4.0)
ADD = dict(K=24, t_second=3, n_second=12, slots=[6, 7, 8, 10, 11, 14, 16, 21, 22])


# ---------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    """eight noisy drifting frames and their pyramids, computed once"""
    frames = _drifting(CLIP["T"], CLIP["H"], CLIP["W"], CLIP["seed"])
    return dict(frames=frames, pyr=[S.pyramid(f, 3) for f in frames], kw=dict(quality_level=CLIP["q"], min_distance=CLIP["md"]))


@pytest.mark.parametrize("D,accepted,reused", [(1, 6, 37), (2, 7, 32), (3, 11, 27)])
def test_pushes_are_the_rows_of_the_sequence_call_on_one_more_frame(clip, D, accepted, reused):
    """7 pushes == the 7-frame call told that an 8th frame follows == rows 0 .. 6 of the 8-frame call.  Row 6 is a detection
    row for every D here, and the plain 7-frame call (whose last row never detects) accepts nothing on it."""
    frames, pyr, K = clip["frames"], clip["pyr"], CLIP["K"]
    got, birth = TM.pushes(frames[:7], K, D, pyramids=pyr[:7], **clip["kw"])
    told = M.sequence(frames[:7], K, D, T=8, pyramids=pyr[:7], **clip["kw"])
    whole = M.sequence(frames, K, D, pyramids=pyr, **clip["kw"])
    plain = M.sequence(frames[:7], K, D, pyramids=pyr[:7], **clip["kw"])
    M.same(got, told, f"D={D}: pushes against the 7-frame call with T=8")
    M.same(told, tuple(a[:7] for a in whole), f"D={D}: the prefix of the 8-frame call")
    tr, vis, born, det, res = got
    assert det[6] > 0 and det[6] == accepted and plain[3][6] == 0, (det[6], plain[3][6])
    held = np.cumsum(np.vstack([np.zeros((1, K), np.uint8), vis[:-1]]), 0) > 0   # the slot held a track on an earlier row
    assert int((born.astype(bool) & held).sum()) == reused
    TM.check_birth(vis, born, birth)
    assert np.isnan(res[0]).all()


def test_detect_every_0_never_detects(clip):
    got, _ = TM.pushes(clip["frames"][:3], 10, 0, pyramids=clip["pyr"][:3], **clip["kw"])
    assert not got[1].any() and not got[2].any() and not got[3].any() and np.isnan(got[0]).all() and np.isnan(got[4]).all()


def add_points_scenario(frames, pyr=None):
    """The add_points scenario shared with the GPU test: K = 24, D = 0; the 24 features of frame 0 after push 0 and 12
    features of frame 3 after push 3.  Returns the two point lists, the queries (t, x, y) that
    the sparse-tracks statement takes for them -- the 24, then those of the 12 that find a dead slot -- their slots, and
    the statement's rows per slot (T, K, 2), (T, K)."""
    K, t2 = ADD["K"], ADD["t_second"]
    T = frames.shape[0]
    pyr = pyr if pyr is not None else [S.pyramid(f, 3) for f in frames]
    n0, first, _ = FM.select(FM.score(frames[0], 5), 0.05, 4.0, K)
    n3, second, _ = FM.select(FM.score(frames[t2], 5), 0.05, 4.0, ADD["n_second"])
    assert n0 == K and n3 == ADD["n_second"]
    tr0, vis0 = S.track(frames, np.zeros(K, np.int64), first, 3, 5, 3, pyramids=pyr)
    dead = np.flatnonzero(vis0[t2] == 0)
    started = min(len(dead), n3)
    slots = dead[:started]
    tr3, vis3 = S.track(frames, np.full(started, t2, np.int64), second[:started], 3, 5, 3, pyramids=pyr)
    want_tr, want_vis = tr0.copy(), vis0.copy()
    want_tr[t2:, slots], want_vis[t2:, slots] = tr3[t2:], vis3[t2:]
    qt = np.concatenate([np.zeros(K, np.int32), np.full(started, t2, np.int32)])
    qxy = np.concatenate([first, second[:started]]).astype(np.float32)
    assert T > t2 + 1
    return dict(first=first, second=second, qt=qt, qxy=qxy, slots=slots, alive=vis0.sum(1), want=(want_tr, want_vis))


def test_add_points_start_tracks_in_the_dead_slots(clip):
    frames, pyr = clip["frames"], clip["pyr"]
    sc = add_points_scenario(frames, pyr)
    assert sc["alive"][:4].tolist() == [24, 18, 17, 15]
    assert sc["slots"].tolist() == ADD["slots"] and len(sc["slots"]) == 9, "9 of the 12 points start, 3 are dropped"
    tm = TM.Tracker(ADD["K"], 0)
    rows = []
    for t, f in enumerate(frames):
        tm.push(f, pyr[t])
        if t == 0:
            assert tm.add_points(sc["first"]).tolist() == list(range(ADD["K"]))
        if t == ADD["t_second"]:
            assert tm.add_points(sc["second"]).tolist() == ADD["slots"]
        rows.append(tm.row())
    xy, vis, born, birth, res, det = (np.stack([r[j] for r in rows]) for j in range(6))
    M.same((xy, vis), sc["want"], "every slot's rows are sparse_model.track of its queries")
    assert not det.any()
    want_born = np.zeros_like(born)
    want_born[0], want_born[ADD["t_second"], ADD["slots"]] = 1, 1
    assert np.array_equal(born, want_born)
    TM.check_birth(vis, born, birth)


def test_add_points_drops_points_outside_the_frame(clip):
    tm = TM.Tracker(6, 0)
    tm.push(clip["frames"][0], clip["pyr"][0])
    pts = [(np.nan, 3), (5, 6), (-0.5, 3), (51, 39), (51.5, 3), (3, 39.25), (np.inf, 1), (-0.0, 0.0)]
    assert tm.add_points(pts).tolist() == [0, 1, 2]
    xy, vis = tm.row()[:2]
    assert vis.tolist() == [1, 1, 1, 0, 0, 0] and xy[:3].tolist() == [[5, 6], [51, 39], [0, 0]] and not np.signbit(xy[2]).any()
    assert tm.add_points(np.tile(np.float32([[7, 7]]), (9, 1))).tolist() == [3, 4, 5], "no more than the dead slots"
    assert tm.add_points([(1, 1)]).size == 0


# ---------------------------------------------------------------------------------------------------------------
# the ABI and its refusals, before any device call
# ---------------------------------------------------------------------------------------------------------------
def _create(H=24, W=32, u8=0, L=3, w=5, it=3, alpha=0.01, beta=0.5, mr=4.0, q=0.01, md=3.0, K=8, D=2, null=False, device=0):
    """(code, handle) of oflk_tracker_create"""
    import _oflk

    h = ctypes.c_void_p()
    rc = _oflk.lib().oflk_tracker_create(None if null else ctypes.byref(h), device, H, W, u8, L, w, it, alpha, beta, mr, q, md, K, D)
    return rc, h


REFUSALS = [
    (dict(w=4), UNSUPPORTED), (dict(w=13), UNSUPPORTED), (dict(w=1), UNSUPPORTED), (dict(H=7, W=9), UNSUPPORTED),
    (dict(H=1, W=40, L=1), UNSUPPORTED), (dict(H=0), INVALID), (dict(W=-2), INVALID), (dict(H=1 << 23, W=4), UNSUPPORTED),
    (dict(H=1 << 15, W=1 << 14), UNSUPPORTED),   # 2^29 pixels: oflk_plan_create's bound, which the sequence call meets there
    (dict(it=0), INVALID), (dict(L=0), INVALID), (dict(L=17), INVALID), (dict(alpha=-1.0), INVALID), (dict(beta=float("nan")), INVALID),
    (dict(alpha=float("inf")), INVALID), (dict(mr=-0.5), INVALID), (dict(mr=float("nan")), INVALID), (dict(q=2.0), INVALID),
    (dict(q=float("nan")), INVALID), (dict(md=-1.0), INVALID), (dict(md=float("inf")), INVALID), (dict(K=0), INVALID),
    (dict(K=-3), INVALID), (dict(D=-1), INVALID), (dict(null=True), INVALID), (dict(device=-1), INVALID),
]


def test_symbols_and_signatures_exist():
    import _oflk
    import lucas_kanade_pyramidal as P

    for name in SYMBOLS:
        assert hasattr(_oflk.lib(), name) and name in _oflk.SIGNATURES, name
    assert callable(_oflk.Tracker) and callable(P.SparseKltTracker)
    assert P.TrackerRow._fields == ("xy", "visible", "born", "birth", "residual", "detected")


@pytest.mark.parametrize("u8", [0, 1], ids=["f32", "u8"])
@pytest.mark.parametrize("kw,code", REFUSALS, ids=lambda v: str(v))
def test_create_refuses_without_a_device(kw, code, u8):
    import _oflk

    rc, h = _create(u8=u8, **kw)
    assert rc == code and not h.value
    assert _oflk.lib().oflk_last_error()
    if "D" in kw:
        assert b"detect_every" in _oflk.lib().oflk_last_error()


@pytest.mark.parametrize("D", [0, 1, 2 ** 31 - 1])
def test_a_tracker_refuses_its_row_before_the_first_push(D):
    """creation makes no device call, so a tracker exists on a machine without a GPU; what needs a pushed frame is refused
    there, before any device call"""
    import _oflk

    L = _oflk.lib()
    rc, h = _create(D=D)
    assert rc == 0 and h.value
    try:
        assert L.oflk_tracker_frame_index(h) == -1 and L.oflk_tracker_workspace_bytes(h) == 0
        out = [ctypes.c_void_p(7) for _ in range(6)]
        assert L.oflk_tracker_row_device(h, *[ctypes.byref(p) for p in out]) == INVALID and b"pushed" in L.oflk_last_error()
        assert all(p.value == 7 for p in out)
        assert L.oflk_tracker_read_row(h, None, None, None, None, None, None, None) == INVALID
        pts = np.float32([[3, 4], [5, 6]])
        assert L.oflk_tracker_add_points(h, _oflk.ptr(pts), 2, None) == INVALID and b"pushed" in L.oflk_last_error()
        assert L.oflk_tracker_reset(h, None) == 0 and L.oflk_tracker_frame_index(h) == -1
        # a NULL frame is refused whatever the machine
        assert L.oflk_tracker_push_device(h, None, None) == INVALID
        assert L.oflk_tracker_push(h, None, None, None, None, None, None, None) == INVALID
        assert L.oflk_tracker_frame_index(h) == -1
    finally:
        assert L.oflk_tracker_destroy(h) == 0


def test_a_null_tracker_is_refused_everywhere():
    import _oflk

    L = _oflk.lib()
    frame = np.zeros((24, 32), np.float32)
    pts = np.float32([[3, 4]])
    assert L.oflk_tracker_push_device(None, frame.ctypes.data, None) == INVALID
    assert L.oflk_tracker_push(None, frame.ctypes.data, None, None, None, None, None, None) == INVALID
    assert L.oflk_tracker_row_device(None, None, None, None, None, None, None) == INVALID
    assert L.oflk_tracker_read_row(None, None, None, None, None, None, None, None) == INVALID
    assert L.oflk_tracker_add_points(None, _oflk.ptr(pts), 1, None) == INVALID
    assert L.oflk_tracker_reset(None, None) == INVALID
    assert L.oflk_tracker_destroy(None) == 0 and L.oflk_tracker_frame_index(None) == -1 and L.oflk_tracker_workspace_bytes(None) == 0


def test_shims_raise_value_error_before_any_library_call(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    def no_library():
        raise AssertionError("the argument checks come before any library call")

    created = []
    real = _oflk.lib
    monkeypatch.setattr(_oflk, "lib", no_library)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="detect_every"):
            P.SparseKltTracker((24, 32), 10, bad)
    for kw in (dict(num_levels=0), dict(num_iterations=0), dict(window_size=4), dict(window_size=13), dict(window_size=1),
               dict(max_residual=-1.0), dict(max_residual=float("nan")), dict(alpha=-0.1), dict(beta=float("inf")),
               dict(quality_level=1.5), dict(min_distance=-1.0), dict(min_distance=float("inf")), dict(dtype=np.float64),
               dict(dtype=np.int8)):
        with pytest.raises(ValueError):
            P.SparseKltTracker((24, 32), 10, 2, **kw)
    for K in (0, -1, 2.5):
        with pytest.raises(ValueError):
            P.SparseKltTracker((24, 32), K)
    for shape in ((7, 9), (24,), (24, 32, 3), (0, 32)):   # 7 x 9 at 3 levels: a level of width 1
        with pytest.raises(ValueError):
            P.SparseKltTracker(shape, 10)
    monkeypatch.setattr(_oflk, "lib", real)
    # a tracker is created without a device; its frame and point checks raise before the library is called
    with P.SparseKltTracker((24, 32), 10, 0, dtype=np.float32) as tr:
        created.append(tr)
        assert tr.frame_index == -1 and tr.detect_every == 0 and tr.shape == (24, 32)
        monkeypatch.setattr(_oflk, "lib", no_library)
        with pytest.raises(ValueError, match="shape"):
            tr.push(np.zeros((24, 33), np.float32))
        for pts in (np.zeros((3, 3), np.float32), np.zeros(4, np.float32)):
            with pytest.raises(ValueError, match="points"):
                tr.add_points(pts)
        monkeypatch.setattr(_oflk, "lib", real)
        with pytest.raises(ValueError, match="pushed"):
            tr.read_row()
        with pytest.raises(ValueError, match="pushed"):
            tr.row_device()
        with pytest.raises(ValueError, match="pushed"):
            tr.add_points([(1.0, 2.0)])
        with pytest.raises(ValueError):
            tr.add_points(np.zeros((0, 2), np.float32))   # n < 1
    assert not created[0]._t._h
