"""GPU tests of the online sparse KLT tracker (run on an MI355X: python -m pytest tests/test_gpu_tracker.py -m gpu -q).

The rows of T pushes must equal rows 0 .. T-1 of oflk_pyramidal_sequence_klt_sparse_replenish[_u8] on those frames followed
by one more, and the tracks of add_points those of oflk_pyramidal_sequence_sparse_tracks, byte for byte (NaN bit patterns
normalised).  No tolerance anywhere.

The pyramid: at the library's scale of 0.5 every step of every admissible frame takes the fused kernel
(tests/test_stages_cpu.py::test_ratio_two_is_always_staged_and_fused sweeps the sizes), so there is no shape on which a
tracker could run the unfused chain, and a tracker refuses one at creation.  Both shapes here are asserted fused.
"""
import numpy as np
import pytest

import sparse_model as S
import sparse_replenish_model as M
import tracker_model as TM
from test_gpu_sparse_replenish import _call
from test_sparse_cpu import _drifting
from test_tracker_cpu import ADD, CLIP, add_points_scenario

pytestmark = pytest.mark.gpu

_clip = {}


def _frames(u8):
    """the CPU test's clip (8 frames of 40 x 52); uint8: rounded"""
    if not _clip:
        f = _drifting(CLIP["T"], CLIP["H"], CLIP["W"], CLIP["seed"])
        _clip[False], _clip[True] = f, np.rint(f).astype(np.uint8)
    return _clip[u8]


def _tracker(frames, K, D, q=CLIP["q"], md=CLIP["md"], levels=3, win=5, iters=3, **kw):
    import _oflk

    return _oflk.Tracker(0, frames.shape[1], frames.shape[2], frames.dtype == np.uint8, K, D, levels, win, iters,
                         quality_level=q, min_distance=md, **kw)


def _stack(rows):
    """rows as read_row gives them -> ((tracks, visible, born, detected, residual) in the sequence call's order, birth)"""
    xy, vis, born, birth, res = (np.stack([r[j] for r in rows]) for j in range(5))
    return (xy, vis, born, np.array([r[5] for r in rows], np.int32), res), birth


def _push_all(tr, frames):
    return _stack([tr.push(np.ascontiguousarray(f)) for f in frames])


def _all_fused(H, W, levels):
    import _oflk

    d = S.O.pyramid_dims(H, W, levels)
    return all(_oflk.lib().oflk_pyramid_step_fused(*d[l + 1], *d[l], 8) for l in range(levels - 1))


# ---------------------------------------------------------------------------------------------------------------
# pushes against the sequence call
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [3, 5, 11])
@pytest.mark.parametrize("D", [1, 2, 3, 100])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_pushes_equal_the_rows_of_the_sequence_call(u8, D, win):
    frames = _frames(u8)
    K = CLIP["K"]
    want = _call(frames, K, D, CLIP["q"], CLIP["md"], win=win)
    tr = _tracker(frames, K, D, win=win)
    try:
        got, birth = _push_all(tr, frames[:7])
        assert tr.frame_index == 6
    finally:
        tr.close()
    M.same(got, tuple(a[:7] for a in want), f"u8={u8} D={D} window {win}")
    TM.check_birth(got[1], got[2], birth)
    assert got[3][0] > 0 and (got[3][6] > 0) == (D < 100), "frame 6 detects when it is pushed, unless D = 100"
    if D < 100:
        assert got[2][1:].any(), "ended tracks should be replaced on this clip"


def test_pushes_equal_the_model():
    frames = _frames(False)
    want, wbirth = TM.pushes(frames[:7], CLIP["K"], 2, quality_level=CLIP["q"], min_distance=CLIP["md"])
    tr = _tracker(frames, CLIP["K"], 2)
    try:
        got, birth = _push_all(tr, frames[:7])
    finally:
        tr.close()
    M.same(got, want, "tracker_model")
    v = got[1] != 0
    assert np.array_equal(birth[v], wbirth[v])


@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_an_odd_width_at_two_and_three_levels(u8, levels):
    """W % 4 != 0 and odd level sizes: the pyramid and the samples take the element-wise loads, and a frame's ring slot and
    pyramid slot start at odd offsets"""
    H, W = 41, 53
    assert _all_fused(CLIP["H"], CLIP["W"], 3) and _all_fused(H, W, levels)
    f = _drifting(6, H, W, 7)
    frames = np.rint(f).astype(np.uint8) if u8 else f
    want = _call(frames, 30, 2, 0.05, 4.0, levels=levels)
    tr = _tracker(frames, 30, 2, q=0.05, md=4.0, levels=levels)
    try:
        got, birth = _push_all(tr, frames[:5])
    finally:
        tr.close()
    M.same(got, tuple(a[:5] for a in want), f"41 x 53, {levels} levels, u8={u8}")
    assert got[3][4] > 0


# ---------------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------------
class _DevicePtr:
    """a device address as something torch.as_tensor reads"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


def _from_device(ptr, shape, typestr):
    import torch

    return torch.as_tensor(_DevicePtr(ptr, shape, typestr), device="cuda:0").cpu().numpy()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_push_device_on_a_side_stream_equals_push(u8):
    import torch

    frames = _frames(u8)
    K = CLIP["K"]
    host = _tracker(frames, K, 2)
    dev = _tracker(frames, K, 2)
    side = torch.cuda.Stream()
    try:
        want, wbirth = _push_all(host, frames[:5])
        d_frames = torch.from_numpy(frames[:5]).to("cuda:0")
        torch.cuda.synchronize()
        rows = []
        for t in range(5):
            dev.push_device(d_frames[t].data_ptr(), side.cuda_stream)
            row = dev.read_row(side.cuda_stream)
            p = dev.row_device()
            held = (_from_device(p[0], (K, 2), "<f4"), _from_device(p[1], (K,), "|u1"), _from_device(p[2], (K,), "|u1"),
                    _from_device(p[3], (K,), "<i4"), _from_device(p[4], (K,), "<f4"), int(_from_device(p[5], (1,), "<i4")[0]))
            M.same((held[0], held[1], held[2], np.int32([held[5]]), held[4]), (row[0], row[1], row[2], np.int32([row[5]]), row[4]),
                   f"row_device on frame {t}")
            assert np.array_equal(held[3], row[3])
            rows.append(row)
        got, birth = _stack(rows)
        M.same(got, want, "push_device + read_row against push")
        v = got[1] != 0
        assert np.array_equal(birth[v], wbirth[v])
    finally:
        host.close()
        dev.close()


def test_reset_two_trackers_at_once_and_a_constant_workspace():
    frames, other = _frames(False), _frames(True)
    K = CLIP["K"]
    a, b = _tracker(frames, K, 2), _tracker(other, 25, 3, md=6.0)
    try:
        assert a.workspace_bytes == 0
        rows_a, rows_b, ws = [], [], {}
        for t in range(7):   # interleaved: neither disturbs the other
            rows_a.append(a.push(frames[t]))
            rows_b.append(b.push(other[t]))
            ws[t] = (a.workspace_bytes, b.workspace_bytes)
        assert ws[1] == ws[6] and ws[1][0] > 0, "nothing is allocated after the first push"
        first, _ = _stack(rows_a)
        M.same(first, tuple(x[:7] for x in _call(frames, K, 2, CLIP["q"], CLIP["md"])), "tracker a, interleaved")
        M.same(_stack(rows_b)[0], tuple(x[:7] for x in _call(other, 25, 3, CLIP["q"], 6.0)), "tracker b, interleaved")
        a.reset()
        assert a.frame_index == -1
        with pytest.raises(ValueError, match="pushed"):
            a.read_row()
        again, _ = _push_all(a, frames[:7])
        M.same(again, first, "the same pushes after reset")
        assert a.workspace_bytes == ws[6][0]
    finally:
        a.close()
        b.close()


def test_a_destroyed_tracker_leaves_the_plan_calls_working():
    frames = _frames(False)
    before = _call(frames, 20, 2, CLIP["q"], CLIP["md"])
    tr = _tracker(frames, 20, 2)
    tr.push(frames[0])
    tr.close()
    M.same(_call(frames, 20, 2, CLIP["q"], CLIP["md"]), before, "the sequence call after a tracker came and went")


def test_python_tracker():
    import lucas_kanade_pyramidal as P

    frames = _frames(True)
    want = _call(frames, CLIP["K"], 2, CLIP["q"], CLIP["md"])
    with P.SparseKltTracker(frames.shape[1:], CLIP["K"], 2, CLIP["q"], CLIP["md"]) as tr:
        rows = [tr.push(f) for f in frames[:7]]
        assert tr.frame_index == 6
    assert rows[0].visible.dtype == bool and rows[0].born.dtype == bool and isinstance(rows[0].detected, int)
    got = (np.stack([r.xy for r in rows]), np.stack([r.visible for r in rows]), np.stack([r.born for r in rows]),
           np.int32([r.detected for r in rows]), np.stack([r.residual for r in rows]))
    M.same(got, tuple(a[:7] for a in want), "SparseKltTracker")
    TM.check_birth(got[1], got[2], np.stack([r.birth for r in rows]))


# ---------------------------------------------------------------------------------------------------------------
# add_points
# ---------------------------------------------------------------------------------------------------------------
def _sparse_tracks(frames, qt, qxy):
    import _oflk

    T, H, W = frames.shape
    N = len(qxy)
    tr, vis = np.full((T, N, 2), -7.0, np.float32), np.full((T, N), 9, np.uint8)
    qt, qxy = np.ascontiguousarray(qt, np.int32), np.ascontiguousarray(qxy, np.float32)
    _oflk.check(_oflk.lib().oflk_pyramidal_sequence_sparse_tracks(_oflk.ptr(frames), T, H, W, 3, 5, 3, 0.01, 0.5, 4.0,
                                                                  qt.ctypes.data_as(_oflk._i32p), _oflk.ptr(qxy), N, _oflk.ptr(tr),
                                                                  vis.ctypes.data))
    return tr, vis


def test_add_points_equal_the_sparse_tracks_of_their_queries():
    frames = _frames(False)
    K, t2 = ADD["K"], ADD["t_second"]
    sc = add_points_scenario(frames)
    qtr, qvis = _sparse_tracks(frames, sc["qt"], sc["qxy"])
    want_tr, want_vis = qtr[:, :K].copy(), qvis[:, :K].copy()
    want_tr[t2:, sc["slots"]], want_vis[t2:, sc["slots"]] = qtr[t2:, K:], qvis[t2:, K:]
    assert sc["slots"].tolist() == ADD["slots"]
    tr = _tracker(frames, K, 0)
    rows = []
    try:
        for t, f in enumerate(frames):
            row = tr.push(f)
            assert row[5] == 0 and not row[2].any(), "D = 0 never detects"
            if t == 0:   # NaN points and points outside the frame take no slot
                junk = np.float32([[np.nan, 3], [-1, 3], [52, 3], [3, 40], [np.inf, 1]])
                tr.add_points(np.concatenate([junk[:2], sc["first"][:10], junk[2:], sc["first"][10:]]))
                row = tr.read_row()
            if t == t2:   # 12 points for 9 dead slots: three are dropped
                tr.add_points(sc["second"])
                row = tr.read_row()
            rows.append(row)
    finally:
        tr.close()
    got, birth = _stack(rows)
    M.same(got[:2], (want_tr, want_vis), "tracks of add_points against oflk_pyramidal_sequence_sparse_tracks")
    M.same(got[:2], sc["want"], "... and against sparse_model.track")
    want_born = np.zeros_like(got[2])
    want_born[0], want_born[t2, sc["slots"]] = 1, 1
    assert np.array_equal(got[2], want_born) and not got[3].any()
    TM.check_birth(got[1], got[2], birth)


def test_added_points_seed_later_detections():
    """with D > 0 an added point is an ordinary track: the model with the same calls gives the same rows"""
    frames = _frames(False)
    pts = np.float32([[20, 20], [30.5, 12.25], [-0.0, 0.0], [51, 39]])
    model = TM.Tracker(CLIP["K"], 2, CLIP["q"], CLIP["md"])
    tr = _tracker(frames, CLIP["K"], 2)
    want, rows = [], []
    try:
        for t, f in enumerate(frames[:5]):
            model.push(f)
            tr.push(f)
            if t == 1:
                model.add_points(pts)
                tr.add_points(pts)
            want.append(model.row())
            rows.append(tr.read_row())
    finally:
        tr.close()
    got, birth = _stack(rows)
    exp, ebirth = _stack(want)
    M.same(got, exp, "add_points between detections")
    v = got[1] != 0
    assert np.array_equal(birth[v], ebirth[v])
    assert got[2][1].sum() == 4 and got[3][1] == 0, "the four points start on frame 1, which does not detect"
    assert got[3][2] > 0, "frame 2 detects around them"
