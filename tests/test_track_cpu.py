"""CPU tests of the point-track statement (tests/track_model.py), of the track entry points' argument checks and of the new
C ABI surface.  Nothing here touches a device."""
import re
from pathlib import Path

import numpy as np
import pytest

import fb_model as FM
import track_model as M

ROOT = Path(__file__).resolve().parents[1]
TRACK_SYMBOLS = ["oflk_track_points", "oflk_track_points_host", "oflk_pyramidal_sequence_tracks",
                 "oflk_pyramidal_sequence_tracks_u8"]
NAN_ROW = np.array([np.nan, np.nan], np.float32)


def _const(B, H, W, *vals):
    return tuple(np.full((B, H, W), v, np.float32) for v in vals)


@pytest.mark.parametrize("F", [(1.25, -0.5), (-2.0, 0.75), (0.5, 1.5), (3.0, 0.0)])
def test_opposite_constant_flows_move_by_whole_steps_until_they_leave(F):
    """F constant and dyadic, G = -F: every step is exact (e2 = 0) and the track is p + t*F until the step whose target
    leaves the frame; that row and every later one are NaN / 0"""
    B, H, W = 12, 17, 23
    dx, dy = F
    flows = _const(B, H, W, dx, dy, -dx, -dy)
    q = np.array([[11.0, 8.0], [0.0, 0.0], [22.0, 16.0], [3.5, 12.25], [W - 1.0, 0.0]], np.float32)
    tr, vis = M.track(*flows, None, q)
    for n, (x, y) in enumerate(q.astype(np.float64)):
        end = B + 1
        for t in range(1, B + 1):
            px, py = x + t * dx, y + t * dy
            if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
                end = t
                break
        for t in range(B + 1):
            if t < end:
                assert vis[t, n] == 1 and np.array_equal(tr[t, n], np.float32([x + t * dx, y + t * dy])), (n, t, tr[t, n])
            else:
                assert vis[t, n] == 0 and np.isnan(tr[t, n]).all(), (n, t)


def test_large_forward_flow_with_zero_backward_ends_at_the_first_failing_step():
    """G = 0: e2 = m2 = |F|^2, so a step passes while e2 <= alpha*m2 + beta (float32); |F| grows by 0.25 px per pair"""
    B, H, W = 8, 40, 60
    alpha, beta = 0.01, 0.5
    steps = [0.25 * (t + 1) for t in range(B)]
    uf = np.stack([np.full((H, W), s, np.float32) for s in steps])
    z = np.zeros_like(uf)
    tr, vis = M.track(uf, z, z, z, None, np.array([[5.0, 20.0]], np.float32), alpha, beta)
    first_fail = next(t for t, s in enumerate(steps)
                      if not np.float32(s) * np.float32(s) <= np.float32(alpha) * (np.float32(s) * np.float32(s)) + np.float32(beta))
    assert first_fail == 2
    assert vis[:first_fail + 1, 0].all() and not vis[first_fail + 1:, 0].any()
    assert tr[first_fail, 0, 0] == np.float32(5.0 + sum(steps[:first_fail]))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (9, 13)])
def test_last_row_and_column_stay_inside(H, W):
    """zero flows: queries on the last row / column and at x = W-1 exactly stay visible where they are (closed interval);
    a step landing exactly on W-1 stays inside, one landing 2^-18 beyond it ends the track"""
    B = 4
    z = _const(B, H, W, 0, 0, 0, 0)
    q = np.array([[W - 1.0, H - 1.0], [W - 1.0, 0.0], [0.0, H - 1.0], [0.0, 0.0]], np.float32)
    tr, vis = M.track(*z, None, q)
    assert vis.all() and np.array_equal(tr, np.broadcast_to(q, tr.shape))
    if W > 1:
        for off, want in ((0.0, True), (2.0 ** -18, False)):
            uf = np.full((B, H, W), 0.5 + off, np.float32)
            tr, vis = M.track(uf, z[1], -uf, z[3], None, np.array([[W - 1.5, 0.0]], np.float32), 1e6, 1e6)
            assert bool(vis[1, 0]) == want, off
            if want:
                assert tr[1, 0, 0] == np.float32(W - 1) and not vis[2:, 0].any()   # the next step leaves


def test_rows_before_the_query_and_queries_outside_are_nan():
    B, H, W = 5, 10, 12
    z = _const(B, H, W, 0, 0, 0, 0)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    qt = np.array([2, 0, 0, 1, 3, 0, 5, 0], np.int64)
    q = np.array([[3, 4], [-0.5, 2], [W - 1 + 2.0 ** -18, 2], [nan, 1], [2, inf], [2, -1e-30], [1, 1], [-0.0, -0.0]],
                 np.float32)
    tr, vis = M.track(*z, qt, q)
    assert not vis[:2, 0].any() and np.isnan(tr[:2, 0]).all() and vis[2:, 0].all()
    for n in (1, 2, 3, 4, 5):
        assert not vis[:, n].any() and np.isnan(tr[:, n]).all(), n
    assert not vis[:5, 6].any() and vis[5, 6] and np.array_equal(tr[5, 6], [1, 1])
    assert vis[:, 7].all() and (tr[:, 7].view(np.int32) == 0).all()   # -0 reads as +0


def test_first_step_at_integer_queries_is_the_fb_check():
    """at pixel queries, step 1 samples the flows at the pixel itself: visible[1] is fb_check's valid_f and tracks[1] is
    f32(x + uf)"""
    B, H, W = 1, 33, 41
    flows = M.smooth_flows(B, H, W, seed=4, scale=4.0)
    _, _, valid_f, _ = FM.fb_check(*flows)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float32)
    tr, vis = M.track(*flows, None, q)
    assert np.array_equal(vis[1], valid_f[0].ravel())
    assert 0.2 < vis[1].mean() < 0.95   # both outcomes occur
    ok = vis[1] == 1
    want = np.stack([(xx.ravel() + flows[0][0].ravel().astype(np.float64)).astype(np.float32),
                     (yy.ravel() + flows[1][0].ravel().astype(np.float64)).astype(np.float32)], 1)
    assert np.array_equal(tr[1][ok], want[ok])


@pytest.mark.parametrize("cut", [1, 3, 5])
def test_chunks_continue_from_the_last_row(cut):
    B, H, W = 8, 30, 40
    flows = M.smooth_flows(B, H, W, seed=7, scale=2.0)
    rng = np.random.default_rng(1)
    N = 400
    qt = rng.integers(0, B + 1, N)
    q = (rng.random((N, 2)) * [W - 1, H - 1]).astype(np.float32)
    tr, vis = M.track(*flows, qt, q)
    a_tr, a_vis = M.track(*(f[:cut] for f in flows), qt, q)
    b_tr, b_vis = M.track(*(f[cut:] for f in flows), qt, q, t0=cut, prev=(a_tr[-1], a_vis[-1]))
    got_tr, got_vis = np.concatenate([a_tr, b_tr[1:]]), np.concatenate([a_vis, b_vis[1:]])
    assert np.array_equal(got_vis, vis)
    assert np.array_equal(got_tr, tr, equal_nan=True)
    assert np.array_equal(b_tr[0], a_tr[-1], equal_nan=True)   # row 0 rewritten for qt == cut is the same row
    assert 0.1 < vis[-1].mean() < 0.9


def test_sample_is_the_oracles_warp_at_grid_points():
    """the statement's sampler equals the oracle's warp_image wherever warp_image can express the point"""
    import oflk_oracle as O

    H, W = 21, 26
    img = np.random.default_rng(2).random((H, W)).astype(np.float32) * 255
    uf, vf, _, _ = M.smooth_flows(1, H, W, seed=3, scale=3.0)
    want = O.warp_image(img, uf[0], vf[0])
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    got = M.sample(img, (xx + uf[0].astype(np.float64)).ravel(), (yy + vf[0].astype(np.float64)).ravel()).reshape(H, W)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_scene_meaning_on_the_oracle_flows():
    """the occluder scene's tracks on the CPU oracle's flows show what tests/test_gpu_tracks.py asks of the GPU's"""
    import oflk_oracle as O

    T, S = 5, M.SCENE
    frames, corners = FM.occluder_scene(T, S["H"], S["W"], S["size"], S["step"])
    fl = [[], [], [], []]
    for t in range(T - 1):
        for lst, a in zip(fl, O.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3) +
                          O.lucas_kanade_pyramidal(frames[t + 1], frames[t], 3, 5, 3)):
            lst.append(a)
    flows = [np.stack(x) for x in fl]

    def run(q):
        tr, vis = M.track(*flows, q[:, 0].astype(np.int64), q[:, 1:])
        return tr, vis.astype(bool)

    M.check_scene_tracks(run, T, corners, S["H"], S["W"], S["size"], S["step"])


# ---- the entry points' checks, before any device call -------------------------------------------------------------------
def test_host_forms_reject_bad_arguments():
    import _oflk

    L = _oflk.lib()
    INV = _oflk.OFLK_ERR_INVALID
    B, H, W, N = 2, 16, 16, 4
    fl = [np.zeros((B, H, W), np.float32) for _ in range(4)]
    frames = np.zeros((B + 1, H, W), np.float32)
    q = np.zeros((N, 2), np.float32)
    qt = np.zeros(N, np.int32)
    tr = np.empty((B + 1, N, 2), np.float32)
    vis = np.empty((B + 1, N), np.uint8)
    i32 = lambda a: a.ctypes.data_as(_oflk._i32p)  # noqa: E731
    P = _oflk.ptr

    def host(**kw):
        a = dict(fl=[P(x) for x in fl], B=B, alpha=0.01, beta=0.5, qt=i32(qt), q=P(q), N=N, tr=P(tr), vis=vis.ctypes.data)
        a.update(kw)
        return L.oflk_track_points_host(*a["fl"], a["B"], H, W, a["alpha"], a["beta"], a["qt"], a["q"], a["N"], a["tr"], a["vis"])

    def seq(u8=False, **kw):
        a = dict(f=frames.ctypes.data, T=B + 1, alpha=0.01, beta=0.5, qt=i32(qt), q=P(q), N=N, tr=P(tr), vis=vis.ctypes.data)
        a.update(kw)
        fn = L.oflk_pyramidal_sequence_tracks_u8 if u8 else L.oflk_pyramidal_sequence_tracks
        f = a["f"] if u8 else ctypes_f32(a["f"])
        return fn(f, a["T"], H, W, 3, 5, 3, a["alpha"], a["beta"], a["qt"], a["q"], a["N"], a["tr"], a["vis"])

    for bad in ([-1, 0, 0, 0], [0, 3, 0, 0], [0, 0, 99, 0]):   # query frames outside [0, T-1]
        qt[:] = bad
        assert host() == INV and seq() == INV and seq(True) == INV
    qt[:] = 0
    for kw in (dict(N=0), dict(N=-3), dict(q=None), dict(tr=None), dict(vis=None), dict(alpha=-0.5), dict(beta=float("nan")),
               dict(alpha=float("inf"))):
        assert host(**kw) == INV, kw
        assert seq(**kw) == INV and seq(True, **kw) == INV, kw
    for T in (1, 0):
        assert seq(T=T) == INV and seq(True, T=T) == INV
    assert seq(f=None) == INV
    assert host(B=0) == INV
    for i in range(4):
        f = [P(x) for x in fl]
        f[i] = None
        assert host(fl=f) == INV
    dev = lambda **kw: L.oflk_track_points(*[P(x) for x in fl], kw.get("B", B), H, W, 0.01, kw.get("beta", 0.5),  # noqa: E731
                                            kw.get("t0", 0), None, kw.get("q", P(q)), kw.get("N", N), kw.get("tr", P(tr)),
                                            vis.ctypes.data, None)
    assert dev(t0=-1) == INV and dev(N=0) == INV and dev(B=0) == INV and dev(q=None) == INV and dev(beta=-1.0) == INV
    assert dev(tr=tr.ctypes.data + 4) == INV   # d_tracks must be 8-byte aligned


def ctypes_f32(addr):
    import ctypes

    return None if addr is None else ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))


def test_python_layer_rejects_bad_input_before_any_device_call(monkeypatch):
    import _oflk
    import flow_metrics
    import lucas_kanade_pyramidal as P

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_oflk, "lib", no_device)
    f = np.zeros((3, 16, 16), np.float32)
    fl = [f[:2]] * 4
    good = np.array([[0, 1.0, 1.0]], np.float32)
    for q in (np.zeros((0, 3)), np.zeros((4,)), np.zeros((2, 4)), [[3, 1.0, 1.0]], [[-1, 1.0, 1.0]], [[0.5, 1.0, 1.0]],
              [[np.nan, 1.0, 1.0]]):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_tracks(f, q)
        with pytest.raises(ValueError):
            flow_metrics.track_points(*fl, q)
    for alpha, beta in ((-0.01, 0.5), (0.01, float("nan"))):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_tracks(f, good, alpha=alpha, beta=beta)
        with pytest.raises(ValueError):
            flow_metrics.track_points(*fl, good, alpha, beta)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_tracks(f[:1], good)
    with pytest.raises(ValueError):
        flow_metrics.track_points(f[:2], f[:2], f[:2], f[:1], good)
    qt, qxy = _oflk.as_queries(np.array([[1, 2.5, 3.5], [0, 0, 0]]), 3)
    assert qt.dtype == np.int32 and list(qt) == [1, 0] and qxy.dtype == np.float32 and qxy.shape == (2, 2)
    qt, qxy = _oflk.as_queries([[2.5, 3.5]], 3)
    assert qt is None and qxy.tolist() == [[2.5, 3.5]]


def test_new_symbols_are_declared_and_exported():
    import _oflk

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oflk.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oflk_[a-z0-9_]+)\s*\(", text))
    L = _oflk.lib()
    for name in TRACK_SYMBOLS:
        assert name in declared, f"{name} not declared in include/oflk.h"
        assert hasattr(L, name), f"{name} not exported by liboflk.so"
        assert name in _oflk.SIGNATURES
