"""GPU tests of the replenished KLT (run on an MI355X: python -m pytest tests/test_gpu_replenish.py -m gpu -q).

oflk_replenish_features (host and device form) must equal replenish_model.detect, and oflk_pyramidal_sequence_klt_replenish
must equal replenish_model.sequence on the flows of oflk_pyramidal_sequence_fb and the scores of oflk_corner_score_host for
the same frames, byte for byte (NaN bit patterns normalised).  With detect_every >= T the call is
oflk_pyramidal_sequence_klt.
"""
import numpy as np
import pytest

import feature_model as FM
import replenish_model as M
from test_gpu_fb import _host_fb, _same
from test_gpu_features import _frame, _plateau
from test_gpu_sequence import _dev, _video
from test_replenish_cpu import MDS, check_invariants

pytestmark = pytest.mark.gpu


def _norm(xy):
    t = np.array(xy, np.float32, copy=True)
    t[np.isnan(t)] = np.float32(np.nan)
    return t


def _garbage(K, seed):
    """qt / qxy with bytes that a detection must leave alone in the slots it does not fill"""
    rng = np.random.default_rng(seed)
    return rng.integers(-5, 1000, K).astype(np.int32), rng.normal(0, 100, (K, 2)).astype(np.float32)


def _state(S, K, md, seed, free, half=False, stacked=0):
    """a slot row as a running call has it: the frame's own corners (so that seeds sit on candidates), moved by up to half a
    pixel; `free` of the K slots dead; `half`: every position at x.5, y.5; `stacked`: that many alive slots on one corner"""
    rng = np.random.default_rng(seed)
    H, W = S.shape
    n, xy, _ = FM.select(S, 0.01, max(md, 2.0) if md < 1e3 else 10.0, K)
    xy = xy.copy()
    xy[n:] = (rng.random((K - n, 2)) * [W - 1, H - 1]).astype(np.float32)
    if half:
        xy = np.minimum(np.floor(xy) + np.float32(0.5), np.float32([W - 1.5, H - 1.5])).astype(np.float32)
    else:
        xy = np.clip(xy + rng.uniform(-0.5, 0.5, (K, 2)), 0, [W - 1, H - 1]).astype(np.float32)
    if stacked:
        xy[:stacked] = xy[0]
    vis = np.ones(K, bool)
    dead = rng.permutation(np.arange(stacked, K))[:free] if free < K else np.arange(K)
    vis[dead] = False
    xy[~vis] = np.nan
    return xy, vis


def _want(S, xy, vis, q, md, t, qt, qxy):
    return M.apply(*M.detect(S, xy, vis, q, md), t, qt, qxy)


def _same_detection(got, want, what):
    _same(np.asarray(got[0], np.int32), want[0], f"{what}: qt")
    _same(_norm(got[1]), _norm(want[1]), f"{what}: qxy")
    _same(np.asarray(got[2], np.uint8), want[2], f"{what}: born")
    assert int(got[3]) == int(want[3]), f"{what}: detected {int(got[3])} != {int(want[3])}"


def _host_form(frame, xy, vis, q, md, win, t, qt, qxy):
    import lucas_kanade_core as LK

    return LK.replenish_features(frame, xy, vis, None, q, md, win, t, qt, qxy)


class _DeviceForm:
    """the buffers of oflk_replenish_features for one shape; run() uploads a state into them and enqueues one detection"""

    def __init__(self, H, W, K, md, win, u8):
        import torch

        import _oflk

        dev = torch.device("cuda", 0)
        self.H, self.W, self.K, self.md, self.win, self.u8 = H, W, K, md, win, u8
        self.nbytes = _oflk.replenish_features_workspace(H, W, win, md, K)
        self.ws = torch.full((self.nbytes,), 0xA5, dtype=torch.uint8, device=dev)   # garbage: no zeroed workspace is needed
        self.frame = torch.empty((H, W), dtype=torch.uint8 if u8 else torch.float32, device=dev)
        self.xy = torch.empty((K, 2), dtype=torch.float32, device=dev)
        self.vis = torch.empty((K,), dtype=torch.uint8, device=dev)
        self.qt = torch.empty((K,), dtype=torch.int32, device=dev)
        self.qxy = torch.empty((K, 2), dtype=torch.float32, device=dev)
        self.born = torch.full((K,), 7, dtype=torch.uint8, device=dev)
        self.det = torch.full((1,), -1, dtype=torch.int32, device=dev)

    def load(self, frame, xy, vis, qt, qxy):
        import torch

        for dst, src in ((self.frame, frame), (self.xy, xy), (self.vis, np.asarray(vis, np.uint8)), (self.qt, qt), (self.qxy, qxy)):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        self.born.fill_(7)
        self.det.fill_(-1)

    def enqueue(self, q, t, stream):
        import _oflk

        _oflk.replenish_features(self.frame.data_ptr(), self.H, self.W, t, self.xy.data_ptr(), self.vis.data_ptr(),
                                 self.ws.data_ptr(), self.nbytes, self.qt.data_ptr(), self.qxy.data_ptr(), self.born.data_ptr(),
                                 self.det.data_ptr(), self.K, q, self.md, self.win, u8=self.u8, stream=stream)

    def read(self):
        import torch

        torch.cuda.synchronize()
        return self.qt.cpu().numpy(), self.qxy.cpu().numpy(), self.born.cpu().numpy(), int(self.det.cpu().numpy()[0])

    def run(self, frame, xy, vis, q, t, qt, qxy):
        import torch

        self.load(frame, xy, vis, qt, qxy)
        self.enqueue(q, t, torch.cuda.current_stream().cuda_stream)
        return self.read()


# ---------------------------------------------------------------------------------------------------------------
# one detection
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_one_detection_equals_statement(u8):
    """both forms, every min_distance of the CPU tests, budgets 0, 1, some and K, seeds stacked and at rint ties"""
    H, W, K, q = 120, 160, 90, 0.01
    frame = _frame(H, W, seed=31, u8=u8)
    S = FM.score(frame, 5)
    filled = 0
    for md in MDS:
        dev = _DeviceForm(H, W, K, md, 5, u8)
        for i, (free, half, stacked) in enumerate([(0, False, 0), (1, False, 0), (30, False, 0), (K, False, 0), (30, True, 0),
                                                   (30, False, 9), (30, True, 9)]):
            xy, vis = _state(S, K, md, seed=10 * i + 1, free=free, half=half, stacked=stacked)
            qt, qxy = _garbage(K, i)
            want = _want(S, xy, vis, q, md, 4, qt, qxy)
            assert want[3] <= free and (free or want[3] == 0)
            filled += want[3]
            what = f"md={md} free={free} half={half} stacked={stacked}"
            _same_detection(_host_form(frame, xy, vis, q, md, 5, 4, qt, qxy), want, "host form " + what)
            _same_detection(dev.run(frame, xy, vis, q, 4, qt, qxy), want, "device form " + what)
    assert filled > 100, "the cases should fill slots"


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_one_detection_on_every_window(u8):
    H, W, K, q, md = 120, 160, 120, 0.02, 7.0
    frame = _frame(H, W, seed=33, u8=u8)
    for win in FM.WINDOWS:
        S = FM.score(frame, win)
        xy, vis = _state(S, K, md, seed=win, free=40)
        qt, qxy = _garbage(K, win)
        want = _want(S, xy, vis, q, md, 0, qt, qxy)
        assert want[3] > 0
        _same_detection(_host_form(frame, xy, vis, q, md, win, 0, qt, qxy), want, f"host form window {win}")
        _same_detection(_DeviceForm(H, W, K, md, win, u8).run(frame, xy, vis, q, 0, qt, qxy), want, f"device form window {win}")


def _periodic(H, W, seed):
    """a 5 x 5 tile of multiples of 8 repeated over the frame: with the 5 x 5 window every interior pixel sums one whole
    period of exact products, so S is one value on the whole interior and every interior pixel is a candidate"""
    tile = np.random.default_rng(seed).integers(0, 16, (5, 5)) * 8.0
    return np.tile(tile, (H // 5 + 1, W // 5 + 1))[:H, :W].astype(np.float32)


def test_plateau_frames_and_a_frame_without_corners():
    H, W, K = 60, 70, 400
    flat = _periodic(H, W, 3)
    S = FM.score(flat, 5)
    inner = S[3:-3, 3:-3]   # one pixel inside the scored region: its 8 neighbours carry the plateau's value too
    assert inner.min() == inner.max() > 0, "the periodic frame should score one value"
    assert len(FM.candidates(S, 0.0)[0]) >= inner.size, "every such pixel is a candidate"
    for frame in (flat, _plateau(H, W)):
        S = FM.score(frame, 5)
        for md in (0.0, 0.5, 1.0, 1.5, 7.0):
            for free in (0, 150, K):
                xy, vis = _state(S, K, md, seed=int(md * 10) + free, free=free, half=free == 150, stacked=0 if free == K else 6)
                qt, qxy = _garbage(K, free)
                want = _want(S, xy, vis, 0.0, md, 2, qt, qxy)
                _same_detection(_host_form(frame, xy, vis, 0.0, md, 5, 2, qt, qxy), want, f"plateau md={md} free={free}")
                _same_detection(_DeviceForm(H, W, K, md, 5, False).run(frame, xy, vis, 0.0, 2, qt, qxy), want,
                                f"plateau, device form md={md} free={free}")
    # M = 0: nothing detected, nothing written
    zero = np.zeros((H, W), np.float32)
    xy, vis = _state(FM.score(_plateau(H, W), 5), K, 5.0, seed=1, free=200)
    qt, qxy = _garbage(K, 9)
    for got in (_host_form(zero, xy, vis, 0.01, 5.0, 5, 3, qt, qxy), _DeviceForm(H, W, K, 5.0, 5, False).run(zero, xy, vis, 0.01, 3,
                                                                                                            qt, qxy)):
        _same_detection(got, (qt, qxy, np.zeros(K, np.uint8), 0), "a frame without corners")


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_one_detection_at_1080p_with_a_tenth_of_10000_slots_free(u8):
    H, W, K, q, md = 1080, 1920, 10000, 0.01, 10.0
    frame = _frame(H, W, seed=12, u8=u8)
    S = FM.score(frame, 5)
    xy, vis = _state(S, K, md, seed=5, free=K // 10)
    assert vis.sum() == K - K // 10
    qt, qxy = _garbage(K, 1)
    want = _want(S, xy, vis, q, md, 8, qt, qxy)
    print(f"1080p: {len(FM.candidates(S, q)[0])} candidates, {want[3]} of {K // 10} free slots filled")
    _same_detection(_host_form(frame, xy, vis, q, md, 5, 8, qt, qxy), want, "host form")
    _same_detection(_DeviceForm(H, W, K, md, 5, u8).run(frame, xy, vis, q, 8, qt, qxy), want, "device form")
    # everything free and no seeds is the plain selection; md beyond the diagonal: one live slot removes every candidate
    none = np.zeros(K, bool)
    got = _host_form(frame, np.full((K, 2), np.nan, np.float32), none, q, md, 5, 0, qt, qxy)
    n, wxy, _ = FM.select(S, q, md, K)
    assert got[3] == n and got[2][:n].all() and not got[2][n:].any()
    _same(got[1][:n], wxy[:n], "all free: the plain selection")
    one = none.copy()
    one[17] = True
    pos = np.full((K, 2), np.nan, np.float32)
    pos[17] = (3.0, 1070.0)
    for far in (2300.0, 1e9):
        got = _host_form(frame, pos, one, q, far, 5, 0, qt, qxy)
        _same_detection(got, (qt, qxy, np.zeros(K, np.uint8), 0), f"md={far}")
    got = _host_form(frame, pos, one, q, 300.0, 5, 0, qt, qxy)
    _same_detection(got, _want(S, pos, one, q, 300.0, 0, qt, qxy), "md=300")
    assert 0 < got[3] <= 100


def test_device_form_replays_from_a_graph_with_changed_inputs():
    """captured once, replayed on other frames and slot rows in the same buffers (the process keeps the default number of
    hardware queues)"""
    import torch

    H, W, K, q, md = 240, 320, 500, 0.01, 6.0
    dev = _DeviceForm(H, W, K, md, 5, False)
    cases = []
    for i in range(3):
        frame = _frame(H, W, seed=40 + i, u8=False)
        S = FM.score(frame, 5)
        xy, vis = _state(S, K, md, seed=i, free=(120, 0, K)[i], stacked=(5, 0, 0)[i])
        qt, qxy = _garbage(K, 20 + i)
        cases.append((frame, xy, vis, qt, qxy, _want(S, xy, vis, q, md, 6, qt, qxy)))
    _same_detection(dev.run(*cases[0][:3], q, 6, *cases[0][3:5]), cases[0][5], "eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    dev.load(*cases[0][:5])
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        dev.enqueue(q, 6, torch.cuda.current_stream().cuda_stream)
    for rep, i in enumerate((1, 2, 0, 1)):
        dev.load(*cases[i][:5])
        dev.ws.zero_()
        g.replay()
        _same_detection(dev.read(), cases[i][5], f"replay {rep} of case {i}")
    del g


# ---------------------------------------------------------------------------------------------------------------
# the whole call
# ---------------------------------------------------------------------------------------------------------------
def _call(frames, K, D, q, md, levels=3, win=5, iters=3, alpha=0.01, beta=0.5):
    """the C entry point, every output preset with bytes that it must overwrite"""
    import _oflk

    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    tr, vis = np.full((T, K, 2), -7.0, np.float32), np.full((T, K), 9, np.uint8)
    born, det = np.full((T, K), 9, np.uint8), np.full(T, -3, np.int32)
    fn = _oflk.lib().oflk_pyramidal_sequence_klt_replenish_u8 if u8 else _oflk.lib().oflk_pyramidal_sequence_klt_replenish
    f = np.ascontiguousarray(frames)
    _oflk.check(fn(f.ctypes.data if u8 else _oflk.ptr(f), T, H, W, levels, win, iters, alpha, beta, q, md, K, D, _oflk.ptr(tr),
                   vis.ctypes.data, born.ctypes.data, det.ctypes.data_as(_oflk._i32p)))
    return tr, vis, born, det


def _klt(frames, K, q, md, levels=3, win=5, iters=3):
    import _oflk

    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    cnt = np.zeros(1, np.int32)
    xy, sc = np.empty((K, 2), np.float32), np.empty(K, np.float32)
    tr, vis = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    fn = _oflk.lib().oflk_pyramidal_sequence_klt_u8 if u8 else _oflk.lib().oflk_pyramidal_sequence_klt
    f = np.ascontiguousarray(frames)
    _oflk.check(fn(f.ctypes.data if u8 else _oflk.ptr(f), T, H, W, levels, win, iters, 0.01, 0.5, q, md, K,
                   cnt.ctypes.data_as(_oflk._i32p), _oflk.ptr(xy), _oflk.ptr(sc), _oflk.ptr(tr), vis.ctypes.data))
    return int(cnt[0]), tr, vis


def _model(frames, flows, K, D, q, md, win=5):
    import lucas_kanade_core as LK

    return M.sequence(lambda t: LK.corner_min_eigenvalue(frames[t], win), flows, K, D, q, md)


def _same_call(got, want, what):
    _same(_norm(got[0]), _norm(want[0]), f"{what}: tracks")
    for g, w, name in zip(got[1:], want[1:], ("visible", "born", "detected")):
        _same(g, w, f"{what}: {name}")


def _same_as_klt(frames, K, q, md, **kw):
    T = frames.shape[0]
    n, ktr, kvis = _klt(frames, K, q, md, **kw)
    for D in (T, T + 1, 2 ** 31 - 1):
        tr, vis, born, det = _call(frames, K, D, q, md, **kw)
        _same(_norm(tr), _norm(ktr), f"D={D}: tracks of the KLT call")
        _same(vis, kvis, f"D={D}: visible of the KLT call")
        _same(born[0], vis[0], f"D={D}: born on frame 0")
        assert not born[1:].any() and det.tolist() == [n] + [0] * (T - 1)
    return n


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_whole_call_equals_the_model_on_its_own_flows_small(u8):
    frames = _video(11, 120, 160, seed=5, u8=u8)
    K, q, md = 120, 0.01, 6.0
    flows = _host_fb(frames, 3, 5, 3)[0][:4]
    reborn = 0
    for D in (1, 2, 3, 5):
        got = _call(frames, K, D, q, md)
        _same_call(got, _model(frames, flows, K, D, q, md), f"D={D}")
        check_invariants(*got, D, md)
        reborn += int(got[3][1:].sum())
    assert reborn > 0, "tracks should end and be replaced on this video"
    assert _same_as_klt(frames, K, q, md) > 50
    # another window, a budget above the number of corners (slots that never fill), md = 0 and md <= 1
    flows = _host_fb(frames[:6], 2, 7, 2)[0][:4]
    for md_, K_ in ((0.0, 40), (1.0, 40), (9.0, 5000)):
        got = _call(frames[:6], K_, 2, 0.05, md_, levels=2, win=7, iters=2)
        _same_call(got, _model(frames[:6], flows, K_, 2, 0.05, md_, win=7), f"window 7 md={md_} K={K_}")
        check_invariants(*got, 2, md_)
    _same_as_klt(frames[:6], 5000, 0.05, 9.0, levels=2, win=7, iters=2)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_whole_call_equals_the_model_chunked_1080p(u8):
    """18 frames of 1080p: chunks of 4, 4, 4, 4 and 1 pairs.  D = 3: detection frames 0, 3, .. 15, inside chunks and on chunk
    starts; D = 4: 0, 4, .. 16, on every chunk start and on T-2"""
    frames = _video(18, 1080, 1920, seed=8, u8=u8)
    K, q, md = 2000, 0.01, 10.0
    flows = _host_fb(frames, 3, 5, 3)[0][:4]
    for D in (3, 4):
        got = _call(frames, K, D, q, md)
        _same_call(got, _model(frames, flows, K, D, q, md), f"1080p D={D}")
        check_invariants(*got, D, md)
        assert got[3][0] == K and got[3][D::D].sum() > 0, got[3]
        print(f"1080p u8={u8} D={D}: detected {got[3].tolist()}, visible on the last frame {int(got[1][-1].sum())}")
    assert _same_as_klt(frames, K, q, md) == K


def test_python_call_and_split_tracks():
    import lucas_kanade_core as LK
    import lucas_kanade_pyramidal as P

    frames = _video(9, 120, 160, seed=6, u8=True)
    res = P.lucas_kanade_pyramidal_sequence_klt_replenish(frames, 80, 2, 0.01, 6.0)
    got = _call(frames, 80, 2, 0.01, 6.0)
    _same(_norm(res.tracks), _norm(got[0]), "python tracks")
    assert res.visible.dtype == bool and np.array_equal(res.visible, got[1].astype(bool))
    assert res.born.dtype == bool and np.array_equal(res.born, got[2].astype(bool))
    assert np.array_equal(res.detected, got[3])
    parts = LK.split_tracks(res.visible, res.born)
    assert len(parts) == int(res.detected.sum())
    for n, a, b in parts:
        assert res.born[a, n] and res.visible[a:b + 1, n].all() and not np.isnan(res.tracks[a:b + 1, n]).any()
    # one detection through Python equals row 0 of the call
    qt, qxy, born, n = LK.replenish_features(frames[0], np.full((80, 2), np.nan, np.float32), np.zeros(80, bool), 80, 0.01, 6.0)
    assert n == res.detected[0] and np.array_equal(born, res.born[0])
    _same(_norm(qxy), _norm(res.tracks[0]), "row 0")
    assert (qt[born] == 0).all() and (qt[~born] == -1).all()


# ---------------------------------------------------------------------------------------------------------------
# meaning
# ---------------------------------------------------------------------------------------------------------------
def _pan(T=13, H=120, W=200, step=5):
    from oflk_synth import synth_pair

    base = synth_pair(H, W + step * T, pair_index=3)[0].astype(np.float64)
    rng = np.random.default_rng(7)
    out = np.empty((T, H, W), np.float32)
    for t in range(T):
        out[t] = np.clip(base[:, step * t:step * t + W] + rng.normal(0.0, 1.5, (H, W)), 0, 255)
    return out


@pytest.mark.parametrize("K", [60, 150])
def test_replenishing_keeps_more_points_on_a_pan(K):
    """a 5 px per frame pan: content leaves at the left edge and enters at the right.  The detect-once call only loses
    points; detecting every 4th frame ends with strictly more, and some of the new points lie in the strip that entered
    the frame (x >= W - 5 t on frame t).  (The NumPy model on the CPU oracle's flows gives 23 against 30 visible points on
    the last frame for K = 60 and 56 against 77 for K = 150, 11 and 36 of the later-born points in the entered strip;
    those counts are not asserted.)"""
    frames = _pan()
    T, H, W = frames.shape
    q, md, D = 0.01, 8.0, 4
    n, ktr, kvis = _klt(frames, K, q, md)
    tr, vis, born, det = _call(frames, K, D, q, md)
    check_invariants(tr, vis, born, det, D, md)
    entered = 0
    for t in range(1, T):
        x = tr[t][born[t].astype(bool), 0]
        entered += int((x >= W - 5 * t).sum())
    print(f"pan K={K}: visible on the last frame {int(kvis[-1].sum())} (detect once) against {int(vis[-1].sum())} (D={D}); "
          f"{int(det[1:].sum())} born after frame 0, {entered} of them in the entered strip")
    assert vis[-1].sum() > kvis[-1].sum()
    assert entered >= 1


# ---------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------
def test_errors_are_loud():
    import _oflk
    import lucas_kanade_pyramidal as P

    frames = _video(4, 40, 50, seed=1)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_replenish(frames, 10, bad)
        with pytest.raises(ValueError, match="detect_every"):   # OFLK_ERR_INVALID
            _call(frames, 10, bad, 0.01, 5.0)
    for win in (4, 13):
        with pytest.raises(_oflk.OflkError) as e:
            _call(frames, 10, 2, 0.01, 5.0, win=win)
        assert e.value.code == _oflk.OFLK_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="T >= 2"):
        _call(frames[:1], 10, 2, 0.01, 5.0)
    L = _oflk.lib()
    T, H, W = frames.shape
    outs = [np.empty((T, 10, 2), np.float32), np.empty((T, 10), np.uint8), np.empty((T, 10), np.uint8), np.empty(T, np.int32)]
    ptrs = [_oflk.ptr(outs[0]), outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data_as(_oflk._i32p)]
    for i in range(4):
        a = [None if j == i else p for j, p in enumerate(ptrs)]
        assert L.oflk_pyramidal_sequence_klt_replenish(_oflk.ptr(frames), T, H, W, 3, 5, 3, 0.01, 0.5, 0.01, 5.0, 10, 2,
                                                       *a) == _oflk.OFLK_ERR_INVALID
    # the device form: a workspace one byte short, a NULL slot row
    import torch

    d = _DeviceForm(H, W, 10, 5.0, 5, False)
    d.load(frames[0], np.zeros((10, 2), np.float32), np.zeros(10, np.uint8), *_garbage(10, 0))
    d.nbytes -= 1
    with pytest.raises(ValueError, match="workspace"):
        d.enqueue(0.01, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
