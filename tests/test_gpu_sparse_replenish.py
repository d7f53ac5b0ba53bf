"""GPU tests of the replenished KLT on the sparse tracker (run on an MI355X: python -m pytest tests/test_gpu_sparse_replenish.py
-m gpu -q).

oflk_pyramidal_sequence_klt_sparse_replenish (host form) and oflk_plan_sparse_klt_replenish (device form) must equal
sparse_replenish_model.sequence, and oflk_pyramidal_sequence_klt_sparse must equal oflk_good_features_host on frame 0
followed by oflk_pyramidal_sequence_sparse_tracks, byte for byte (NaN bit patterns normalised).  No tolerance anywhere.
"""
import numpy as np
import pytest

import sparse_model as S
import sparse_replenish_model as M
from test_gpu_fb import _same
from test_gpu_replenish import _pan
from test_gpu_sequence import _dev, _video
from test_gpu_tracks import _norm, _queries, _same_tracks
from test_replenish_cpu import check_invariants

pytestmark = pytest.mark.gpu

MR = np.float32(4.0)


# ---------------------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------------------
def _src(frames):
    import _oflk

    return frames.ctypes.data if frames.dtype == np.uint8 else _oflk.ptr(frames)


def _call(frames, K, D, q, md, levels=3, win=5, iters=3, alpha=0.01, beta=0.5, mr=4.0, residual=True):
    """the C entry point, every output preset with bytes that it must overwrite; residual=False: a NULL residual"""
    import _oflk

    frames = np.ascontiguousarray(frames)
    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    tr, vis = np.full((T, K, 2), -7.0, np.float32), np.full((T, K), 9, np.uint8)
    born, det, res = np.full((T, K), 9, np.uint8), np.full(T, -3, np.int32), np.full((T, K), -5.0, np.float32)
    L = _oflk.lib()
    fn = L.oflk_pyramidal_sequence_klt_sparse_replenish_u8 if u8 else L.oflk_pyramidal_sequence_klt_sparse_replenish
    _oflk.check(fn(_src(frames), T, H, W, levels, win, iters, alpha, beta, mr, q, md, K, D, _oflk.ptr(tr), vis.ctypes.data,
                   born.ctypes.data, det.ctypes.data_as(_oflk._i32p), _oflk.ptr(res) if residual else None))
    return tr, vis, born, det, res


def _klt_sparse(frames, K, q, md, levels=3, win=5, iters=3, alpha=0.01, beta=0.5, mr=4.0):
    import _oflk

    frames = np.ascontiguousarray(frames)
    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    cnt = np.full(1, -3, np.int32)
    xy, sc = np.full((K, 2), -7.0, np.float32), np.full(K, -7.0, np.float32)
    tr, vis = np.full((T, K, 2), -7.0, np.float32), np.full((T, K), 9, np.uint8)
    L = _oflk.lib()
    fn = L.oflk_pyramidal_sequence_klt_sparse_u8 if u8 else L.oflk_pyramidal_sequence_klt_sparse
    _oflk.check(fn(_src(frames), T, H, W, levels, win, iters, alpha, beta, mr, q, md, K, cnt.ctypes.data_as(_oflk._i32p),
                   _oflk.ptr(xy), _oflk.ptr(sc), _oflk.ptr(tr), vis.ctypes.data))
    return int(cnt[0]), xy, sc, tr, vis


def _features_then_sparse_tracks(frames, K, q, md, levels=3, win=5, iters=3, alpha=0.01, beta=0.5, mr=4.0):
    """oflk_good_features_host on frame 0, then oflk_pyramidal_sequence_sparse_tracks on all K rows of its xy"""
    import _oflk

    frames = np.ascontiguousarray(frames)
    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    cnt = np.zeros(1, np.int32)
    xy, sc = np.empty((K, 2), np.float32), np.empty(K, np.float32)
    tr, vis = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    L = _oflk.lib()
    gf = L.oflk_good_features_host_u8 if u8 else L.oflk_good_features_host
    st = L.oflk_pyramidal_sequence_sparse_tracks_u8 if u8 else L.oflk_pyramidal_sequence_sparse_tracks
    _oflk.check(gf(_src(frames), 1, H, W, win, q, md, K, cnt.ctypes.data_as(_oflk._i32p), _oflk.ptr(xy), _oflk.ptr(sc)))
    _oflk.check(st(_src(frames), T, H, W, levels, win, iters, alpha, beta, mr, None, _oflk.ptr(xy), K, _oflk.ptr(tr), vis.ctypes.data))
    return int(cnt[0]), xy, sc, tr, vis


def _ended_by_residual(out, mr=MR):
    """(ended tracks, those whose last finite residual exceeds max_residual): a track of split_tracks that ends before the
    last frame; its residuals are its slot's rows from the one after its birth to the one on which it ended"""
    import lucas_kanade_core as LK

    tr, vis, born, det, res = out
    T = vis.shape[0]
    ended = over = 0
    for n, a, b in LK.split_tracks(vis.astype(bool), born.astype(bool)):
        if b == T - 1:
            continue
        ended += 1
        r = res[a + 1:b + 2, n]
        r = r[np.isfinite(r)]
        over += int(r.size > 0 and r[-1] > mr)
    return ended, over


def _births_after_frame_0(out):
    return int(out[3][1:].sum())


# ---------------------------------------------------------------------------------------------------------------
# the whole call on the _video clip
# ---------------------------------------------------------------------------------------------------------------
VIDEO = dict(K=120, q=0.01, md=6.0)
_clips = {}


def _video_clip(u8):
    """the clip, its pyramids and the statement's outputs, computed once per element type"""
    if u8 not in _clips:
        frames = _video(11, 120, 160, seed=5, u8=u8)
        pyr = [S.pyramid(f.astype(np.float32), 3) for f in frames]
        _clips[u8] = dict(frames=frames, pyr=pyr, want={})
    return _clips[u8]


def _video_want(u8, D):
    c = _video_clip(u8)
    if D not in c["want"]:
        c["want"][D] = M.sequence(c["frames"], VIDEO["K"], D, VIDEO["q"], VIDEO["md"], pyramids=c["pyr"])
    return c["want"][D]


@pytest.mark.parametrize("D", [1, 2, 3, 5])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_whole_call_equals_the_model(u8, D):
    frames = _video_clip(u8)["frames"]
    want = _video_want(u8, D)
    got = _call(frames, VIDEO["K"], D, VIDEO["q"], VIDEO["md"])
    M.same(got, want, f"D={D}")
    check_invariants(*got[:4], D, VIDEO["md"])
    ended, over = _ended_by_residual(got)
    print(f"video u8={u8} D={D}: {_births_after_frame_0(got)} born after frame 0, {ended} tracks ended, {over} of them with a last "
          f"residual above max_residual")
    assert _births_after_frame_0(got) > 0
    assert over >= 1, "at least one track should end by the residual test"


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_detect_once_equals_klt_sparse_equals_features_then_sparse_tracks(u8):
    frames = _video_clip(u8)["frames"]
    T = frames.shape[0]
    K, q, md = VIDEO["K"], VIDEO["q"], VIDEO["md"]
    n, xy, sc, ktr, kvis = _klt_sparse(frames, K, q, md)
    assert n > 50
    wn, wxy, wsc, wtr, wvis = _features_then_sparse_tracks(frames, K, q, md)
    assert n == wn
    _same(_norm(xy), _norm(wxy), "klt_sparse: xy")
    _same(sc, wsc, "klt_sparse: score")
    _same_tracks((ktr, kvis), (wtr, wvis), "klt_sparse: tracks of good-features then sparse-tracks")
    want = _video_want(u8, T)
    _same_tracks((ktr, kvis), want[:2], "klt_sparse: the statement at D = T")
    for D in (T, T + 1, 2 ** 31 - 1):
        tr, vis, born, det, res = _call(frames, K, D, q, md)
        _same_tracks((tr, vis), (ktr, kvis), f"D={D}: rows of klt_sparse")
        _same(born[0], vis[0], f"D={D}: born on frame 0")
        assert not born[1:].any() and det.tolist() == [n] + [0] * (T - 1)
        _same(_norm(res), _norm(want[4]), f"D={D}: residual")


def test_python_calls():
    import lucas_kanade_core as LK
    import lucas_kanade_pyramidal as P

    frames = _video_clip(True)["frames"]
    K, q, md = VIDEO["K"], VIDEO["q"], VIDEO["md"]
    r = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, K, 2, q, md)
    want = _video_want(True, 2)
    assert r.visible.dtype == bool and r.born.dtype == bool and r.residual.dtype == np.float32
    M.same((r.tracks, r.visible, r.born, r.detected, r.residual), want, "python call")
    parts = LK.split_tracks(r.visible, r.born)
    assert len(parts) == int(r.detected.sum())
    k = P.lucas_kanade_pyramidal_sequence_klt_sparse(frames, K, q, md)
    n, xy, _, tr, vis = _klt_sparse(frames, K, q, md)
    assert k.xy.shape == (n, 2) and k.visible.dtype == bool
    _same(k.xy, xy[:n], "python klt_sparse: xy")
    _same_tracks((k.tracks, k.visible), (tr[:, :n], vis[:, :n]), "python klt_sparse")


# ---------------------------------------------------------------------------------------------------------------
# other configurations
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md,K", [(0.0, 40), (1.0, 40), (9.0, 5000)])
def test_window_7_two_levels_two_iterations(md, K):
    frames = _video_clip(False)["frames"][:6]
    want = M.sequence(frames, K, 2, 0.05, md, 2, 7, 2)
    got = _call(frames, K, 2, 0.05, md, levels=2, win=7, iters=2)
    M.same(got, want, f"7x7 md={md} K={K}")
    check_invariants(*got[:4], 2, md)
    assert _births_after_frame_0(got) > 0
    if K == 5000:
        assert 0 < got[3][0] < K and not got[1][:, -1000:].any(), "slots that never fill"
        n, xy, sc, tr, vis = _klt_sparse(frames, K, 0.05, md, levels=2, win=7, iters=2)
        assert n == got[3][0]
        _same_tracks((tr, vis), M.sequence(frames, K, 6, 0.05, md, 2, 7, 2)[:2], "klt_sparse with empty slots")


@pytest.mark.parametrize("win", [3, 9, 11])
def test_other_windows(win):
    frames = _video_clip(False)["frames"][:5]
    u8 = np.rint(frames).astype(np.uint8)
    for f in (frames, u8):
        got = _call(f, 60, 2, 0.01, 6.0, levels=2, win=win, iters=2)
        M.same(got, M.sequence(f, 60, 2, 0.01, 6.0, 2, win, 2), f"window {win} {f.dtype}")
        assert _births_after_frame_0(got) > 0


def test_a_null_residual_gives_the_same_other_outputs():
    frames = _video_clip(False)["frames"]
    got = _call(frames, VIDEO["K"], 2, VIDEO["q"], VIDEO["md"], residual=False)
    M.same(got[:4], _video_want(False, 2)[:4], "NULL residual")
    assert (got[4] == np.float32(-5.0)).all()


# ---------------------------------------------------------------------------------------------------------------
# the chunk cut
# ---------------------------------------------------------------------------------------------------------------
_long = {}


def _long_clip():
    """70 frames of 40 x 52 (the recipe of test_a_long_sequence_is_cut_into_chunks): 69 pairs go as chunks of 64 and 5"""
    if not _long:
        from scipy.ndimage import gaussian_filter, shift

        T, H, W = 70, 40, 52
        rng = np.random.default_rng(9)
        base = gaussian_filter(rng.random((H + 40, W + 60)) * 255.0, 1.5)
        base = (base - base.min()) / (base.max() - base.min()) * 220.0 + 15.0
        frames = np.stack([shift(base, (0.11 * t, -0.23 * t), order=1, mode="nearest")[20:20 + H, 40:40 + W] +
                           rng.normal(0, 0.7, (H, W)) for t in range(T)]).astype(np.float32)
        _long.update(frames=frames, pyr=[S.pyramid(f, 3) for f in frames])
    return _long


@pytest.mark.parametrize("D", [4, 3, 64])
def test_a_long_sequence_is_cut_into_chunks(D):
    """the second chunk begins on frame 64.  D = 4: a detection frame on the cut and others after it; D = 3: detections inside
    both chunks, none on the cut; D = 64: the only later detection is on the cut"""
    c = _long_clip()
    K, md = 60, 4.0
    want = M.sequence(c["frames"], K, D, 0.01, md, pyramids=c["pyr"])
    got = _call(c["frames"], K, D, 0.01, md)
    M.same(got, want, f"70 frames D={D}")
    check_invariants(*got[:4], D, md)
    tr, vis, born, det, res = got
    on, after = int(det[64]), int(det[65:].sum())
    across = int((vis[63] & vis[64] & vis[65] & (1 - born[64]) & (1 - born[65])).sum())
    print(f"70 frames D={D}: {on} born on the cut, {after} after it, {across} tracks alive across it")
    assert across > 0
    if D == 4:
        assert on > 0 and after > 0
    elif D == 3:
        assert on == 0 and after > 0 and det[1:64].sum() > 0
    else:
        assert on > 0 and det[1:64].sum() == 0 and after == 0


# ---------------------------------------------------------------------------------------------------------------
# the device form
# ---------------------------------------------------------------------------------------------------------------
class _DeviceForm:
    """the buffers of oflk_plan_sparse_klt_replenish for plans of B pairs of one shape; outputs preset with sentinels"""

    def __init__(self, B, H, W, K, md, levels=3, win=5, iters=3, u8=False, garbage=0xA5):
        import torch

        import _oflk

        dev = torch.device("cuda", 0)
        self.B, self.H, self.W, self.K, self.md, self.win, self.u8 = B, H, W, K, md, win, u8
        self.plan = _oflk.Plan(0, B, H, W, levels, win, iters)
        self.nbytes = _oflk.replenish_features_workspace(H, W, win, md, K)
        self.ws = torch.full((self.nbytes,), garbage, dtype=torch.uint8, device=dev)   # no zeroed workspace is needed
        self.frames = torch.empty((B + 1, H, W), dtype=torch.uint8 if u8 else torch.float32, device=dev)
        self.qt = torch.full((K,), 12345, dtype=torch.int32, device=dev)
        self.qxy = torch.full((K, 2), -7.0, dtype=torch.float32, device=dev)
        self.tr = torch.empty((B + 1, K, 2), dtype=torch.float32, device=dev)
        self.vis = torch.empty((B + 1, K), dtype=torch.uint8, device=dev)
        self.born = torch.empty((B + 1, K), dtype=torch.uint8, device=dev)
        self.det = torch.empty((B + 1,), dtype=torch.int32, device=dev)
        self.res = torch.empty((B + 1, K), dtype=torch.float32, device=dev)
        self.preset()

    def preset(self):
        self.tr.fill_(-7.0)
        self.vis.fill_(9)
        self.born.fill_(9)
        self.det.fill_(-3)
        self.res.fill_(-5.0)

    def load(self, frames, state=None):
        """the frames and, for a continued call, the previous call's last row as row 0 (qt and qxy stay as the previous
        call on these buffers left them)"""
        import torch

        self.frames.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
        self.preset()
        if state is not None:
            self.tr[0] = torch.from_numpy(np.ascontiguousarray(state[0], np.float32)).to(self.tr.device)
            self.vis[0] = torch.from_numpy(np.asarray(state[1], np.uint8)).to(self.tr.device)

    def enqueue(self, D, q, t0, stream, residual=True, **kw):
        import _oflk

        _oflk.sparse_klt_replenish(self.plan, self.frames.data_ptr(), self.ws.data_ptr(), self.nbytes, self.qt.data_ptr(),
                                   self.qxy.data_ptr(), self.tr.data_ptr(), self.vis.data_ptr(), self.born.data_ptr(),
                                   self.det.data_ptr(), self.K, D, q, self.md, t0=t0, d_residual=self.res.data_ptr() if residual else 0,
                                   u8=self.u8, stream=stream, **kw)

    def read(self):
        import torch

        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.tr, self.vis, self.born, self.det, self.res))

    def run(self, frames, D, q, t0=0, state=None, **kw):
        import torch

        self.load(frames, state)
        self.enqueue(D, q, t0, torch.cuda.current_stream().cuda_stream, **kw)
        return self.read()

    def close(self):
        self.plan.close()


DEV = dict(T=7, H=120, W=160, K=80, q=0.01, md=6.0, D=2)


@pytest.fixture(scope="module")
def dev_clip():
    """seven frames of two clips and the statement on them (D = 2), computed once"""
    out = []
    for seed in (5, 6):
        frames = _video(DEV["T"], DEV["H"], DEV["W"], seed=seed)
        pyr = [S.pyramid(f, 3) for f in frames]
        out.append(dict(frames=frames, pyr=pyr, want=M.sequence(frames, DEV["K"], DEV["D"], DEV["q"], DEV["md"], pyramids=pyr)))
    assert all(c["want"][3][1:].sum() > 0 for c in out)
    return out


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_device_form_equals_the_model(dev_clip, u8):
    """one call, float32 and uint8 frames, over a workspace of two kinds of garbage; a NULL residual changes nothing else"""
    frames = dev_clip[0]["frames"]
    want = dev_clip[0]["want"]
    if u8:
        frames = np.rint(frames).astype(np.uint8)
        want = M.sequence(frames, DEV["K"], DEV["D"], DEV["q"], DEV["md"])
    for garbage in (0xA5, 0xFF):
        d = _DeviceForm(DEV["T"] - 1, DEV["H"], DEV["W"], DEV["K"], DEV["md"], u8=u8, garbage=garbage)
        try:
            M.same(d.run(frames, DEV["D"], DEV["q"]), want, f"one call, workspace of {garbage:#x}")
            got = d.run(frames, DEV["D"], DEV["q"], residual=False)
            M.same(got[:4], want[:4], "NULL residual")
            assert (got[4] == np.float32(-5.0)).all()
        finally:
            d.close()


@pytest.mark.parametrize("cut", [2, 3], ids=["cut on a detection frame", "cut between detection frames"])
def test_device_form_in_two_calls_equals_one(dev_clip, cut):
    """the second call starts from the first's last row (t0 = cut > 0) with the first's d_qt and d_qxy; row 0 of its residual is
    not written"""
    frames, want = dev_clip[0]["frames"], dev_clip[0]["want"]
    T = DEV["T"]
    a = _DeviceForm(cut, DEV["H"], DEV["W"], DEV["K"], DEV["md"])
    b = _DeviceForm(T - 1 - cut, DEV["H"], DEV["W"], DEV["K"], DEV["md"])
    try:
        first = a.run(frames[:cut + 1], DEV["D"], DEV["q"])
        assert not first[2][-1].any() and first[3][-1] == 0, "the last row of a call is never a detection row"
        b.qt.copy_(a.qt)
        b.qxy.copy_(a.qxy)
        second = b.run(frames[cut:], DEV["D"], DEV["q"], t0=cut, state=(first[0][-1], first[1][-1]))
        assert (second[4][0] == np.float32(-5.0)).all(), "residual row 0 of a continued call is the caller's"
        M.same(M.join(first, second), want, f"two calls cut at {cut}")
        assert (second[3][0] > 0) == (cut % DEV["D"] == 0)
    finally:
        a.close()
        b.close()


def test_device_form_replays_from_a_graph_and_leaves_the_plan_usable(dev_clip, oracle):
    """after one eager call, a capture on a side stream is replayed on other frames in the same buffers; then a dense pass
    and a plain oflk_plan_sparse_tracks call on the same plan equal their own statements"""
    import torch

    import _oflk

    T, H, W = DEV["T"], DEV["H"], DEV["W"]
    d = _DeviceForm(T - 1, H, W, DEV["K"], DEV["md"])
    try:
        M.same(d.run(dev_clip[0]["frames"], DEV["D"], DEV["q"]), dev_clip[0]["want"], "eager")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            d.enqueue(DEV["D"], DEV["q"], 0, torch.cuda.current_stream().cuda_stream)
        for rep, i in enumerate((1, 0, 1)):
            d.load(dev_clip[i]["frames"])
            d.ws.fill_(rep)
            d.qt.fill_(777)
            g.replay()
            M.same(d.read(), dev_clip[i]["want"], f"replay {rep} of clip {i}")
        del g
        # the plan afterwards: plain sparse tracks, a dense pass, sparse tracks again
        frames = dev_clip[0]["frames"]
        qt, qxy = _queries(T - 1, H, W, 200, seed=8)
        d_f, d_q, d_qt = _dev(frames), _dev(qxy), _dev(qt.astype(np.int32))
        want = S.track(frames, qt, qxy, 3, 5, 3, pyramids=dev_clip[0]["pyr"])

        def sparse():
            tr = torch.full((T, len(qxy), 2), -7.0, dtype=torch.float32, device=d_f.device)
            vis = torch.full((T, len(qxy)), 9, dtype=torch.uint8, device=d_f.device)
            _oflk.sparse_tracks(d.plan, d_f.data_ptr(), d_q.data_ptr(), len(qxy), tr.data_ptr(), vis.data_ptr(), d_qt=d_qt.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return tr.cpu().numpy(), vis.cpu().numpy()

        _same_tracks(sparse(), want, "plain sparse tracks after the replenished calls")
        d_u, d_v = (torch.empty((T - 1, H, W), dtype=torch.float32, device=d_f.device) for _ in range(2))
        st = torch.cuda.current_stream().cuda_stream
        d.plan.pyramidal_sequence(d_f.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
        flags = d.plan.read_uncertain(st)
        torch.cuda.synchronize()
        flags = (np.asarray(flags) != 0).any(1)
        u, v = d_u.cpu().numpy(), d_v.cpu().numpy()
        sure = np.flatnonzero(~flags)
        assert sure.size > 0
        for t in sure[:3]:   # a pair whose exit decisions were certain is the oracle's flow
            ou, ov = oracle.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3)
            assert np.array_equal(u[t], ou) and np.array_equal(v[t], ov), f"dense pair {t} after the replenished calls"
        _same_tracks(sparse(), want, "plain sparse tracks after the dense pass")
        M.same(d.run(frames, DEV["D"], DEV["q"]), dev_clip[0]["want"], "the replenished call after the dense pass")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------
# meaning
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [60, 150])
def test_replenishing_keeps_more_points_on_a_pan(K):
    """the 5 px per frame pan of the dense replenished call's test, both calls sparse: detecting every 4th frame ends with
    strictly more points than detecting once, and some later-born points lie in the strip that entered the frame.  (The
    statement gives 43 against 34 visible points on the last frame for K = 60 and 119 against 94 for K = 150, 10 and 30
    later-born points in the entered strip; those counts are not asserted.)"""
    frames = _pan()
    T, H, W = frames.shape
    q, md, D = 0.01, 8.0, 4
    n, _, _, ktr, kvis = _klt_sparse(frames, K, q, md)
    tr, vis, born, det, res = _call(frames, K, D, q, md)
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
    import torch

    import _oflk
    import lucas_kanade_pyramidal as P

    frames = _video(4, 40, 50, seed=1)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, 10, bad)
        with pytest.raises(ValueError, match="detect_every"):
            _call(frames, 10, bad, 0.01, 5.0)
    for win in (4, 13):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, 10, 2, window_size=win)
        for fn in (lambda: _call(frames, 10, 2, 0.01, 5.0, win=win), lambda: _klt_sparse(frames, 10, 0.01, 5.0, win=win)):
            with pytest.raises(_oflk.OflkError) as e:
                fn()
            assert e.value.code == _oflk.OFLK_ERR_UNSUPPORTED
    with pytest.raises(_oflk.OflkError) as e:
        _call(frames[:, :7, :9], 10, 2, 0.01, 5.0)   # a level below 2 x 2
    assert e.value.code == _oflk.OFLK_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="T >= 2"):
        _call(frames[:1], 10, 2, 0.01, 5.0)
    for kw in (dict(iters=0), dict(levels=0), dict(alpha=-1.0), dict(beta=float("nan")), dict(mr=-1.0), dict(mr=float("nan"))):
        with pytest.raises(ValueError):
            _call(frames, 10, 2, 0.01, 5.0, **kw)
        with pytest.raises(ValueError):
            _klt_sparse(frames, 10, 0.01, 5.0, **kw)
    for q, md, K in ((2.0, 5.0, 10), (0.01, -1.0, 10), (0.01, 5.0, 0)):
        with pytest.raises(ValueError):
            _call(frames, K, 2, q, md)
    # the device form, before any device call
    T, H, W = frames.shape
    d = _DeviceForm(T - 1, H, W, 10, 5.0)
    st = torch.cuda.current_stream().cuda_stream
    try:
        d.load(frames)
        for kw in (dict(D=0), dict(t0=-1), dict(q=1.5), dict(alpha=-1.0), dict(max_residual=-1.0), dict(max_residual=float("nan"))):
            a = dict(D=2, q=0.01, t0=0)
            extra = {k: kw[k] for k in kw if k not in a}
            a.update({k: kw[k] for k in kw if k in a})
            with pytest.raises(ValueError):
                d.enqueue(a["D"], a["q"], a["t0"], st, **extra)
        d.nbytes -= 1
        with pytest.raises(ValueError, match="workspace"):   # a workspace one byte short
            d.enqueue(2, 0.01, 0, st)
        d.nbytes += 1
        args = [d.ws.data_ptr(), d.nbytes, d.qt.data_ptr(), d.qxy.data_ptr(), d.tr.data_ptr(), d.vis.data_ptr(), d.born.data_ptr(),
                d.det.data_ptr()]
        for i in (0, 2, 3, 4, 5, 6, 7):   # a NULL workspace, query buffer, slot row (tracks, visible) or output
            a = list(args)
            a[i] = 0
            with pytest.raises(ValueError, match="NULL"):
                _oflk.sparse_klt_replenish(d.plan, d.frames.data_ptr(), *a, 10, 2, 0.01, 5.0, stream=st)
        with pytest.raises(ValueError, match="NULL"):
            _oflk.sparse_klt_replenish(d.plan, 0, *args, 10, 2, 0.01, 5.0, stream=st)
        with pytest.raises(ValueError, match="aligned"):
            a = list(args)
            a[0] += 8
            _oflk.sparse_klt_replenish(d.plan, d.frames.data_ptr(), *a, 10, 2, 0.01, 5.0, stream=st)
        torch.cuda.synchronize()
        assert (d.read()[1] == 9).all(), "a refused call writes nothing"
    finally:
        d.close()
