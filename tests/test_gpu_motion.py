"""GPU tests of the global motion fit (run on an MI355X: python -m pytest tests/test_gpu_motion.py -m gpu -q).

Every output -- model, mask, counts -- of oflk_estimate_motion, oflk_tracks_motion, the host form and the tracker's motion row
must equal the statement (tests/motion_model.py) byte for byte; a NaN equals a NaN.  No tolerance anywhere.
"""
import ctypes

import numpy as np
import pytest

import motion_model as MM
from test_gpu_sparse_replenish import _call
from test_sparse_cpu import _drifting

pytestmark = pytest.mark.gpu

MODELS = [MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE]
IDS = ["translation", "similarity", "affine"]


class _Device:
    """the device form on buffers of S steps of N correspondences: outputs and workspace preset with bytes that the call must
    overwrite"""

    def __init__(self, S, N, hyps):
        import torch

        import _oflk

        self.S, self.N, self.hyps = S, N, hyps
        d = "cuda:0"
        self.src, self.dst = torch.zeros((S, N, 2), device=d), torch.zeros((S, N, 2), device=d)
        self.valid = torch.zeros((S, N), dtype=torch.uint8, device=d)
        self.ws_bytes = _oflk.motion_workspace(S, N, hyps)
        self.ws = torch.full((self.ws_bytes,), 0xA5, dtype=torch.uint8, device=d)
        self.model = torch.full((S, 6), -7.0, device=d)
        self.inlier = torch.full((S, N), 9, dtype=torch.uint8, device=d)
        self.counts = torch.full((S, 3), -3, dtype=torch.int32, device=d)

    def load(self, src, dst, valid=None):
        import torch

        self.src.copy_(torch.from_numpy(np.ascontiguousarray(src, np.float32).reshape(self.S, self.N, 2)))
        self.dst.copy_(torch.from_numpy(np.ascontiguousarray(dst, np.float32).reshape(self.S, self.N, 2)))
        if valid is not None:
            self.valid.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(valid) != 0, np.uint8).reshape(self.S, self.N)))

    def enqueue(self, model, thr, seed, step0=0, stream=0, masked=True):
        import _oflk

        _oflk.estimate_motion(self.src.data_ptr(), self.dst.data_ptr(), self.valid.data_ptr() if masked else 0, self.S, self.N,
                              self.ws.data_ptr(), self.ws_bytes, self.model.data_ptr(), self.inlier.data_ptr(),
                              self.counts.data_ptr(), model, self.hyps, thr, seed, step0, stream)

    def read(self):
        import torch

        torch.cuda.synchronize()
        return self.model.cpu().numpy(), self.inlier.cpu().numpy(), self.counts.cpu().numpy()

    def run(self, src, dst, valid, model, thr, seed, step0=0):
        self.load(src, dst, valid)
        self.enqueue(model, thr, seed, step0, masked=valid is not None)
        return self.read()


def _mixed(S, N, seed):
    """S planted steps of N correspondences, 30 % outliers, a few invalid and a few not finite"""
    rng = np.random.default_rng(seed)
    scenes = [MM.planted_scene(N, 0.3, seed * 10 + s) for s in range(S)]
    src, dst = np.stack([x[0] for x in scenes]), np.stack([x[1] for x in scenes])
    valid = rng.random((S, N)) < 0.9
    if N >= 4:
        dst[0, N // 2, 1] = np.nan
        src[S - 1, N // 3, 0] = np.inf
    return src, dst, valid


# ---------------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_every_size_equals_the_model(model, S):
    """N around the sample sizes, the wave, the compaction's and the refit's blocks; hypotheses below, at and over the four
    waves of a scoring block and over a multiple of 64; with a mask and without; step0 != 0 in the batches"""
    step0 = 0 if S == 1 else 17
    for N in (1, 2, 3, 4, 63, 64, 65, 129, 1000, 1025):
        src, dst, valid = _mixed(S, N, N)
        for hyps in (1, 3, 4, 64, 257):
            dev = _Device(S, N, hyps)
            for v in (valid, None):
                got = dev.run(src, dst, v, model, 1.0, seed=N + hyps, step0=step0)
                want = MM.estimate_batch(src, dst, v, model, hyps, 1.0, N + hyps, step0)
                MM.same(got, want, f"S={S} N={N} Hn={hyps} family {model} masked={v is not None}")


def test_a_step_without_valid_correspondences_in_the_middle_of_a_batch():
    src, dst, valid = _mixed(3, 65, 4)
    valid[1] = False
    dev = _Device(3, 65, 64)
    for model in MODELS:
        got = dev.run(src, dst, valid, model, 1.0, seed=2, step0=5)
        MM.same(got, MM.estimate_batch(src, dst, valid, model, 64, 1.0, 2, 5), f"family {model}")
        assert got[2][1].tolist() == [0, 0, 0] and np.isnan(got[0][1]).all() and not got[1][1].any()
        assert got[2][0][2] == 1 and got[2][2][2] == 1
    # the index of a step, not its place in the batch, decides its draws
    one = _Device(1, 65, 64)
    got = one.run(src[2], dst[2], valid[2], MM.AFFINE, 1.0, seed=2, step0=7)
    MM.same(tuple(x[0] for x in got), MM.estimate(src[2], dst[2], valid[2], MM.AFFINE, 64, 1.0, 2, 7), "step 2 alone")


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("N,share,hyps", MM.PLANTED)
def test_planted_scenes(N, share, hyps, model):
    src, dst, planted = MM.planted_scene(N, share, 100)
    got = _Device(1, N, hyps).run(src, dst, None, model, 1.0, seed=0)
    MM.same(tuple(x[0] for x in got), MM.estimate(src, dst, None, model, hyps, 1.0, 0), f"N={N} family {model}")
    if model != MM.TRANSLATION:
        assert np.array_equal(got[1][0].astype(bool), planted)


def test_edge_cases_on_the_device_and_through_the_host_form():
    import lucas_kanade_core as K

    names = {v: k for k, v in MM.FAMILIES.items()}
    for name, src, dst, valid, model, hyps, thr in MM.edge_cases():
        want = MM.estimate(src, dst, valid, model, hyps, thr, seed=1, index=3)
        got = _Device(1, len(src), hyps).run(src, dst, valid, model, thr, seed=1, step0=3)
        MM.same(tuple(x[0] for x in got), want, name)
        m = K.estimate_motion(src, dst, valid, names[model], hyps, thr, seed=1, step0=3)
        MM.same((m.model.reshape(6), m.inlier, np.int32([m.n_inliers, m.n_valid, m.status])), want, name + " (host form)")
        assert m.model.shape == (2, 3) and m.inlier.dtype == bool and isinstance(m.status, int)


def test_the_host_form_equals_the_device_form():
    import lucas_kanade_core as K

    src, dst, valid = _mixed(3, 200, 9)
    dev = _Device(3, 200, 128)
    for v in (valid, None):
        got = dev.run(src, dst, v, MM.SIMILARITY, 1.0, seed=77, step0=2)
        m = K.estimate_motion(src, dst, v, "similarity", 128, 1.0, seed=77, step0=2)
        assert m.model.shape == (3, 2, 3) and m.inlier.shape == (3, 200) and m.status.tolist() == [1, 1, 1]
        MM.same((m.model.reshape(3, 6), m.inlier, np.stack([m.n_inliers, m.n_valid, m.status], -1)), got, "host against device")
        MM.same(got, MM.estimate_batch(src, dst, v, MM.SIMILARITY, 128, 1.0, 77, 2), "device against the model")


# ---------------------------------------------------------------------------------------------------------------------
# rows of the track calls
# ---------------------------------------------------------------------------------------------------------------------
CLIP = dict(T=6, H=96, W=128, seed=11, K=64, D=2, q=0.05, md=6.0)
_clip = {}


def _rows():
    """the clip and the rows of oflk_pyramidal_sequence_klt_sparse_replenish on it, once"""
    if not _clip:
        frames = _drifting(CLIP["T"], CLIP["H"], CLIP["W"], CLIP["seed"])
        _clip["frames"] = frames
        _clip["rows"] = _call(frames, CLIP["K"], CLIP["D"], CLIP["q"], CLIP["md"])
        tr, vis, born = _clip["rows"][:3]
        refilled = (vis[:-1] != 0) & (born[1:] != 0)
        assert born[1:].any() and refilled.any(), "the clip must refill slots, one of them on the row its track ended on"
    return _clip["frames"], _clip["rows"]


def _tracks_device(tr, vis, born, model, hyps, thr, seed, t0):
    import torch

    import _oflk

    T, K = vis.shape
    d = "cuda:0"
    t_tr, t_vis = torch.from_numpy(tr).to(d), torch.from_numpy(vis).to(d)
    t_born = None if born is None else torch.from_numpy(born).to(d)
    nb = _oflk.motion_workspace(T - 1, K, hyps)
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=d)
    out = torch.full((T - 1, 6), -7.0, device=d)
    inl = torch.full((T - 1, K), 9, dtype=torch.uint8, device=d)
    cnt = torch.full((T - 1, 3), -3, dtype=torch.int32, device=d)
    _oflk.tracks_motion(t_tr.data_ptr(), t_vis.data_ptr(), 0 if born is None else t_born.data_ptr(), T, K, ws.data_ptr(), nb,
                        out.data_ptr(), inl.data_ptr(), cnt.data_ptr(), model, hyps, thr, seed, t0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), inl.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_tracks_motion_on_the_rows_of_the_sequence_call(model):
    import lucas_kanade_core as K

    _, (tr, vis, born, det, res) = _rows()
    want = MM.tracks(tr, vis, born, model, 64, 0.5, seed=3, t0=5)
    MM.same(_tracks_device(tr, vis, born, model, 64, 0.5, 3, 5), want, "oflk_tracks_motion")
    assert want[2][1][1] == (vis[1] != 0).sum() - ((vis[1] != 0) & (born[2] != 0)).sum() - ((vis[1] != 0) & (vis[2] == 0)).sum()
    MM.same(_tracks_device(tr, vis, None, model, 64, 0.5, 3, 5), MM.tracks(tr, vis, None, model, 64, 0.5, 3, 5), "without born")
    m = K.tracks_motion(tr, vis, born, IDS[model], 64, 0.5, seed=3, t0=5)
    MM.same((m.model.reshape(-1, 6), m.inlier, np.stack([m.n_inliers, m.n_valid, m.status], -1)), want, "tracks_motion (Python)")


# ---------------------------------------------------------------------------------------------------------------------
# the online tracker
# ---------------------------------------------------------------------------------------------------------------------
def _tracker(frames, **kw):
    import _oflk

    return _oflk.Tracker(0, frames.shape[1], frames.shape[2], frames.dtype == np.uint8, CLIP["K"], CLIP["D"], 3, 5, 3,
                         quality_level=CLIP["q"], min_distance=CLIP["md"], **kw)


def _stack(ms):
    return tuple(np.stack([m[j] for m in ms]) for j in range(3))


@pytest.mark.parametrize("model", [MM.SIMILARITY, MM.AFFINE], ids=["similarity", "affine"])
def test_the_motions_of_the_pushes_equal_tracks_motion_of_the_sequence_call(model):
    frames, (tr, vis, born, det, res) = _rows()
    want = MM.tracks(tr, vis, born, model, 64, 0.5, seed=3, t0=0)
    t = _tracker(frames)
    try:
        t.set_motion(model, 64, 0.5, 3)
        ws0 = t.workspace_bytes
        ms = []
        for f in frames:
            t.push(np.ascontiguousarray(f))
            ms.append(t.read_motion())
        assert t.workspace_bytes > ws0 == 0
        first = ms[0]
        assert np.isnan(first[0]).all() and not first[1].any() and first[2].tolist() == [0, 0, 0], "frame 0 has no step"
        MM.same(_stack(ms[1:]), want, "motion rows of the pushes")
        p = t.motion_device()
        assert all(p) and len(set(p)) == 3
        # after a reset the first frame has no step again, and the same pushes give the same motions
        t.reset()
        with pytest.raises(ValueError):
            t.read_motion()
        t.push(np.ascontiguousarray(frames[0]))
        assert t.read_motion()[2].tolist() == [0, 0, 0]
        t.push(np.ascontiguousarray(frames[1]))
        MM.same(t.read_motion(), tuple(x[0] for x in want), "step 0 after a reset")
    finally:
        t.close()


def test_set_motion_between_pushes_takes_effect_on_the_next_push_and_leaves_the_rows_alone():
    frames, (tr, vis, born, det, res) = _rows()
    plain, mixed = _tracker(frames), _tracker(frames)
    try:
        for i, f in enumerate(frames):
            f = np.ascontiguousarray(f)
            want_row = plain.push(f)
            if i == 2:
                mixed.set_motion(MM.AFFINE, 300, 0.5, 8)
            if i == 4:
                mixed.set_motion(MM.TRANSLATION, 16, 1.5, 9)
            if i == 5:
                mixed.set_motion(-1)
            row = mixed.push(f)
            for a, b in zip(row[:5], want_row[:5]):
                assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"row {i} of a tracker with motion set"
            assert row[5] == want_row[5]
            if i in (2, 3):
                MM.same(mixed.read_motion(), MM.estimate(tr[i - 1], tr[i], MM.tracks_valid(vis, born)[i - 1], MM.AFFINE, 300, 0.5, 8, i - 1),
                        f"push {i}")
            elif i == 4:
                MM.same(mixed.read_motion(), MM.estimate(tr[3], tr[4], MM.tracks_valid(vis, born)[3], MM.TRANSLATION, 16, 1.5, 9, 3),
                        "push 4")
            else:
                with pytest.raises(ValueError):
                    mixed.read_motion()
    finally:
        plain.close()
        mixed.close()


def test_python_tracker_motion():
    import lucas_kanade_pyramidal as P

    frames, (tr, vis, born, det, res) = _rows()
    u8 = np.rint(frames).astype(np.uint8)
    rows = _call(u8, CLIP["K"], CLIP["D"], CLIP["q"], CLIP["md"])
    want = MM.tracks(rows[0], rows[1], rows[2], MM.SIMILARITY, 256, 1.0, 0, 0)
    with P.SparseKltTracker(u8.shape[1:], CLIP["K"], CLIP["D"], CLIP["q"], CLIP["md"], motion="similarity") as t:
        ms = []
        for f in u8:
            t.push(f)
            ms.append(t.motion())
    assert ms[0].status == 0 and ms[0].n_valid == 0 and np.isnan(ms[0].model).all()
    got = (np.stack([m.model.reshape(6) for m in ms[1:]]), np.stack([m.inlier for m in ms[1:]]),
           np.int32([[m.n_inliers, m.n_valid, m.status] for m in ms[1:]]))
    MM.same(got, want, "SparseKltTracker.motion")
    assert ms[1].model.shape == (2, 3) and ms[1].inlier.dtype == bool


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_device_form_replays_from_a_graph_with_changed_inputs():
    """captured once after one eager call, replayed on other correspondences in the same buffers (the process keeps the
    default number of hardware queues); the workspace is scribbled over between replays: nothing in it is carried"""
    import torch

    S, N, hyps = 2, 300, 96
    dev = _Device(S, N, hyps)
    cases = []
    for i in range(3):
        src, dst, valid = _mixed(S, N, 50 + i)
        if i == 2:
            valid[1] = False
        cases.append((src, dst, valid, MM.estimate_batch(src, dst, valid, MM.AFFINE, hyps, 1.0, 6, 9)))
    MM.same(dev.run(*cases[0][:3], MM.AFFINE, 1.0, 6, 9), cases[0][3], "eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        dev.enqueue(MM.AFFINE, 1.0, 6, 9, torch.cuda.current_stream().cuda_stream)
    for rep, i in enumerate((1, 2, 0)):
        dev.load(*cases[i][:3])
        dev.ws.fill_(0x3C + rep)
        dev.model.fill_(-7.0)
        dev.inlier.fill_(9)
        dev.counts.fill_(-3)
        g.replay()
        MM.same(dev.read(), cases[i][3], f"replay {rep} of case {i}")
    del g


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing():
    import torch

    import _oflk

    L = _oflk.lib()
    dev = _Device(2, 10, 16)
    src, dst, valid = _mixed(2, 10, 1)
    dev.load(src, dst, valid)
    a = dict(src=dev.src.data_ptr(), dst=dev.dst.data_ptr(), valid=dev.valid.data_ptr(), S=2, N=10, step0=0, model=1, hyps=16,
             thr=1.0, seed=0, ws=dev.ws.data_ptr(), nb=dev.ws_bytes, out=dev.model.data_ptr(), inl=dev.inlier.data_ptr(),
             cnt=dev.counts.data_ptr())

    def call(**kw):
        b = dict(a, **kw)
        return L.oflk_estimate_motion(b["src"], b["dst"], b["valid"], b["S"], b["N"], b["step0"], b["model"], b["hyps"], b["thr"],
                                      b["seed"], b["ws"], b["nb"], b["out"], b["inl"], b["cnt"], None)

    for kw in [dict(model=3), dict(model=-1), dict(hyps=0), dict(hyps=MM.MAX_HYPOTHESES + 1), dict(thr=0.0), dict(thr=float("nan")),
               dict(thr=float("inf")), dict(thr=-2.0), dict(S=0), dict(N=0), dict(src=None), dict(dst=None), dict(out=None),
               dict(inl=None), dict(cnt=None), dict(ws=None), dict(nb=dev.ws_bytes - 1), dict(ws=a["ws"] + 64), dict(src=a["src"] + 4)]:
        assert call(**kw) == _oflk.OFLK_ERR_INVALID, kw
    nb = ctypes.c_size_t(0)
    assert L.oflk_motion_workspace(2, 10, 0, ctypes.byref(nb)) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_tracks_motion(a["src"], a["valid"], None, 1, 10, 0, 1, 16, 1.0, 0, a["ws"], a["nb"], a["out"], a["inl"], a["cnt"],
                                None) == _oflk.OFLK_ERR_INVALID
    torch.cuda.synchronize()
    m, inl, cnt = dev.read()
    assert (m == -7.0).all() and (inl == 9).all() and (cnt == -3).all(), "a refused call wrote nothing"
    assert (dev.ws.cpu().numpy() == 0xA5).all()
    assert call() == 0
    MM.same(dev.read(), MM.estimate_batch(src, dst, valid, MM.SIMILARITY, 16, 1.0, 0, 0), "the accepted call")
