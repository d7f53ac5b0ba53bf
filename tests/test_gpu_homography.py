"""GPU tests of the homography fit and the perspective warp (run on an MI355X: python -m pytest tests/test_gpu_homography.py
-m gpu -q).

Every output of oflk_estimate_homography, oflk_tracks_homography, oflk_warp_perspective and their host forms must equal the
statement (tests/homography_model.py) byte for byte; a NaN equals a NaN.  No tolerance anywhere.
"""
import numpy as np
import pytest

import homography_model as HM
import stabilize_model as SM

pytestmark = pytest.mark.gpu


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
        self.ws_bytes = _oflk.homography_workspace(S, N, hyps)
        self.ws = torch.full((self.ws_bytes,), 0xA5, dtype=torch.uint8, device=d)
        self.model = torch.full((S, 9), -7.0, device=d)
        self.inlier = torch.full((S, N), 9, dtype=torch.uint8, device=d)
        self.counts = torch.full((S, 3), -3, dtype=torch.int32, device=d)

    def load(self, src, dst, valid=None):
        import torch

        self.src.copy_(torch.from_numpy(np.ascontiguousarray(src, np.float32).reshape(self.S, self.N, 2)))
        self.dst.copy_(torch.from_numpy(np.ascontiguousarray(dst, np.float32).reshape(self.S, self.N, 2)))
        if valid is not None:
            self.valid.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(valid) != 0, np.uint8).reshape(self.S, self.N)))

    def enqueue(self, thr, seed, step0=0, stream=0, masked=True):
        import _oflk

        _oflk.estimate_homography(self.src.data_ptr(), self.dst.data_ptr(), self.valid.data_ptr() if masked else 0, self.S, self.N,
                                  self.ws.data_ptr(), self.ws_bytes, self.model.data_ptr(), self.inlier.data_ptr(),
                                  self.counts.data_ptr(), self.hyps, thr, seed, step0, stream)

    def read(self):
        import torch

        torch.cuda.synchronize()
        return self.model.cpu().numpy(), self.inlier.cpu().numpy(), self.counts.cpu().numpy()

    def run(self, src, dst, valid, thr, seed, step0=0):
        self.load(src, dst, valid)
        self.enqueue(thr, seed, step0, masked=valid is not None)
        return self.read()


def _mixed(S, N, seed):
    """S planted steps of N correspondences, 30 % outliers, a few invalid and a few not finite"""
    rng = np.random.default_rng(seed)
    scenes = [HM.planted_scene(N, 0.3, seed * 10 + s) for s in range(S)]
    src, dst = np.stack([x[0] for x in scenes]), np.stack([x[1] for x in scenes])
    valid = rng.random((S, N)) < 0.9
    if N >= 5:
        dst[0, N // 2, 1] = np.nan
        src[S - 1, N // 3, 0] = np.inf
    return src, dst, valid


def _host(m):
    return m.model.reshape(-1, 9) if m.model.ndim == 3 else m.model.reshape(9)


# ---------------------------------------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no mask"])
@pytest.mark.parametrize("S", [1, 3])
def test_every_size_equals_the_model(S, masked):
    """N around the sample, the wave, the four loads in flight and the blocks; hypotheses below, at and over the four waves of
    a scoring block and over the refit's block; step0 at 2^32 - 1, and 2^32 - 2 in the batches, so that the index wraps inside one"""
    step0 = 2 ** 32 - 1 if S == 1 else 2 ** 32 - 2
    for N in (3, 4, 5, 63, 64, 65, 257, 1025):
        src, dst, valid = _mixed(S, N, N)
        v = valid if masked else None
        for hyps in (1, 3, 4, 5, 64, 257):
            got = _Device(S, N, hyps).run(src, dst, v, 1.0, seed=N + hyps, step0=step0)
            want = HM.estimate_batch(src, dst, v, hyps, 1.0, N + hyps, step0)
            HM.same(got, want, f"S={S} N={N} Hn={hyps} masked={masked}")
            if N >= 64 and hyps >= 64 and not masked:
                assert (got[2][:, 2] == 1).all() and (got[2][:, 0] > N // 2).all(), "the planted scenes are found"


def test_edge_cases_on_the_device_and_through_the_host_form():
    import lucas_kanade_core as K

    for name, src, dst, valid, hyps, thr in HM.edge_cases():
        want = HM.estimate(src, dst, valid, hyps, thr, seed=1, index=3)
        got = _Device(1, len(src), hyps).run(src, dst, valid, thr, seed=1, step0=3)
        HM.same(tuple(x[0] for x in got), want, name)
        m = K.estimate_homography(src, dst, valid, hyps, thr, seed=1, step0=3)
        HM.same((_host(m), m.inlier, np.int32([m.n_inliers, m.n_valid, m.status])), want, name + " (host form)")
        assert m.model.shape == (3, 3) and m.inlier.dtype == bool and isinstance(m.status, int)


@pytest.mark.parametrize("N,share,hyps", HM.PLANTED)
def test_planted_scenes(N, share, hyps):
    src, dst, planted = HM.planted_scene(N, share, 100)
    got = _Device(1, N, hyps).run(src, dst, None, 1.0, seed=0)
    HM.same(tuple(x[0] for x in got), HM.estimate(src, dst, None, hyps, 1.0, 0), f"N={N}")
    assert np.array_equal(got[1][0].astype(bool), planted)


def test_the_host_form_equals_the_device_form_and_two_calls_give_the_same_bytes():
    import lucas_kanade_core as K

    src, dst, valid = _mixed(3, 200, 9)
    dev = _Device(3, 200, 128)
    for v in (valid, None):
        got = dev.run(src, dst, v, 1.0, seed=77, step0=2)
        m = K.estimate_homography(src, dst, v, 128, 1.0, seed=77, step0=2)
        assert m.model.shape == (3, 3, 3) and m.inlier.shape == (3, 200) and m.status.tolist() == [1, 1, 1]
        HM.same((_host(m), m.inlier, np.stack([m.n_inliers, m.n_valid, m.status], -1)), got, "host against device")
        HM.same(got, HM.estimate_batch(src, dst, v, 128, 1.0, 77, 2), "device against the model")
        dev.ws.fill_(0x11)
        dev.model.fill_(-7.0)
        dev.inlier.fill_(9)
        dev.counts.fill_(-3)
        dev.enqueue(1.0, 77, 2, masked=v is not None)
        HM.same(dev.read(), got, "the second call")


def _rows(T=5, K=70, seed=21):
    """T rows of K slots under the planted homography step by step, with planted deaths, births and a refilled slot"""
    rng = np.random.default_rng(seed)
    tr = np.empty((T, K, 2), np.float32)
    tr[0] = HM.planted_scene(K, 0.0, seed)[0]
    for t in range(1, T):
        nxt = HM.apply(HM.planted_homography(), tr[t - 1])
        out = rng.random(K) < 0.25
        tr[t] = np.where(out[:, None], nxt + rng.uniform(5, 40, (K, 2)), nxt).astype(np.float32)
    vis = np.ones((T, K), np.uint8)
    born = np.zeros((T, K), np.uint8)
    vis[2:, 5] = 0                   # dies
    vis[:2, 9], born[2, 9] = 0, 1    # born on row 2
    born[3, 12] = 1                  # dies and is refilled on row 3: visible throughout, two tracks
    vis[1, 20], born[2, 20] = 0, 1   # gone on row 1, back on row 2
    tr[3, 30, 0] = np.nan
    return tr, vis, born


def _tracks_device(tr, vis, born, hyps, thr, seed, t0):
    import torch

    import _oflk

    T, K = vis.shape
    d = "cuda:0"
    t_tr, t_vis = torch.from_numpy(tr).to(d), torch.from_numpy(vis).to(d)
    t_born = None if born is None else torch.from_numpy(born).to(d)
    nb = _oflk.homography_workspace(T - 1, K, hyps)
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=d)
    out = torch.full((T - 1, 9), -7.0, device=d)
    inl = torch.full((T - 1, K), 9, dtype=torch.uint8, device=d)
    cnt = torch.full((T - 1, 3), -3, dtype=torch.int32, device=d)
    _oflk.tracks_homography(t_tr.data_ptr(), t_vis.data_ptr(), 0 if born is None else t_born.data_ptr(), T, K, ws.data_ptr(), nb,
                            out.data_ptr(), inl.data_ptr(), cnt.data_ptr(), hyps, thr, seed, t0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), inl.cpu().numpy(), cnt.cpu().numpy()


def test_tracks_homography_on_rows_with_deaths_and_births():
    import lucas_kanade_core as K

    tr, vis, born = _rows()
    want = HM.tracks(tr, vis, born, 64, 1.0, seed=3, t0=5)
    HM.same(_tracks_device(tr, vis, born, 64, 1.0, 3, 5), want, "oflk_tracks_homography")
    # step 2: slot 5 is dead, slot 30 not finite, and slot 12 was refilled on row 3
    assert want[2][:, 2].tolist() == [1, 1, 1, 1] and want[2][2, 1] == 70 - 3 and not want[1][2, 12]
    without = HM.tracks(tr, vis, None, 64, 1.0, 3, 5)
    HM.same(_tracks_device(tr, vis, None, 64, 1.0, 3, 5), without, "without born")
    assert without[2][2, 1] == 70 - 2
    m = K.tracks_homography(tr, vis, born, 64, 1.0, seed=3, t0=5)
    HM.same((_host(m), m.inlier, np.stack([m.n_inliers, m.n_valid, m.status], -1)), want, "tracks_homography (Python)")
    assert m.model.shape == (4, 3, 3)


def test_device_form_replays_from_a_graph_with_the_same_bytes():
    """captured once after one eager call and replayed twice (the process keeps the default number of hardware queues); the
    outputs and the workspace are scribbled over between replays: nothing in them is carried"""
    import torch

    S, N, hyps = 2, 300, 96
    dev = _Device(S, N, hyps)
    src, dst, valid = _mixed(S, N, 50)
    want = HM.estimate_batch(src, dst, valid, hyps, 1.0, 6, 9)
    HM.same(dev.run(src, dst, valid, 1.0, 6, 9), want, "eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        dev.enqueue(1.0, 6, 9, torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        dev.ws.fill_(0x3C + rep)
        dev.model.fill_(-7.0)
        dev.inlier.fill_(9)
        dev.counts.fill_(-3)
        g.replay()
        HM.same(dev.read(), want, f"replay {rep}")
    del g


# ---------------------------------------------------------------------------------------------------------------------
# the perspective warp
# ---------------------------------------------------------------------------------------------------------------------
def _warp_device(frames, maps, inside=True, offset=0, affine=False):
    """the device form on buffers whose base is `offset` elements past an allocation's start; outputs preset"""
    import torch

    import _oflk

    frames = np.ascontiguousarray(frames)
    F, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    d = "cuda:0"
    n = frames.size
    t_in = torch.zeros(n + offset, dtype=torch.uint8 if u8 else torch.float32, device=d)
    t_in[offset:].copy_(torch.from_numpy(frames.reshape(-1)))
    t_out = torch.full((n + offset,), 77, dtype=t_in.dtype, device=d)
    t_ins = torch.full((n + offset,), 9, dtype=torch.uint8, device=d)
    t_map = torch.from_numpy(np.ascontiguousarray(maps, np.float64).reshape(F, 6 if affine else 9)).to(d)
    sz = frames.itemsize
    fn = _oflk.warp_affine if affine else _oflk.warp_perspective
    fn(t_in.data_ptr() + offset * sz, F, H, W, t_map.data_ptr(), t_out.data_ptr() + offset * sz,
       t_ins.data_ptr() + offset if inside else 0, u8)
    torch.cuda.synchronize()
    out, ins = t_out.cpu().numpy(), t_ins.cpu().numpy()
    assert (out[:offset] == 77).all() and (ins[:offset] == 9).all(), "nothing is written ahead of the base"
    if not inside:
        assert (ins == 9).all()
    return out[offset:].reshape(F, H, W), ins[offset:].reshape(F, H, W)


def _frames(F, H, W, dtype, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.random((F, H, W)) * 255
    return np.rint(f).astype(np.uint8) if dtype == np.uint8 else f.astype(np.float32)


def _maps(H, W):
    """the identity, an integer translation, a general projective map, one whose w crosses zero inside the frame, one with
    a NaN coefficient, one with m8 = 2: (6, 9) float64"""
    general = [1.02, -0.03, 0.7, 0.04, 0.97, -0.6, 0.3 / W, -0.2 / H, 1.0]
    crossing = [1, 0, 0, 0, 1, 0, -2.0 / W, 0.3 / H, 1.0]
    nan = [1, 0, 0, 0, np.nan, 0, 0, 0, 1.0]
    return np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1.0], [1, 0, 1, 0, 1, -1, 0, 0, 1.0], general, crossing, nan, [2, 0, 1, 0, 2, 0, 0, 0, 2.0]])


# (12, 264): a row length that is a multiple of a lane's four pixels (the vector stores) and wider than one block's 256 pixels
SHAPES = [(2, 2), (5, 7), (33, 65), (64, 129), (12, 264)]


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_the_warp_equals_the_model(H, W, dtype):
    maps = _maps(H, W)
    for F in (1, 2, 3):
        fr = _frames(F, H, W, dtype, seed=F)
        for first in range(0, len(maps), F):
            m = maps[[(first + k) % len(maps) for k in range(F)]]
            want = HM.warp(fr, m)
            for inside in (True, False):
                for offset in ((0, 1) if F == 1 else (0,)):   # offset 1: bases that are not aligned to a lane's store
                    got = _warp_device(fr, m, inside, offset)
                    SM.same(got[0], want[0], f"F={F} maps from {first} inside={inside} offset={offset}: samples")
                    if inside:
                        SM.same(got[1], want[1], f"F={F} maps from {first} offset={offset}: inside")
    x = HM.warp(_frames(1, H, W, dtype), maps[3:4])[1]
    if W > 2:
        assert 0 < x.sum() < x.size, "w crosses zero inside the frame"


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_a_third_row_of_0_0_1_gives_the_affine_warp_s_bytes(dtype):
    for H, W in SHAPES[1:]:
        fr = _frames(3, H, W, dtype, seed=3)
        aff = np.array([[1.01, -0.03, 0.6, 0.02, 0.99, -0.4], [1, 0, 2, 0, 1, -1], [0.5, 0.25, 1.125, -0.25, 0.5, 3.0]])
        persp = np.concatenate([aff, np.tile([0.0, 0.0, 1.0], (3, 1))], 1)
        a, b = _warp_device(fr, aff, affine=True), _warp_device(fr, persp)
        SM.same(b[0], a[0], f"{H} x {W}: samples")
        SM.same(b[1], a[1], f"{H} x {W}: inside")
        assert 0 < a[1].sum() < a[1].size


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_the_host_forms_over_a_chunk_boundary_equal_the_device_form(dtype):
    import lucas_kanade_core as K

    F, H, W = 65, 9, 12   # chunks of at most 64 frames: 64 + 1
    fr = _frames(F, H, W, dtype, seed=8)
    base = _maps(H, W)
    maps = base[np.arange(F) % len(base)].copy()
    maps[:, 2] += np.arange(F) * 0.125
    dev = _warp_device(fr, maps)
    out, ins = K.warp_perspective(fr, maps.reshape(F, 3, 3), return_inside=True)
    SM.same(out, dev[0], "host samples")
    SM.same(ins.astype(np.uint8), dev[1], "host inside")
    SM.same(K.warp_perspective(fr, maps), dev[0], "without inside")
    one = K.warp_perspective(fr[64], maps[64].reshape(3, 3))
    assert one.shape == (H, W)
    SM.same(one, dev[0][64], "the frame after the boundary, alone")
    SM.same(dev[0], HM.warp(fr, maps)[0], "device against the model")
