"""GPU tests of the video mosaic (run on an MI355X: python -m pytest tests/test_gpu_mosaic.py -m gpu -q).

Every output of oflk_mosaic_chain, oflk_mosaic_accumulate + oflk_mosaic_resolve and their host and sequence forms must equal the
statement (tests/mosaic_model.py) byte for byte; a NaN equals a NaN.  No tolerance anywhere but in the one end-to-end accuracy
case.  The model has no cull, so equality on the scenes below -- frames that graze a tile, lie on its closed boundary, lie far
away, cross w = 0 inside a tile, are not finite or huge -- is the whole test of the kernel's cull.
"""
import numpy as np
import pytest

import homography_model as HM
import mosaic_model as M
import stabilize_model as SM

pytestmark = pytest.mark.gpu

# The end-to-end case below: the mean absolute difference (grey levels) between the feathered mosaic of 16 tracked frames and
# the image they were cut from, measured on an MI355X with this commit; the gate is four times that.
PAN_MOSAIC_MAD = 0.3307

BLENDS = [("mean", M.MEAN), ("feather", M.FEATHER), ("first", M.FIRST), ("last", M.LAST)]
TILE_W, TILE_H = 64, 16   # the accumulate kernel's block tile (a wave's is 64 x 4)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def _chain_device(model, counts, T, anchor, H, W, extent, held=True):
    import torch

    import _oflk

    d = "cuda:0"
    S = T - 1
    t_model = torch.from_numpy(np.ascontiguousarray(model, np.float32).reshape(S, 9)).to(d) if S else None
    t_counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(d) if counts is not None and S else None
    fr, to = torch.full((T, 9), -7.0, dtype=torch.float64, device=d), torch.full((T, 9), -7.0, dtype=torch.float64, device=d)
    box = torch.full((T, 4), -7.0, dtype=torch.float64, device=d)
    t_held, t_drop = torch.full((max(S, 1),), 9, dtype=torch.uint8, device=d), torch.full((T,), 9, dtype=torch.uint8, device=d)
    _oflk.mosaic_chain(t_model.data_ptr() if S else 0, 0 if t_counts is None else t_counts.data_ptr(), T, anchor, H, W, extent,
                       fr.data_ptr(), to.data_ptr(), box.data_ptr(), t_held.data_ptr() if held else 0, t_drop.data_ptr())
    torch.cuda.synchronize()
    h = t_held.cpu().numpy()
    if not held:
        assert (h == 9).all()
    return fr.cpu().numpy(), to.cpu().numpy(), box.cpu().numpy(), h[:S], t_drop.cpu().numpy()


def _chain_scene(T, seed):
    """T-1 planted steps with held ones (status 0, a NaN, a singular model) and, from T = 9 on, one that throws its tail out"""
    rng = np.random.default_rng(seed)
    S = T - 1
    model = M.planted_steps(S, seed, scale=2.0)
    counts = np.ones((S, 3), np.int32)
    if S >= 1:
        counts[0, :2] = (37, 50)
    if S >= 8:
        counts[2, 2] = 0
        model[3, int(rng.integers(9))] = np.nan
        model[5] = [1, 2, 0, 2, 4, 0, 0, 0, 1]
        model[6] = [1, 0, 0, 0, 1, 0, 0.01, 0, 1]   # the far corners land behind the camera
    if S >= 100:
        model[90] = M.translation(1e5, 0)
        model[40, 4] = np.inf
    return model, counts


def _same_chain(got, want, what):
    for g, w, name in zip(got, want, ("from_anchor", "to_anchor", "box", "held", "dropped")):
        SM.same(g, w, f"{what}: {name}")


@pytest.mark.parametrize("T", [1, 2, 9, 130])
def test_the_chain_equals_the_model(T):
    import _oflk

    H, W = 120, 160
    model, counts = _chain_scene(T, T)
    anchors = range(T) if T <= 9 else (0, 64, 100, 129)
    dropped_any = False
    for anchor in anchors:
        for cnt in (counts, None):
            want = M.chain(model, cnt, T, anchor, H, W, 8.0 * W)
            _same_chain(_chain_device(model, cnt, T, anchor, H, W, 8.0 * W), want, f"T={T} anchor={anchor} device")
            got = _oflk.mosaic_chain_host(model, cnt, T, anchor, H, W, 8.0 * W)
            _same_chain(got, want, f"T={T} anchor={anchor} host")
            dropped_any = dropped_any or want[4].any()
            if T > 1:
                assert _oflk.mosaic_canvas(want[2], want[4]) == M.canvas(want[2], want[4])
    assert dropped_any == (T >= 9)
    want = M.chain(model, counts, T, 0, H, W, 50.0)   # an extent that only the anchor meets
    got = _chain_device(model, counts, T, 0, H, W, 50.0, held=False)   # held is not asked for and stays as it was preset
    _same_chain(got[:3] + (want[3], got[4]), want, f"T={T} small extent, no held")
    assert want[4].sum() == T - 1


def test_the_python_chain_returns_the_model_and_its_canvas():
    import lucas_kanade_core as K

    model, counts = _chain_scene(9, 4)
    want = M.chain(model, counts, 9, 4, 90, 120, 8.0 * 120)
    c = K.mosaic_chain(model.reshape(8, 3, 3), counts[:, 2], (90, 120), anchor=4)
    _same_chain((c.from_anchor.reshape(9, 9), c.to_anchor.reshape(9, 9), c.box, c.held.astype(np.uint8), c.dropped.astype(np.uint8)), want,
                "mosaic_chain")
    x0, y0, Wc, Hc = M.canvas(want[2], want[4])
    assert c.origin == (x0, y0) and c.canvas_shape == (Hc, Wc)
    one = K.mosaic_chain(np.zeros((0, 3, 3), np.float32), None, (6, 8))
    assert one.origin == (0, 0) and one.canvas_shape == (6, 8) and one.held.size == 0 and not one.dropped[0]


# ---------------------------------------------------------------------------------------------------------------------
# accumulate and resolve
# ---------------------------------------------------------------------------------------------------------------------
def _frames(F, H, W, dtype, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.random((F, H, W)) * 255
    return np.rint(f).astype(np.uint8) if dtype == np.uint8 else f.astype(np.float32)


class _Canvas:
    """the device form on one canvas: the state cleared with zero bytes (and fenced), outputs preset with bytes that the call
    must overwrite, their bases `offset` elements past an allocation's start"""

    def __init__(self, Hc, Wc, x0, y0, u8, offset=0):
        import torch

        import _oflk

        self.Hc, self.Wc, self.x0, self.y0, self.u8, self.offset = Hc, Wc, x0, y0, u8, offset
        self.bytes = _oflk.mosaic_state_bytes(Hc, Wc)
        self.state = torch.full((self.bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.out = torch.full((Hc * Wc + offset,), 77, dtype=torch.uint8 if u8 else torch.float32, device="cuda:0")
        self.count = torch.full((Hc * Wc + offset,), -3, dtype=torch.int32, device="cuda:0")
        self.keep = []
        self.clear()

    def clear(self):
        self.state[:self.bytes].zero_()

    def add(self, frames, maps, skip, blend, stream=0):
        import torch

        import _oflk

        F, H, W = frames.shape
        t_in = torch.from_numpy(np.ascontiguousarray(frames)).to("cuda:0")
        t_map = torch.from_numpy(np.ascontiguousarray(maps, np.float64).reshape(F, 9)).to("cuda:0")
        t_skip = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, np.uint8)).to("cuda:0")
        self.keep += [t_in, t_map, t_skip]
        _oflk.mosaic_accumulate(t_in.data_ptr(), F, H, W, t_map.data_ptr(), 0 if t_skip is None else t_skip.data_ptr(), self.x0, self.y0,
                                self.Hc, self.Wc, blend, self.state.data_ptr(), self.bytes, self.u8, stream)

    def resolve(self, count=True, stream=0):
        import _oflk

        _oflk.mosaic_resolve(self.state.data_ptr(), self.Hc, self.Wc, self.out.data_ptr() + self.offset * self.out.element_size(),
                             self.count.data_ptr() + 4 * self.offset if count else 0, self.u8, stream)

    def read(self, count=True):
        import torch

        torch.cuda.synchronize()
        out, cnt = self.out.cpu().numpy(), self.count.cpu().numpy()
        assert (out[:self.offset] == 77).all() and (cnt[:self.offset] == -3).all(), "nothing is written ahead of the base"
        assert (self.state[self.bytes:] == 0xA5).all().item(), "nothing is written past the state"
        if not count:
            assert (cnt == -3).all()
        return out[self.offset:].reshape(self.Hc, self.Wc), cnt[self.offset:].reshape(self.Hc, self.Wc)


def _device(frames, maps, skip, x0, y0, Hc, Wc, blend, cuts=(), offset=0, count=True):
    c = _Canvas(Hc, Wc, x0, y0, frames.dtype == np.uint8, offset)
    edges = [0, *cuts, frames.shape[0]]
    for lo, hi in zip(edges[:-1], edges[1:]):
        c.add(frames[lo:hi], maps[lo:hi], None if skip is None else skip[lo:hi], blend)
    c.resolve(count)
    return c.read(count)


def _maps(F, H, W, x0, y0, Hc, Wc, seed):
    """F maps from canvas coordinates, drawn in turn from the kinds that matter to the cull and to the blend, each moved on a
    little from one use to the next: (maps (F, 9), skip (F,))"""
    rng = np.random.default_rng(seed)
    edge = x0 + TILE_W   # the map coordinate of the first column of the second tile
    mid = x0 + TILE_W / 2 + 0.5
    kinds = [
        lambda j: M.translation(-(x0 + j % max(Wc - 1, 1)), -(y0 + j % max(Hc - 1, 1))),                    # integer translations
        lambda j: M.translation(-(x0 - 1.25 + 0.37 * j), -(y0 - 0.5 + 0.21 * j)),                           # sub-pixel translations
        lambda j: HM.planted_homography() * [1, 1, 0, 1, 1, 0, 4, 4, 1] + M.translation(-x0 - 0.1 * j, -y0 + 0.3 * j) - M.IDENTITY,
        lambda j: M.translation(-(edge + 0.5 - (W - 1)) - 0.001 * j, -y0),     # reaches into the second tile by less than a pixel
        lambda j: M.translation(-(edge - (W - 1)), -(y0 + j % 3)),             # column `edge` exactly on the closed boundary xs == W-1
        lambda j: M.translation(-(x0 + Wc - 1), -(y0 + Hc - 1)),               # only the canvas's last pixel, at the frame's (0, 0)
        lambda j: M.translation(1e6 + j, -3e5),                                # far outside
        lambda j: np.array([0, 0, 3.0, 0, 0, 2.0, 0.05, 0.001 * j, -0.05 * mid]),   # w = 0 crosses the first tile through its middle
        lambda j: np.array([1, 0, -x0, 0, 1, -y0, 0, 0, -1.0]),                # w < 0 everywhere
        lambda j: np.array([1, 0, -x0, 0, np.nan, -y0, 0, 0, 1.0]),            # a NaN coefficient
        lambda j: np.array([1e150, 0, -1e150 * x0, 0, 1e150, -1e150 * y0, 0, 0, 1e150]),   # coefficients near 1e150
        lambda j: np.array([1, 0, -x0, 0, 1, -y0, 0, 0, 1.0]) * 1e150 * [1, 1, 1, 1, 1, 1, 0, 0, 1e-150],
        lambda j: np.array([0.5, 0.1, -0.5 * x0 + 1, -0.1, 0.5, -0.5 * y0 + 2 + 0.1 * j, 1e-3, -1e-3, 1.0]),   # a zoom: many frames deep
    ]
    order = rng.permutation(len(kinds)) if F >= len(kinds) else rng.permutation(len(kinds))[:F]
    maps = np.stack([kinds[order[f % len(order)]](f // len(order)) for f in range(F)]).astype(np.float64)
    skip = (rng.random(F) < 0.15).astype(np.uint8)
    return maps, skip


# frame size, canvas size, origin, number of frames: canvases one less and one more than the block tile of 64 x 16 and than a
# wave's 64 x 4, a multiple of neither, one pixel high, one pixel wide; origins of both signs; F past one and two groups of 64
CASES = [((9, 13), (TILE_H - 1, TILE_W - 1), (-7, 3), 1),
         ((9, 13), (TILE_H + 1, TILE_W + 1), (5, -4), 2),
         ((5, 64), (1, 2 * TILE_W + 7), (-70, -2), 65),
         ((6, 257), (37, 1), (100, -20), 65),
         ((33, 100), (TILE_H, TILE_W), (0, 0), 2),
         ((9, 13), (5, TILE_W + 4), (-3, -3), 130),
         ((33, 100), (3 * TILE_H + 3, 3 * TILE_W - 2), (-40, 11), 130)]


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("blend", BLENDS, ids=[b[0] for b in BLENDS])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_accumulate_and_resolve_equal_the_model(case, blend, dtype):
    (H, W), (Hc, Wc), (x0, y0), F = CASES[case]
    frames = _frames(F, H, W, dtype, seed=case)
    maps, skip = _maps(F, H, W, x0, y0, Hc, Wc, seed=case)
    what = f"case {case} {blend[0]}"
    for sk in (skip, None):
        want = M.composite(frames, maps, sk, x0, y0, Hc, Wc, blend[1])
        for offset in (0, 1):   # offset 1: outputs that are not aligned to a lane's store
            got = _device(frames, maps, sk, x0, y0, Hc, Wc, blend[1], offset=offset)
            SM.same(got[0], want[0], f"{what} offset={offset} skip={sk is not None}: canvas")
            SM.same(got[1], want[1], f"{what} offset={offset} skip={sk is not None}: count")
        if F >= 65 and sk is None:
            assert want[1].max() >= 20, "the frames lie many deep"
    got = _device(frames, maps, skip, x0, y0, Hc, Wc, blend[1], count=False)
    SM.same(got[0], M.composite(frames, maps, skip, x0, y0, Hc, Wc, blend[1])[0], f"{what}: without count")
    for k in (1, 64, 65):
        if k < F:
            got = _device(frames, maps, skip, x0, y0, Hc, Wc, blend[1], cuts=(k,))
            want = M.composite(frames, maps, skip, x0, y0, Hc, Wc, blend[1])
            SM.same(got[0], want[0], f"{what} cut at {k}: canvas")
            SM.same(got[1], want[1], f"{what} cut at {k}: count")


def test_the_scenes_hold_what_they_promise():
    """the kinds of _maps do what their comments say, on the model: a sliver under a pixel wide, the closed boundary, w = 0 inside
    the first tile"""
    (H, W), (Hc, Wc), (x0, y0), _ = CASES[1]
    f = np.full((1, H, W), 200, np.uint8)
    edge = x0 + TILE_W
    sliver = M.composite(f, M.translation(-(edge + 0.5 - (W - 1)), -y0)[None], None, x0, y0, Hc, Wc, M.MEAN)[1]
    assert sliver[:, TILE_W].any() and not sliver[:, TILE_W + 1:].any()
    closed = M.composite(f, M.translation(-(edge - (W - 1)), -y0)[None], None, x0, y0, Hc, Wc, M.MEAN)[1]
    assert closed[:, TILE_W].any() and not closed[:, TILE_W + 1:].any()
    mid = x0 + TILE_W / 2 + 0.5
    cross = M.composite(f, np.array([[0, 0, 3.0, 0, 0, 2.0, 0.05, 0, -0.05 * mid]]), None, x0, y0, Hc, Wc, M.MEAN)[1]
    assert cross[:, TILE_W // 2 + 1:TILE_W].any() and not cross[:, :TILE_W // 2 + 1].any()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_one_frame_on_its_own_canvas_is_the_library_s_perspective_warp(dtype):
    import torch

    import _oflk

    H, W = 33, 100
    frame = _frames(1, H, W, dtype, seed=21)
    for m in [np.array([1.02, -0.03, 0.7, 0.04, 0.97, -0.6, 0.3 / W, -0.2 / H, 1.0]), M.translation(2.5, -1.25),
              np.array([1, 0, 0, 0, 1, 0, -2.0 / W, 0.3 / H, 1.0])]:
        t_in = torch.from_numpy(frame).to("cuda:0")
        t_map = torch.from_numpy(m[None].copy()).to("cuda:0")
        t_out, t_ins = torch.empty_like(t_in), torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda:0")
        _oflk.warp_perspective(t_in.data_ptr(), 1, H, W, t_map.data_ptr(), t_out.data_ptr(), t_ins.data_ptr(), dtype == np.uint8)
        torch.cuda.synchronize()
        warped, inside = t_out.cpu().numpy()[0], t_ins.cpu().numpy()[0]
        assert 0 < inside.sum()
        for _, blend in BLENDS:
            got = _device(frame, m[None], None, 0, 0, H, W, blend)
            SM.same(got[0], warped, f"blend {blend}: the warp's samples")
            SM.same(got[1], inside.astype(np.int32), f"blend {blend}: the warp's inside")


def test_resolve_leaves_the_state_as_it_was():
    frames, (maps, skip) = _frames(5, 9, 13, np.float32, 2), _maps(5, 9, 13, -3, 2, 21, 70, 6)
    c = _Canvas(21, 70, -3, 2, False)
    c.add(frames, maps, None, M.FEATHER)
    import torch

    torch.cuda.synchronize()
    before = c.state.cpu().numpy().copy()
    c.resolve()
    first = c.read()
    assert np.array_equal(c.state.cpu().numpy(), before)
    c.resolve()
    again = c.read()
    SM.same(again[0], first[0], "a second resolve")
    SM.same(first[0], M.composite(frames, maps, None, -3, 2, 21, 70, M.FEATHER)[0], "the first")


def test_clear_accumulate_resolve_replay_from_a_graph_on_new_frames():
    """captured once after one eager call and replayed on new frame contents (the process keeps the default number of hardware
    queues); the outputs are scribbled over between replays"""
    import torch

    F, H, W, Hc, Wc, x0, y0 = 7, 9, 13, 21, 70, -3, 2
    maps, skip = _maps(F, H, W, x0, y0, Hc, Wc, 9)
    c = _Canvas(Hc, Wc, x0, y0, True)
    t_in = torch.zeros((F, H, W), dtype=torch.uint8, device="cuda:0")
    t_map, t_skip = torch.from_numpy(maps).to("cuda:0"), torch.from_numpy(skip).to("cuda:0")

    def enqueue(stream):
        import _oflk

        c.state[:c.bytes].zero_()
        _oflk.mosaic_accumulate(t_in.data_ptr(), F, H, W, t_map.data_ptr(), t_skip.data_ptr(), x0, y0, Hc, Wc, M.FEATHER,
                                c.state.data_ptr(), c.bytes, True, stream)
        c.resolve(True, stream)

    fr = _frames(F, H, W, np.uint8, 30)
    t_in.copy_(torch.from_numpy(fr))
    enqueue(torch.cuda.current_stream().cuda_stream)
    want = M.composite(fr, maps, skip, x0, y0, Hc, Wc, M.FEATHER)
    got = c.read()
    SM.same(got[0], want[0], "eager: canvas")
    SM.same(got[1], want[1], "eager: count")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        fr = _frames(F, H, W, np.uint8, 31 + rep)
        t_in.copy_(torch.from_numpy(fr))
        c.out.fill_(77)
        c.count.fill_(-3)
        g.replay()
        want = M.composite(fr, maps, skip, x0, y0, Hc, Wc, M.FEATHER)
        got = c.read()
        SM.same(got[0], want[0], f"replay {rep}: canvas")
        SM.same(got[1], want[1], f"replay {rep}: count")
    del g


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_the_host_forms_over_a_chunk_boundary_equal_the_device_form(dtype):
    import lucas_kanade_core as K

    F, H, W, Hc, Wc, x0, y0 = 65, 9, 13, 19, 70, -5, 1   # chunks of at most 64 frames: 64 + 1
    frames = _frames(F, H, W, dtype, seed=8)
    maps, skip = _maps(F, H, W, x0, y0, Hc, Wc, 12)
    for name, blend in BLENDS:
        dev = _device(frames, maps, skip, x0, y0, Hc, Wc, blend)
        out, cnt = K.mosaic_composite(frames, maps.reshape(F, 3, 3), (Hc, Wc), (x0, y0), skip, name, return_count=True)
        SM.same(out, dev[0], f"{name}: host canvas")
        SM.same(cnt, dev[1], f"{name}: host count")
    SM.same(K.mosaic_composite(frames, maps, (Hc, Wc), (x0, y0), skip.astype(bool), "last"), dev[0], "without count")
    dev = _device(frames, maps, None, x0, y0, Hc, Wc, M.MEAN)
    SM.same(K.mosaic_composite(frames, maps, (Hc, Wc), (x0, y0)), dev[0], "the defaults: mean, no skip")


# ---------------------------------------------------------------------------------------------------------------------
# the sequence call
# ---------------------------------------------------------------------------------------------------------------------
def _pan(T, H, W, step, seed):
    image = M.smooth_field(H + 8, W + step * (T - 1) + 8, seed)
    frames, _ = M.pan_frames(image, T, H, W, step, 0, 4, 4)
    return image, frames


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_the_sequence_call_is_the_chain_of_its_four_parts(dtype):
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    _, frames = _pan(12, 96, 128, 5, 3)
    frames = frames.astype(dtype)
    kw = dict(max_corners=300, detect_every=4)
    got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, threshold=1.0, seed=5, anchor=3, blend="feather", **kw)
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, **kw)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born, 128, 1.0, seed=5, t0=0)
    chain = K.mosaic_chain(fit.model, fit.status, (96, 128), anchor=3)
    canvas, count = K.mosaic_composite(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", return_count=True)
    assert got.origin == chain.origin and got.canvas.shape == chain.canvas_shape and got.canvas.dtype == dtype
    SM.same(got.canvas, canvas, "canvas")
    SM.same(got.count, count, "count")
    SM.same(got.to_anchor, chain.to_anchor, "to_anchor")
    SM.same(got.model, fit.model, "model")
    assert np.array_equal(got.status, fit.status) and np.array_equal(got.held, chain.held) and np.array_equal(got.dropped, chain.dropped)
    assert got.status.all() and count.max() >= 6 and got.canvas.shape[1] > 128 + 40


def test_the_capacity_refusal_reports_the_canvas_it_needed():
    import ctypes

    import _oflk
    import lucas_kanade_pyramidal as P

    _, frames = _pan(6, 96, 128, 5, 3)
    ok = P.lucas_kanade_pyramidal_sequence_mosaic(frames, max_corners=300)
    Hc, Wc = ok.canvas.shape
    with pytest.raises(_oflk.OflkError) as e:
        P.lucas_kanade_pyramidal_sequence_mosaic(frames, max_corners=300, max_pixels=Hc * Wc - 1)
    assert e.value.code == _oflk.OFLK_ERR_UNSUPPORTED and f"{Wc} x {Hc}" in str(e.value)
    out, canvas = np.full(Hc * Wc - 1, 77, np.uint8), np.full(4, -1, np.int32)
    rc = _oflk.lib().oflk_mosaic_sequence_u8(frames.ctypes.data, 6, 96, 128, 3, 5, 3, 0.01, 0.5, 4.0, 0.01, 10.0, 300, 4, 256, 1.0, 0, 0,
                                             8.0 * 128, M.FEATHER, out.ctypes.data, Hc * Wc - 1, canvas.ctypes.data_as(_oflk._i32p), None,
                                             None, None, None, None, None)
    assert rc == _oflk.OFLK_ERR_UNSUPPORTED and (out == 77).all()
    assert tuple(canvas) == (ok.origin[0], ok.origin[1], Wc, Hc)
    assert ctypes.sizeof(ctypes.c_size_t) == 8


def test_a_tracked_pan_gives_the_picture_the_frames_were_cut_from():
    """16 frames of 120 x 160 cut 6 px apart from one textured image: the feathered mosaic against the image, where frames
    cover it and 2 px away from the rim of the covered region.  Measured on an MI355X with this commit: 0.3307 grey levels over
    28 242 pixels of a 250 x 122 canvas at (0, -1) (PAN_MOSAIC_MAD); the gate is four times that.  No frame may be dropped or
    held."""
    import lucas_kanade_pyramidal as P

    image, frames = _pan(16, 120, 160, 6, 17)
    got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, max_corners=500, detect_every=4, anchor=0, blend="feather")
    assert not got.dropped.any() and not got.held.any() and got.status.all()
    Hc, Wc = got.canvas.shape
    x0, y0 = got.origin
    src = np.zeros((Hc, Wc))
    known = np.zeros((Hc, Wc), bool)
    ys, xs = np.arange(Hc) + y0 + 4, np.arange(Wc) + x0 + 4   # the anchor frame was cut at (4, 4)
    oy, ox = (ys >= 0) & (ys < image.shape[0]), (xs >= 0) & (xs < image.shape[1])
    src[np.ix_(oy, ox)] = image[np.ix_(ys[oy], xs[ox])]
    known[np.ix_(oy, ox)] = True
    cover = (got.count > 0) & known
    core = cover.copy()
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            core &= np.roll(np.roll(cover, dy, 0), dx, 1)
    core[:2], core[-2:], core[:, :2], core[:, -2:] = False, False, False, False
    mad = float(np.abs(got.canvas.astype(np.float64) - src)[core].mean())
    print(f"pan mosaic: canvas {Wc} x {Hc} at {got.origin}, {int(core.sum())} pixels compared, mean absolute difference {mad:.4g}")
    assert core.sum() > 0.9 * 120 * (160 + 15 * 6 - 8) and Wc >= 160 + 15 * 6 - 2
    assert mad <= 4 * PAN_MOSAIC_MAD
