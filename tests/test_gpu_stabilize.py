"""GPU tests of video stabilisation (run on an MI355X: python -m pytest tests/test_gpu_stabilize.py -m gpu -q).

oflk_stabilize_trajectory, oflk_warp_affine, their host forms and oflk_stabilize_sequence must equal the statement
(tests/stabilize_model.py) byte for byte; a NaN equals a NaN.  No tolerance anywhere.
"""
import numpy as np
import pytest

import motion_model as MM
import stabilize_model as SM
from test_gpu_motion import _tracks_device
from test_gpu_sparse_replenish import _call
from test_stabilize_cpu import SCENE, scene

pytestmark = pytest.mark.gpu

FAMILIES = [MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE]


# ---------------------------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------------------------
def _trajectory_device(model, counts, T, w, held=True, stream=0):
    """the device form, every output preset with bytes that it must overwrite"""
    import torch

    import _oflk

    d = "cuda:0"
    t_model = torch.from_numpy(np.ascontiguousarray(model, np.float32)).to(d) if T > 1 else None
    t_counts = None if counts is None or T < 2 else torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(d)
    corr = torch.full((T, 6), -7.0, device=d)
    mp = torch.full((T, 6), -7.0, dtype=torch.float64, device=d)
    hd = torch.full((max(T - 1, 1),), 9, dtype=torch.uint8, device=d)
    _oflk.stabilize_trajectory(t_model.data_ptr() if T > 1 else 0, 0 if t_counts is None else t_counts.data_ptr(), T, w,
                               corr.data_ptr(), mp.data_ptr(), hd.data_ptr() if held else 0, stream)
    torch.cuda.synchronize()
    return corr.cpu().numpy(), mp.cpu().numpy(), hd.cpu().numpy()[:T - 1]


def _warp_device(frames, maps, inside=True, offset=0):
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
    t_map = torch.from_numpy(np.ascontiguousarray(maps, np.float64).reshape(F, 6)).to(d)
    sz = frames.itemsize
    _oflk.warp_affine(t_in.data_ptr() + offset * sz, F, H, W, t_map.data_ptr(), t_out.data_ptr() + offset * sz,
                      t_ins.data_ptr() + offset if inside else 0, u8)
    torch.cuda.synchronize()
    out, ins = t_out.cpu().numpy(), t_ins.cpu().numpy()
    assert (out[:offset] == 77).all() and (ins[:offset] == 9).all(), "nothing is written ahead of the base"
    if not inside:
        assert (ins == 9).all()
    return out[offset:].reshape(F, H, W), ins[offset:].reshape(F, H, W)


def _spoil(model, counts, seed):
    """some steps with status 0, NaN coefficients or a zero determinant (as many as the number of steps allows)"""
    rng = np.random.default_rng(seed)
    model, counts = model.copy(), counts.copy()
    S = len(model)
    steps = rng.permutation(S)[:min(S, 4) if S > 2 else 1]
    for i, s in enumerate(steps):
        if i % 4 == 0:
            counts[s, 2] = 0
        elif i % 4 == 1:
            model[s, rng.integers(6)] = np.nan
        elif i % 4 == 2:
            model[s] = np.float32([2, 4, 1, 1, 2, 3])
        else:
            model[s] = 0
    return model, counts


# ---------------------------------------------------------------------------------------------------------------------
# the trajectory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 3, 64])
@pytest.mark.parametrize("T", [1, 2, 3, 7, 8, 130])
def test_the_trajectory_equals_the_model(T, r):
    w = SM.weights(r)
    for fam in FAMILIES:
        model = SM.noisy_models(T - 1, fam, 10 * T + r)
        counts = np.tile(np.int32([30, 40, 1]), (T - 1, 1))
        if T > 1:
            model, counts = _spoil(model, counts, T + r + fam)
        for c in ((counts, None) if fam == MM.SIMILARITY else (counts,)):
            want = SM.trajectory(model, c, T, w)
            got = _trajectory_device(model, c, T, w)
            for g, x, name in zip(got, want, ("correction", "map", "held")):
                SM.same(g, x, f"T={T} r={r} family {fam} counts={'given' if c is not None else 'NULL'}: {name}")
            if T > 2 and c is not None:
                assert want[2].any(), "a step is held"
    got = _trajectory_device(model, counts, T, w, held=False)   # the last family's models, with counts
    assert (got[2] == 9).all(), "a NULL held is not written"
    SM.same(got[0], want[0], "with a NULL held")
    SM.same(got[1], want[1], "with a NULL held: map")


def test_a_constant_pan_is_the_identity_on_the_device_too():
    T = 12
    model = np.tile(np.float32([1, 0, 3, 0, 1, -2]), (T - 1, 1))
    corr, mp, held = _trajectory_device(model, None, T, SM.weights(3))
    ident = np.tile(SM.IDENTITY, (T, 1))
    SM.same(corr, ident.astype(np.float32), "correction, bit for bit")
    assert np.array_equal(mp, ident) and not held.any()


def test_the_host_trajectory_equals_the_device_form():
    import _oflk
    import lucas_kanade_core as K

    for T, r in [(1, 3), (2, 2), (9, 3), (40, 15)]:
        model = SM.noisy_models(T - 1, MM.AFFINE, T)
        counts = np.tile(np.int32([30, 40, 1]), (T - 1, 1))
        if T > 2:
            model, counts = _spoil(model, counts, T)
        w = SM.weights(r)
        for c in (None, counts):
            dev = _trajectory_device(model, c, T, w)
            host = _oflk.stabilize_trajectory_host(model, c, T, w)
            for g, x, name in zip(host, dev, ("correction", "map", "held")):
                SM.same(g, x, f"T={T}: host against device, {name}")
            for g, x, name in zip(dev, SM.trajectory(model, c, T, w), ("correction", "map", "held")):
                SM.same(g, x, f"T={T}: device against the model, {name}")
        t = K.stabilize_trajectory(model.reshape(-1, 2, 3), counts[:, 2], radius=r)
        assert t.correction.shape == (T, 2, 3) and t.map.shape == (T, 2, 3) and t.held.dtype == bool and t.held.shape == (T - 1,)
        SM.same(t.correction.reshape(T, 6), dev[0], "stabilize_trajectory")
        SM.same(t.map.reshape(T, 6), dev[1], "stabilize_trajectory: map")
        assert np.array_equal(t.held, dev[2].astype(bool))


# ---------------------------------------------------------------------------------------------------------------------
# the warp
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (5, 7), (37, 53), (33, 260), (64, 256)]


def _maps(H, W):
    """nine maps, three batches of three frames"""
    th = np.deg2rad(30.0)
    c, s = np.cos(th), np.sin(th)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return np.array([
        [1, 0, 0, 0, 1, 0],                                            # the identity
        [1, 0, 3, 0, 1, -2],                                           # an integer shift
        [1, 0, 0.5, 0, 1, 0],                                          # half a pixel
        [c, -s, cx - (c * cx - s * cy), s, c, cy - (s * cx + c * cy)],  # 30 degrees about the centre
        [0.5, 0, 0, 0, 0.5, 0],                                        # scales
        [2, 0, 0, 0, 2, 0],
        [1, 0, W + 5, 0, 1, 0],                                        # every pixel outside
        [-1, 0, W - 1, 0, -1, H - 1],                                  # lands exactly on W-1 and H-1 (and on 0)
        [1, 0, -1e-9, 0, 1, -1e-9],                                    # the first row and column at -1e-9
    ], np.float64)


def _frames(dtype, F, H, W, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    return (rng.random((F, H, W)) * 255).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float32", "uint8"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_the_warp_equals_the_model(H, W, dtype):
    frames = _frames(dtype, 3, H, W, H * W)
    maps = _maps(H, W)
    for b in range(3):
        m = maps[3 * b:3 * b + 3]
        want, want_in = SM.warp(frames, m)
        for offset in (0, 1):
            got, got_in = _warp_device(frames, m, True, offset)
            SM.same(got, want, f"{H}x{W} batch {b} offset {offset}")
            SM.same(got_in, want_in, f"{H}x{W} batch {b} offset {offset}: inside")
            got, _ = _warp_device(frames, m, False, offset)
            SM.same(got, want, f"{H}x{W} batch {b} offset {offset}, NULL inside")
        if b == 0:
            assert np.array_equal(want[0], frames[0]) and want_in[0].all(), "the identity returns the frame"
        if b == 2:
            assert not want[0].any() and not want_in[0].any(), "every pixel outside: zeros"
            assert np.array_equal(want[1], frames[1][::-1, ::-1]) and want_in[1].all(), "exactly on the last row and column"
            assert not want_in[2][0].any() and not want_in[2][:, 0].any() and want_in[2][1:, 1:].all(), "-1e-9 is outside"


def test_half_pixel_samples_of_bytes_round_to_even():
    row = np.uint8([1, 2, 3, 2, 0, 1, 2, 3])
    frames = np.tile(row, (1, 4, 1))
    m = np.array([[1, 0, 0.5, 0, 1, 0]], np.float64)
    got, ins = _warp_device(frames, m)
    assert got[0, 0].tolist() == [2, 2, 2, 1, 0, 2, 2, 0], "1.5 -> 2, 2.5 -> 2, 2.5 -> 2, 1.0, 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, outside"
    SM.same(got, SM.warp(frames, m)[0], "half a pixel")
    assert ins[0, 0].tolist() == [1] * 7 + [0]


def test_more_frames_than_the_grid_has_layers_and_a_map_that_is_not_a_number():
    """F beyond the grid's 65535 layers takes the kernel's loop over frames; a NaN map is outside everywhere"""
    F = 65535 + 3
    frames = _frames(np.uint8, F, 2, 4, 1)
    maps = np.tile(SM.IDENTITY, (F, 1))
    maps[-1] = [1, 0, 1, 0, 1, 0]
    maps[-2] = [1, 0, np.nan, 0, 1, 0]
    got, ins = _warp_device(frames, maps)
    assert np.array_equal(got[:-2], frames[:-2]) and ins[:-2].all()
    assert not got[-2].any() and not ins[-2].any()
    assert np.array_equal(got[-1][:, :3], frames[-1][:, 1:]) and not got[-1][:, 3].any()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float32", "uint8"])
def test_the_host_warp_equals_the_device_form_and_does_not_depend_on_the_chunks(dtype):
    import _oflk
    import lucas_kanade_core as K

    F, H, W = 70, 24, 32   # two chunks: a chunk holds at most 64 frames
    frames = _frames(dtype, F, H, W, 5)
    rng = np.random.default_rng(6)
    maps = np.tile(SM.IDENTITY, (F, 1)) + rng.normal(0, [0.02, 0.02, 2.0, 0.02, 0.02, 2.0], (F, 6))
    out, ins = _oflk.warp_affine_host(frames, maps, True)
    dev, dev_in = _warp_device(frames, maps)
    SM.same(out, dev, "host against device")
    SM.same(ins, dev_in, "host against device: inside")
    want, want_in = SM.warp(frames[60:], maps[60:])
    SM.same(out[60:], want, "across the chunk boundary, against the model")
    SM.same(ins[60:], want_in, "across the chunk boundary, against the model: inside")
    for f in range(F):
        one, one_in = _oflk.warp_affine_host(frames[f:f + 1], maps[f:f + 1], True)
        SM.same(one[0], out[f], f"frame {f} alone")
        SM.same(one_in[0], ins[f], f"frame {f} alone: inside")
    got = K.warp_affine(frames, maps.reshape(F, 2, 3))
    SM.same(got, out, "warp_affine")
    got, gi = K.warp_affine(frames[3], maps[3], return_inside=True)
    assert got.shape == (H, W) and gi.dtype == bool
    SM.same(got, out[3], "warp_affine of one frame")
    assert np.array_equal(gi, ins[3].astype(bool))
    assert _oflk.warp_affine_host(frames[:2], maps[:2], False)[1] is None


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
def _rows_under(models, K, H, W, seed):
    """(T, K, 2) float32 rows of K points moved by the step models, a few of them off the model; all visible"""
    rng = np.random.default_rng(seed)
    T = len(models) + 1
    p = (rng.random((K, 2)) * [W - 1, H - 1]).astype(np.float32)
    rows = [p]
    for c in models.astype(np.float64):
        q = rows[-1].astype(np.float64)
        n = np.stack([c[0] * q[:, 0] + c[1] * q[:, 1] + c[2], c[3] * q[:, 0] + c[4] * q[:, 1] + c[5]], -1)
        n[rng.permutation(K)[:K // 5]] += rng.uniform(4, 9, (K // 5, 2))
        rows.append(n.astype(np.float32))
    return np.stack(rows), np.ones((T, K), np.uint8)


def test_the_device_chain_replays_from_a_graph_with_changed_inputs():
    """oflk_tracks_motion -> oflk_stabilize_trajectory -> oflk_warp_affine, a single chain on one stream, captured once after
    one eager call and replayed on other rows and frames in the same buffers (the process keeps the default number of
    hardware queues)"""
    import torch

    import _oflk

    T, K, H, W, hyps, r = 6, 60, 24, 32, 48, 2
    w = SM.weights(r)
    d = "cuda:0"
    cases = []
    for i in range(3):
        models = SM.noisy_models(T - 1, MM.SIMILARITY, 30 + i)
        tr, vis = _rows_under(models, K, H, W, 40 + i)
        if i == 2:
            vis[3] = 0   # two steps cannot be fitted: held
        frames = _frames(np.float32, T, H, W, 50 + i)
        model, _, counts = MM.tracks(tr, vis, None, MM.SIMILARITY, hyps, 1.0, 4, 0)
        corr, mp, held = SM.trajectory(model, counts, T, w)
        cases.append((tr, vis, frames, (model, counts, corr, mp, held) + SM.warp(frames, mp)))
    assert cases[2][3][4].sum() == 2 and not cases[0][3][4].any()
    t_tr, t_vis = torch.zeros((T, K, 2), device=d), torch.zeros((T, K), dtype=torch.uint8, device=d)
    t_fr = torch.zeros((T, H, W), device=d)
    nb = _oflk.motion_workspace(T - 1, K, hyps)
    ws = torch.zeros(nb, dtype=torch.uint8, device=d)
    model, inl = torch.zeros((T - 1, 6), device=d), torch.zeros((T - 1, K), dtype=torch.uint8, device=d)
    counts = torch.zeros((T - 1, 3), dtype=torch.int32, device=d)
    corr, mp = torch.zeros((T, 6), device=d), torch.zeros((T, 6), dtype=torch.float64, device=d)
    held = torch.zeros(T - 1, dtype=torch.uint8, device=d)
    out, ins = torch.zeros((T, H, W), device=d), torch.zeros((T, H, W), dtype=torch.uint8, device=d)

    def load(i):
        t_tr.copy_(torch.from_numpy(cases[i][0]))
        t_vis.copy_(torch.from_numpy(cases[i][1]))
        t_fr.copy_(torch.from_numpy(cases[i][2]))
        for t, v in ((ws, 0x3C + i), (model, -7.0), (inl, 9), (counts, -3), (corr, -7.0), (mp, -7.0), (held, 9), (out, -7.0), (ins, 9)):
            t.fill_(v)

    def enqueue(stream):
        _oflk.tracks_motion(t_tr.data_ptr(), t_vis.data_ptr(), 0, T, K, ws.data_ptr(), nb, model.data_ptr(), inl.data_ptr(),
                            counts.data_ptr(), MM.SIMILARITY, hyps, 1.0, 4, 0, stream)
        _oflk.stabilize_trajectory(model.data_ptr(), counts.data_ptr(), T, w, corr.data_ptr(), mp.data_ptr(), held.data_ptr(), stream)
        _oflk.warp_affine(t_fr.data_ptr(), T, H, W, mp.data_ptr(), out.data_ptr(), ins.data_ptr(), False, stream)

    def check(i, what):
        torch.cuda.synchronize()
        got = (model, counts, corr, mp, held, out, ins)
        for g, x, name in zip(got, cases[i][3], ("model", "counts", "correction", "map", "held", "out", "inside")):
            SM.same(g.cpu().numpy(), x, f"{what}: {name}")

    load(0)
    enqueue(0)
    check(0, "eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for rep, i in enumerate((1, 2, 0)):
        load(i)
        g.replay()
        check(i, f"replay {rep} of case {i}")
    del g


# ---------------------------------------------------------------------------------------------------------------------
# the sequence call
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ("out", "correction", "model", "counts", "held")


def _sequence(frames, K, D, q, md, family, hyps, thr, seed, w, levels=3, win=5, iters=3, optional=True):
    """the C entry point, every output preset with bytes that it must overwrite; optional=False: the last four NULL"""
    import _oflk

    frames = np.ascontiguousarray(frames)
    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    out = np.full(frames.shape, 77, frames.dtype)
    corr, model = np.full((T, 6), -7.0, np.float32), np.full((T - 1, 6), -7.0, np.float32)
    counts, held = np.full((T - 1, 3), -3, np.int32), np.full(T - 1, 9, np.uint8)
    L = _oflk.lib()
    fn = L.oflk_stabilize_sequence_u8 if u8 else L.oflk_stabilize_sequence
    w = np.ascontiguousarray(w, np.float64)
    _oflk.check(fn(frames.ctypes.data if u8 else _oflk.ptr(frames), T, H, W, levels, win, iters, 0.01, 0.5, 4.0, q, md, K, D, family, hyps,
                   thr, seed, _oflk._f64(w), len(w) - 1, out.ctypes.data if u8 else _oflk.ptr(out),
                   _oflk.ptr(corr) if optional else None, _oflk.ptr(model) if optional else None,
                   counts.ctypes.data_as(_oflk._i32p) if optional else None, held.ctypes.data if optional else None))
    return out, corr, model, counts, held


def _scene_args():
    s = SCENE
    return (s["K"], s["D"], s["q"], s["md"], s["family"], s["hyps"], s["thr"], s["seed"], SM.weights(s["r"], s["sigma"]))


def test_the_sequence_call_equals_the_chain_of_statements():
    frames, path, want = scene(0)
    got = _sequence(frames, *_scene_args())
    for g, x, name in zip(got, want, NAMES):
        SM.same(g, x, f"uint8: {name}")
    assert (want[0] != frames).any(), "the frames are moved"
    # float32 frames of the same values: the same rows, models and maps; the samples are not rounded to bytes
    f32 = frames.astype(np.float32)
    got = _sequence(f32, *_scene_args())
    _, mp, _ = SM.trajectory(want[2], want[3], len(frames), SM.weights(SCENE["r"], SCENE["sigma"]))
    for g, x, name in zip(got, (SM.warp(f32, mp)[0],) + want[1:], NAMES):
        SM.same(g, x, f"float32: {name}")
    only = _sequence(frames, *_scene_args(), optional=False)
    SM.same(only[0], want[0], "with the optional outputs NULL")
    assert (only[1] == -7.0).all() and (only[4] == 9).all()


def test_the_python_call_returns_the_same_arrays():
    import lucas_kanade_pyramidal as P

    frames, path, want = scene(0)
    s = SCENE
    got = P.lucas_kanade_pyramidal_sequence_stabilize(frames, s["K"], s["D"], model="translation", radius=s["r"], sigma=s["sigma"],
                                                      hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"], quality_level=s["q"],
                                                      min_distance=s["md"])
    T = len(frames)
    SM.same(got.frames, want[0], "frames")
    SM.same(got.correction.reshape(T, 6), want[1], "correction")
    SM.same(got.model.reshape(T - 1, 6), want[2], "model")
    assert np.array_equal(got.status, want[3][:, 2]) and np.array_equal(got.held, want[4].astype(bool)) and got.held.dtype == bool
    assert got.correction.shape == (T, 2, 3) and got.model.shape == (T - 1, 2, 3)


def test_a_sequence_across_a_chunk_of_pairs_equals_the_chain_of_the_four_calls():
    """T = 70 frames of 24 x 32: the tracking pass crosses a 64-pair chunk and the warp a 64-frame chunk"""
    frames, _ = SM.jitter_scene(9, T=70, H=24, W=32)
    T, H, W = frames.shape
    K, D, q, md, hyps, r = 16, 8, 0.05, 3.0, 32, 5
    w = SM.weights(r)
    got = _sequence(frames, K, D, q, md, MM.SIMILARITY, hyps, 1.0, 2, w, levels=2)
    tr, vis, born, _, _ = _call(frames, K, D, q, md, levels=2)
    model, _, counts = _tracks_device(tr, vis, born, MM.SIMILARITY, hyps, 1.0, 2, 0)
    corr, mp, held = _trajectory_device(model, counts, T, w)
    out, _ = _warp_device(frames, mp)
    for g, x, name in zip(got, (out, corr, model, counts, held), NAMES):
        SM.same(g, x, name)
    assert counts[:, 2].sum() > T // 2, "most steps are fitted"
    for x, y, name in zip((corr, mp, held), SM.trajectory(model, counts, T, w), ("correction", "map", "held")):
        SM.same(x, y, f"the chain's trajectory against the model: {name}")


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing():
    import torch

    import _oflk

    L = _oflk.lib()
    INV = _oflk.OFLK_ERR_INVALID
    d = "cuda:0"
    T, H, W = 5, 8, 12
    model = torch.from_numpy(SM.noisy_models(T - 1, MM.AFFINE, 1)).to(d)
    corr = torch.full((T, 6), -7.0, device=d)
    mp = torch.full((T, 6), -7.0, dtype=torch.float64, device=d)
    held = torch.full((T - 1,), 9, dtype=torch.uint8, device=d)
    frames = torch.from_numpy(_frames(np.float32, T, H, W, 2)).to(d)
    out = torch.full((T, H, W), -7.0, device=d)
    ins = torch.full((T, H, W), 9, dtype=torch.uint8, device=d)
    good = np.ones(4, np.float64)
    a = dict(model=model.data_ptr(), T=T, w=good, radius=3, corr=corr.data_ptr(), mp=mp.data_ptr())

    def traj(**kw):
        b = dict(a, **kw)
        return L.oflk_stabilize_trajectory(b["model"], None, b["T"], _oflk._f64(b["w"]), b["radius"], b["corr"], b["mp"],
                                           held.data_ptr(), None)

    for kw in [dict(T=0), dict(radius=-1), dict(radius=65), dict(w=np.float64([1, 1, 0, 1])), dict(w=np.float64([1, np.nan, 1, 1])),
               dict(w=np.float64([1, 1, 1, np.inf])), dict(w=np.float64([-1, 1, 1, 1])), dict(model=None), dict(corr=None), dict(mp=None),
               dict(mp=a["mp"] + 4)]:
        assert traj(**kw) == INV, kw
    ident = torch.from_numpy(np.tile(SM.IDENTITY, (T, 1))).to(d)
    w_ = dict(frames=frames.data_ptr(), u8=0, F=T, H=H, W=W, mp=ident.data_ptr(), out=out.data_ptr())

    def warp(**kw):
        b = dict(w_, **kw)
        return L.oflk_warp_affine(b["frames"], b["u8"], b["F"], b["H"], b["W"], b["mp"], b["out"], ins.data_ptr(), None)

    for u8 in (0, 1):
        for kw in [dict(F=0), dict(H=1), dict(W=1), dict(frames=None), dict(mp=None), dict(out=None), dict(mp=w_["mp"] + 4)]:
            assert warp(u8=u8, **kw) == INV, (u8, kw)
    torch.cuda.synchronize()
    assert (corr == -7.0).all() and (mp == -7.0).all() and (held == 9).all() and (out == -7.0).all() and (ins == 9).all(), \
        "a refused call wrote nothing"
    assert traj() == 0 and warp() == 0
    torch.cuda.synchronize()
    want = SM.trajectory(model.cpu().numpy(), None, T, good)
    SM.same(corr.cpu().numpy(), want[0], "the accepted trajectory")
    SM.same(mp.cpu().numpy(), want[1], "the accepted trajectory: map")
    SM.same(out.cpu().numpy(), frames.cpu().numpy(), "the accepted warp under identity maps")
    assert ins.all()
    # the sequence call: the caller's arrays stay as they were
    f8, _ = SM.jitter_scene(1, T=4, H=32, W=40)
    o = np.full(f8.shape, 77, np.uint8)
    c = np.full((4, 6), -7.0, np.float32)

    def seq(T=4, K=10, model=0, radius=2, wt=good, D=2):
        return L.oflk_stabilize_sequence_u8(f8.ctypes.data, T, 32, 40, 2, 5, 3, 0.01, 0.5, 4.0, 0.05, 4.0, K, D, model, 16, 1.0, 0,
                                            _oflk._f64(wt), radius, o.ctypes.data, _oflk.ptr(c), None, None, None)

    for kw in [dict(T=1), dict(K=0), dict(model=5), dict(radius=65), dict(wt=np.float64([1, 0, 1, 1])), dict(D=0)]:
        assert seq(**kw) == INV, kw
    assert (o == 77).all() and (c == -7.0).all()
    assert seq() == 0 and (c[0] == np.float32(SM.IDENTITY)).all() and np.array_equal(o[0], f8[0])
