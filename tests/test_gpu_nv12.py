"""GPU tests of NV12 video (run on an MI355X: python -m pytest tests/test_gpu_nv12.py -m gpu -q).

The fused two-plane warps, oflk_stabilize_sequence_nv12 and an NV12 oflk_stabilizer must equal the statement
(tests/nv12_model.py) and the library's own planar results -- Y under the map, U and V under the chroma map, 128 where their
inside is 0 -- byte for byte.  No tolerance anywhere.
"""
import numpy as np
import pytest

import motion_model as MM
import nv12_model as NM
import stabilize_model as SM
from test_gpu_stabilize import _sequence
from test_gpu_tracker import _from_device
from test_stabilize_cpu import SCENE

pytestmark = pytest.mark.gpu

SITINGS = ["left", "center"]


# ---------------------------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------------------------
def _warp_device(frames, maps, siting="left", inside=True, offset=0):
    """the NV12 device warps ((F, 6) maps: affine, (F, 9): perspective).  The frames fill an allocation of exactly their size;
    out and inside start `offset` bytes past their allocations' start, are preset and have a guard behind them"""
    import torch

    import _oflk

    frames = np.ascontiguousarray(frames)
    F, R, W = frames.shape
    H = 2 * R // 3
    maps = np.ascontiguousarray(maps, np.float64)
    d = "cuda:0"
    n, px = frames.size, F * H * W
    t_in = torch.from_numpy(frames.reshape(-1)).to(d)
    t_out = torch.full((offset + n + 8,), 77, dtype=torch.uint8, device=d)
    t_ins = torch.full((offset + px + 8,), 9, dtype=torch.uint8, device=d)
    t_map = torch.from_numpy(maps).to(d)
    fn = _oflk.warp_perspective_nv12 if maps.shape[1] == 9 else _oflk.warp_affine_nv12
    fn(t_in.data_ptr(), F, H, W, t_map.data_ptr(), t_out.data_ptr() + offset, t_ins.data_ptr() + offset if inside else 0,
       NM.SITING_CODES[siting])
    torch.cuda.synchronize()
    out, ins = t_out.cpu().numpy(), t_ins.cpu().numpy()
    assert (out[:offset] == 77).all() and (out[offset + n:] == 77).all(), "nothing is written outside out"
    assert (ins[:offset] == 9).all() and (ins[offset + px:] == 9).all(), "nothing is written outside inside"
    if not inside:
        assert (ins == 9).all()
        return out[offset:offset + n].reshape(frames.shape), None
    return out[offset:offset + n].reshape(frames.shape), ins[offset:offset + px].reshape(F, H, W)


def _planar(frames, maps, siting):
    """the library's own planar u8 warps (host forms): Y under the maps, U and V under the chroma maps, 128 where their
    inside is 0; (out (F, 3H/2, W), inside (F, H, W) of the Y plane)"""
    import lucas_kanade_core as K

    warp = K.warp_perspective if np.shape(maps)[1] == 9 else K.warp_affine
    y, uv = NM.planes(frames)
    oy, ins = warp(np.ascontiguousarray(y), maps, return_inside=True)
    mc = NM.chroma_maps(maps, siting)
    ch = []
    for c in range(2):
        o, i = warp(np.ascontiguousarray(uv[..., c]), mc, return_inside=True)
        ch.append(np.where(i, o, np.uint8(128)).astype(np.uint8))
    return NM.from_planes(oy, np.stack(ch, -1)), ins.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the warp
# ---------------------------------------------------------------------------------------------------------------------
# (4, 4) the smallest, chroma 2 x 2; (6, 10) neither plane vectorised, chroma rows no multiple of 4; (10, 12) luma vectorised,
# chroma not; (8, 16) both; (6, 516) chroma width 258 crosses a block's 256 columns, luma crosses two; (10, 520) the same,
# vectorised, three luma row groups and two chroma
SHAPES = [(4, 4), (6, 10), (10, 12), (8, 16), (6, 516), (10, 520)]


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_the_nv12_warp_equals_the_model_and_the_planar_warps(kind, shape, siting):
    H, W = shape
    named = NM.affine_maps(H, W) if kind == "affine" else NM.perspective_maps(H, W)
    model = NM.warp_affine if kind == "affine" else NM.warp_perspective
    frames = NM.random_frames(2, H, W, 100 * H + W)
    for name, maps in named.items():
        want, want_in = model(frames, maps, siting)
        what = f"{kind} {H}x{W} {siting} {name}"
        got, got_in = _warp_device(frames, maps, siting)
        SM.same(got, want, what)
        SM.same(got_in, want_in, what + ": inside")
        SM.same(_warp_device(frames, maps, siting, inside=False)[0], want, what + ", inside NULL")
        off, off_in = _warp_device(frames, maps, siting, offset=1)
        SM.same(off, want, what + ", bases offset by one byte")
        SM.same(off_in, want_in, what + ", bases offset by one byte: inside")
        lib, lib_in = _planar(frames, maps, siting)
        SM.same(got, lib, what + ": the library's planar warps of the three planes")
        SM.same(got_in, lib_in, what + ": the planar warp's inside")
        if name == "mostly outside":
            assert 0 < want_in.mean() < 0.5 and (NM.planes(want)[1] == 128).any(), what
        else:
            assert want_in.any(), what


@pytest.mark.parametrize("siting", SITINGS)
def test_the_identity_returns_the_frames_and_a_third_row_0_0_1_the_affine_bytes(siting):
    for H, W in ((4, 4), (6, 10), (8, 16)):
        frames = NM.random_frames(3, H, W, H + W)
        ident = np.tile(SM.IDENTITY, (3, 1))
        for maps in (ident, NM.as_homography(ident)):
            out, ins = _warp_device(frames, maps, siting)
            SM.same(out, frames, f"identity, {H}x{W}")   # the last luma pixel and the last chroma pair of the last frame included
            assert (ins == 1).all()
        for name, m in NM.affine_maps(H, W).items():
            maps = np.concatenate([m, m[:1]])
            a, a_in = _warp_device(frames, maps, siting)
            p, p_in = _warp_device(frames, NM.as_homography(maps), siting)
            SM.same(p, a, f"{name}: third row (0, 0, 1) against the affine call")
            SM.same(p_in, a_in, f"{name}: third row (0, 0, 1) against the affine call: inside")


@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_the_frame_loop_above_the_grid_limit(kind):
    """F = 65 537 frames of 4 x 4 (1.5 MB) under maps that differ from frame to frame; a few frames at both ends and around
    65 535 against the model"""
    F, H, W = 65537, 4, 4
    frames = NM.random_frames(F, H, W, 1)
    f = np.arange(F)
    maps = np.zeros((F, 6))
    maps[:, 0] = maps[:, 4] = 1.0
    maps[:, 2], maps[:, 5] = (f % 5 - 2) * 0.5, ((f // 5) % 3 - 1) * 0.75
    if kind == "perspective":
        maps = NM.as_homography(maps)
    model = NM.warp_affine if kind == "affine" else NM.warp_perspective
    got, got_in = _warp_device(frames, maps, "center")
    for sl in (slice(0, 4), slice(65533, 65537)):
        want, want_in = model(frames[sl], maps[sl], "center")
        SM.same(got[sl], want, f"frames {sl}")
        SM.same(got_in[sl], want_in, f"frames {sl}: inside")
    assert (got != 77).any(axis=(1, 2)).all() and (got_in != 9).all(), "every frame is written"


def test_the_host_forms_across_a_chunk_equal_the_device_form():
    import lucas_kanade_pyramidal as P

    F, H, W = 70, 8, 12   # two chunks: a chunk holds at most 64 frames
    frames = NM.random_frames(F, H, W, 4)
    maps = np.stack([NM.rotation(H, W, 0.5 * f, 1.0 + 0.002 * f) for f in range(F)])
    dev, dev_in = _warp_device(frames, maps, "left")
    out, ins = P.warp_affine_nv12(frames, maps, return_inside=True)
    SM.same(out, dev, "affine host form")
    assert ins.dtype == bool and np.array_equal(ins, dev_in.astype(bool))
    SM.same(out[60:], NM.warp_affine(frames[60:], maps[60:])[0], "across the chunk boundary against the model")
    maps9 = NM.as_homography(maps)
    maps9[:, 6] = 1e-3 / W
    dev9, dev9_in = _warp_device(frames, maps9, "center")
    out9, ins9 = P.warp_perspective_nv12(frames, maps9, "center", return_inside=True)
    SM.same(out9, dev9, "perspective host form")
    assert np.array_equal(ins9, dev9_in.astype(bool))
    SM.same(P.warp_affine_nv12(frames[3], maps[3]), dev[3], "one frame")


# ---------------------------------------------------------------------------------------------------------------------
# the offline stabiliser
# ---------------------------------------------------------------------------------------------------------------------
def _scene_args():
    s = SCENE
    return (s["K"], s["D"], s["q"], s["md"], s["family"], s["hyps"], s["thr"], s["seed"], SM.weights(s["r"], s["sigma"]))


def _sequence_nv12(frames, siting, K, D, q, md, family, hyps, thr, seed, w, levels=3, win=5, iters=3):
    """the C entry point, every output preset with bytes that it must overwrite"""
    import _oflk

    frames = np.ascontiguousarray(frames)
    T, R, W = frames.shape
    H = 2 * R // 3
    out = np.full(frames.shape, 77, np.uint8)
    corr, model = np.full((T, 6), -7.0, np.float32), np.full((T - 1, 6), -7.0, np.float32)
    counts, held = np.full((T - 1, 3), -3, np.int32), np.full(T - 1, 9, np.uint8)
    w = np.ascontiguousarray(w, np.float64)
    _oflk.check(_oflk.lib().oflk_stabilize_sequence_nv12(
        frames.ctypes.data, T, H, W, NM.SITING_CODES[siting], levels, win, iters, 0.01, 0.5, 4.0, q, md, K, D, family, hyps, thr, seed,
        _oflk._f64(w), len(w) - 1, out.ctypes.data, _oflk.ptr(corr), _oflk.ptr(model), counts.ctypes.data_as(_oflk._i32p),
        held.ctypes.data))
    return out, corr, model, counts, held


def _check_sequence(frames, siting, args, what, **kw):
    """the NV12 call against the grey call on the Y planes and the NV12 warp under the trajectory's maps"""
    import _oflk
    import lucas_kanade_pyramidal as P

    got = _sequence_nv12(frames, siting, *args, **kw)
    grey = np.ascontiguousarray(NM.planes(frames)[0])
    want = _sequence(grey, *args, **kw)
    for g, x, name in zip(got[1:], want[1:], ("correction", "model", "counts", "held")):
        SM.same(g, x, f"{what}: {name}")
    _, mp, _ = _oflk.stabilize_trajectory_host(want[2], want[3], len(frames), np.ascontiguousarray(args[-1], np.float64))
    SM.same(got[0], P.warp_affine_nv12(frames, mp, siting), f"{what}: out against the NV12 warp under the trajectory's maps")
    SM.same(NM.planes(got[0])[0], want[0], f"{what}: the Y planes against the grey call's frames")
    return got, want, mp


@pytest.mark.parametrize("siting", SITINGS)
def test_the_nv12_sequence_call_is_the_grey_call_on_the_y_planes_and_the_nv12_warp(siting):
    grey, _ = SM.jitter_scene(0)
    frames = NM.from_grey(grey)
    assert frames.shape == (14, 96, 80)
    got, want, mp = _check_sequence(frames, siting, _scene_args(), siting)
    assert (got[0] != frames).any() and want[3][:, 2].sum() >= 10, "the frames are moved, most steps are fitted"
    SM.same(got[0], NM.warp_affine(frames, mp, siting)[0], "out against the model's warp")


def test_an_nv12_sequence_across_the_chunks():
    """T = 70 frames of 24 x 32: the warp crosses a 64-frame chunk, the tracking pass a 64-pair chunk"""
    grey, _ = SM.jitter_scene(9, T=70, H=24, W=32)
    frames = NM.from_grey(grey)
    _, want, _ = _check_sequence(frames, "left", (16, 8, 0.05, 3.0, MM.SIMILARITY, 32, 1.0, 2, SM.weights(5)), "70 frames", levels=2)
    assert want[3][:, 2].sum() > 35, "most steps are fitted"


def test_the_python_sequence_call_takes_nv12_and_keeps_refining():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    grey, _ = SM.jitter_scene(0)
    frames = NM.from_grey(grey)
    s = SCENE
    kw = dict(model="translation", radius=s["r"], sigma=s["sigma"], hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"],
              quality_level=s["q"], min_distance=s["md"])
    got = P.lucas_kanade_pyramidal_sequence_stabilize_nv12(frames, s["K"], s["D"], siting="center", **kw)
    raw = _sequence_nv12(frames, "center", *_scene_args())
    assert got.frames.shape == frames.shape and got.frames.dtype == np.uint8
    SM.same(got.frames, raw[0], "frames")
    SM.same(got.correction, raw[1].reshape(-1, 2, 3), "correction")
    for it in (0, 2):
        c = P.lucas_kanade_pyramidal_sequence_stabilize_nv12(frames, s["K"], s["D"], refine_iterations=it, **kw)
        g = P.lucas_kanade_pyramidal_sequence_stabilize(grey, s["K"], s["D"], refine_iterations=it, **kw)
        SM.same(c.correction, g.correction, f"refine_iterations={it}: correction")
        SM.same(c.model, g.model, f"refine_iterations={it}: model")
        assert np.array_equal(c.status, g.status) and np.array_equal(c.held, g.held)
        mp = K.stabilize_trajectory(g.model, g.status, s["r"], s["sigma"]).map
        SM.same(c.frames, P.warp_affine_nv12(frames, mp), f"refine_iterations={it}: frames")


# ---------------------------------------------------------------------------------------------------------------------
# the online stabiliser
# ---------------------------------------------------------------------------------------------------------------------
def _stabilizer(shape, K, D, q, md, family, hyps, thr, seed, w, nv12=False, siting="left", channels=0):
    import _oflk

    return _oflk.Stabilizer(0, shape[0], shape[1], True, K, D, family, w, hyps, thr, seed, 3, 5, 3, quality_level=q, min_distance=md,
                            channels=channels, nv12=nv12, siting=NM.SITING_CODES[siting])


def _stream_host(st, frames):
    """push every frame and flush: (out, correction (T, 6), inside), in frame order"""
    out, corr, ins = [], [], []
    for t, f in enumerate(frames):
        e, o, c, i = st.push(np.ascontiguousarray(f), True)
        assert e == (t - st.radius if t >= st.radius else -1) and st.frame_index == t
        if e >= 0:
            out.append(o), corr.append(c), ins.append(i)
    first, o, c, i = st.flush(True)
    assert len(o) == min(st.radius, len(frames)) and first == len(frames) - len(o)
    return np.stack(out + list(o)), np.stack(corr + list(c)), np.stack(ins + list(i))


def _stream_device(st, frames, H):
    """the same through push_device / flush_device on a side stream; d_out and d_inside keep their preset until an emission"""
    import torch

    T, r = len(frames), st.radius
    side = torch.cuda.Stream()
    s = side.cuda_stream
    d_frames = torch.from_numpy(frames).to("cuda:0")
    d_out = torch.full((r,) + frames.shape[1:], 77, dtype=torch.uint8, device="cuda:0")
    d_ins = torch.full((r, H, frames.shape[2]), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out, corr, ins = [], [], []
    grown = None
    for t in range(T):
        e = st.push_device(d_frames[t].data_ptr(), d_out.data_ptr(), d_ins.data_ptr(), s)
        side.synchronize()
        assert e == (t - r if t >= r else -1)
        grown = st.workspace_bytes if grown is None else grown
        assert st.workspace_bytes == grown > 0, "no push after the first allocates"
        if e < 0:
            assert (d_out == 77).all() and (d_ins == 9).all(), f"frame {t}: nothing is emitted, nothing is written"
            continue
        assert (d_out[1:] == 77).all() and (d_ins[1:] == 9).all()
        out.append(d_out[0].cpu().numpy()), ins.append(d_ins[0].cpu().numpy())
        corr.append(_from_device(st.correction_device()[0], (6,), "<f4"))
    first, count = st.flush_device(d_out.data_ptr(), d_ins.data_ptr(), s)
    side.synchronize()
    assert (first, count) == (T - r, r)
    corr += list(_from_device(st.correction_device()[0], (r, 6), "<f4"))
    return np.stack(out + list(d_out.cpu().numpy())), np.stack(corr), np.stack(ins + list(d_ins.cpu().numpy())), grown


@pytest.mark.parametrize("siting", SITINGS)
def test_nv12_pushes_and_a_flush_equal_the_nv12_sequence_call(siting):
    import _oflk

    grey, _ = SM.jitter_scene(0)
    frames = NM.from_grey(grey)
    T, H, W = grey.shape
    args = _scene_args()
    r = SCENE["r"]
    assert r == 3
    want = _sequence_nv12(frames, siting, *args)
    _, mp, _ = _oflk.stabilize_trajectory_host(want[2], want[3], T, args[-1])
    want_in = NM.warp_affine(frames, mp, siting)[1]
    host, dev = _stabilizer((H, W), *args, nv12=True, siting=siting), _stabilizer((H, W), *args, nv12=True, siting=siting)
    packed = _stabilizer((H, W), *args, channels=3)
    try:
        assert host.workspace_bytes == 0
        out, corr, ins = _stream_host(host, frames)
        SM.same(out, want[0], "push: frames")
        SM.same(corr, want[1], "push: correction")
        SM.same(ins, want_in, "push: inside")
        assert ins.any() and not ins.all(), "the border is marked"
        d_out, d_corr, d_ins, grown = _stream_device(dev, frames, H)
        SM.same(d_out, want[0], "push_device: frames")
        SM.same(d_corr, want[1], "push_device: correction")
        SM.same(d_ins, want_in, "push_device: inside")
        fb = H * W * 3 // 2
        assert host.workspace_bytes == grown + fb + H * W, "the host forms add one staged frame and one mask"
        assert grown >= (r + 1) * fb, "the delay line holds NV12 frames"
        # a packed 3-channel stabiliser of the same shape: its delay line is twice as large, and it keeps a luma plane
        rgb = np.ascontiguousarray(np.stack([grey[0]] * 3, -1))
        d_rgb = _to_device(rgb)
        d_o = _to_device(np.zeros_like(rgb))
        assert packed.push_device(d_rgb.data_ptr(), d_o.data_ptr()) == -1
        _sync()
        assert grown <= packed.workspace_bytes - H * W, "smaller than the packed stabiliser's by at least the luma plane"
        nbytes = host.workspace_bytes
        host.reset()
        assert host.frame_index == -1
        again = _stream_host(host, frames)
        SM.same(again[0], out, "after a reset: frames")
        SM.same(again[1], corr, "after a reset: correction")
        assert host.workspace_bytes == nbytes, "a reset keeps the state"
    finally:
        host.close()
        dev.close()
        packed.close()


def _to_device(a):
    import torch

    return torch.from_numpy(a).to("cuda:0")


def _sync():
    import torch

    torch.cuda.synchronize()


def test_a_grey_stabiliser_before_and_after_an_nv12_one_is_what_it_was():
    grey, _ = SM.jitter_scene(0)
    frames = NM.from_grey(grey)
    args = _scene_args()
    want = _sequence(grey, *args)
    before, nv12, after = _stabilizer(grey.shape[1:], *args), _stabilizer(grey.shape[1:], *args, nv12=True), None
    try:
        got = [before.push(np.ascontiguousarray(f)) for f in grey[:7]]
        _stream_host(nv12, frames)
        got += [before.push(np.ascontiguousarray(f)) for f in grey[7:]]
        rest = before.flush()
        out = np.stack([g[1] for g in got if g[0] >= 0] + list(rest[1]))
        corr = np.stack([g[2] for g in got if g[0] >= 0] + list(rest[2]))
        SM.same(out, want[0], "a grey stabiliser around an NV12 one: out")
        SM.same(corr, want[1], "a grey stabiliser around an NV12 one: correction")
        after = _stabilizer(grey.shape[1:], *args)
        o, c, _ = _stream_host(after, grey)
        SM.same(o, want[0], "a grey stabiliser made after an NV12 one: out")
        SM.same(c, want[1], "a grey stabiliser made after an NV12 one: correction")
    finally:
        for x in (before, nv12, after):
            if x is not None:
                x.close()


def test_the_python_class_takes_nv12_frames():
    import lucas_kanade_pyramidal as P

    grey, _ = SM.jitter_scene(0)
    frames = NM.from_grey(grey)
    H, W = grey.shape[1:]
    s = SCENE
    kw = dict(model="translation", radius=s["r"], sigma=s["sigma"], hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"],
              quality_level=s["q"], min_distance=s["md"])
    want = P.lucas_kanade_pyramidal_sequence_stabilize_nv12(frames, s["K"], s["D"], siting="center", **kw)
    raw = _sequence_nv12(frames, "center", *_scene_args())
    SM.same(want.frames, raw[0], "the sequence function against the C call: frames")
    SM.same(want.correction, raw[1].reshape(-1, 2, 3), "the sequence function against the C call: correction")
    with P.OnlineStabilizer((H, W), s["K"], s["D"], inside=True, layout="nv12", siting="center", **kw) as st:
        got = [e for e in (st.push(f) for f in frames) if e is not None] + st.flush()
    assert [g.index for g in got] == list(range(len(frames)))
    assert got[0].frame.shape == (3 * H // 2, W) and got[0].inside.shape == (H, W) and got[0].inside.dtype == bool
    SM.same(np.stack([g.frame for g in got]), want.frames, "frames")
    SM.same(np.stack([g.correction for g in got]), want.correction, "correction")
