"""GPU tests of colour video (run on an MI355X: python -m pytest tests/test_gpu_colour.py -m gpu -q).

oflk_luma_u8, the packed warps, oflk_stabilize_sequence_packed, a packed oflk_stabilizer and the colour mosaic must equal the
statement (tests/colour_model.py) and the library's own planar results per channel, byte for byte.  No tolerance anywhere.
"""
import numpy as np
import pytest

import colour_model as CM
import motion_model as MM
import stabilize_model as SM
from test_gpu_stabilize import _sequence
from test_gpu_tracker import _from_device
from test_stabilize_cpu import SCENE

pytestmark = pytest.mark.gpu

ORDERS = ["rgb", "bgr"]


# ---------------------------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------------------------
def _luma_device(frames, order, offset=0):
    """oflk_luma_u8 on buffers whose bases are `offset` bytes past an allocation's start; the output preset, a guard behind it"""
    import torch

    import _oflk

    F, H, W, C = frames.shape
    n = F * H * W
    d = "cuda:0"
    t_in = torch.empty(n * C + offset, dtype=torch.uint8, device=d)
    t_in[offset:].copy_(torch.from_numpy(frames.reshape(-1)))
    t_out = torch.full((offset + n + 8,), 77, dtype=torch.uint8, device=d)
    _oflk.luma(t_in.data_ptr() + offset, F, H, W, C, t_out.data_ptr() + offset, CM.ORDERS[order])
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()
    assert (out[:offset] == 77).all() and (out[offset + n:] == 77).all(), "nothing is written outside the luma"
    return out[offset:offset + n].reshape(F, H, W)


def _warp_device(frames, maps, inside=True, offset=0):
    """the packed device warps ((F, 6) maps: affine, (F, 9): perspective).  The frames fill an allocation of exactly their
    size; out and inside start `offset` bytes past their allocations' start, are preset and have a guard behind them"""
    import torch

    import _oflk

    frames = np.ascontiguousarray(frames)
    F, H, W, C = frames.shape
    maps = np.ascontiguousarray(maps, np.float64)
    d = "cuda:0"
    n = frames.size
    t_in = torch.from_numpy(frames.reshape(-1)).to(d)
    t_out = torch.full((offset + n + 8,), 77, dtype=torch.uint8, device=d)
    t_ins = torch.full((offset + n // C + 8,), 9, dtype=torch.uint8, device=d)
    t_map = torch.from_numpy(maps).to(d)
    fn = _oflk.warp_perspective_packed if maps.shape[1] == 9 else _oflk.warp_affine_packed
    fn(t_in.data_ptr(), F, H, W, C, t_map.data_ptr(), t_out.data_ptr() + offset, t_ins.data_ptr() + offset if inside else 0)
    torch.cuda.synchronize()
    out, ins = t_out.cpu().numpy(), t_ins.cpu().numpy()
    assert (out[:offset] == 77).all() and (out[offset + n:] == 77).all(), "nothing is written outside out"
    assert (ins[:offset] == 9).all() and (ins[offset + n // C:] == 9).all(), "nothing is written outside inside"
    if not inside:
        assert (ins == 9).all()
        return out[offset:offset + n].reshape(frames.shape), None
    return out[offset:offset + n].reshape(frames.shape), ins[offset:offset + n // C].reshape(F, H, W)


def _planar(frames, maps):
    """the library's own planar warp (host form) of every plane: (out (F, H, W, C), inside (F, H, W) of plane 0)"""
    import lucas_kanade_core as K

    warp = K.warp_perspective if np.shape(maps)[1] == 9 else K.warp_affine
    planes = [warp(np.ascontiguousarray(frames[..., c]), maps, return_inside=True) for c in range(frames.shape[-1])]
    for p in planes[1:]:
        assert np.array_equal(p[1], planes[0][1])
    return np.stack([p[0] for p in planes], -1), planes[0][1].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# luma
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(1, 2, 2, 3), (3, 5, 7, 3), (2, 9, 257, 4), (1, 4, 1024, 3), (2, 6, 8, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_the_luma_equals_the_model(shape, order):
    import lucas_kanade_core as K

    frames = CM.random_frames(*shape, seed=sum(shape))
    want = CM.luma(frames, order)
    SM.same(_luma_device(frames, order), want, "device form")
    SM.same(_luma_device(frames, order, offset=1), want, "bases offset by one byte: the element-wise form")
    SM.same(K.rgb_to_luma(frames, order), want, "rgb_to_luma")
    SM.same(K.rgb_to_luma(frames[0], order), want[0], "rgb_to_luma of one frame")


@pytest.mark.parametrize("order", ORDERS)
def test_the_luma_of_every_rgb_triple(order):
    """one 4096 x 4096 x 3 frame that holds every (R, G, B) exactly once: exhaustive"""
    i = np.arange(1 << 24, dtype=np.uint32)
    frame = np.stack([(i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i >> 16).astype(np.uint8)], -1)
    frame = frame.reshape(1, 4096, 4096, 3)
    got = _luma_device(frame, order)
    SM.same(got, CM.luma(frame, order), "every triple")
    grey = (i & 255) == ((i >> 8) & 255)
    grey &= (i & 255) == (i >> 16)
    assert np.array_equal(got.reshape(-1)[grey], np.arange(256, dtype=np.uint8)), "grey returns itself"


def test_the_host_luma_in_chunks_equals_the_device_form():
    import _oflk

    frames = CM.random_frames(70, 6, 10, 3, 5)   # two chunks: a chunk holds at most 64 frames
    SM.same(_oflk.luma_host(frames, 1), CM.luma(frames, "bgr"), "70 frames")


# ---------------------------------------------------------------------------------------------------------------------
# the packed warps
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (3, 5), (7, 13), (8, 16), (5, 260), (6, 1028)]


def _groups(named):
    """the maps three at a time (F = 3, three different maps), the last group filled up from the front"""
    keys = list(named)
    keys += keys[:(-len(keys)) % 3]
    return [keys[i:i + 3] for i in range(0, len(keys), 3)]


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_the_packed_warp_equals_the_model_and_the_planar_warp(kind, shape, channels):
    H, W = shape
    named = CM.affine_maps(H, W) if kind == "affine" else CM.perspective_maps(H, W)
    model = CM.warp_affine if kind == "affine" else CM.warp_perspective
    frames = CM.random_frames(3, H, W, channels, 100 * H + W + channels)
    seen = {}
    for keys in _groups(named):
        maps = np.stack([named[k] for k in keys])
        want, want_in = model(frames, maps)
        what = f"{kind} {H}x{W}x{channels} {keys}"
        got, got_in = _warp_device(frames, maps)
        SM.same(got, want, what)
        SM.same(got_in, want_in, what + ": inside")
        SM.same(_warp_device(frames, maps, inside=False)[0], want, what + ", inside NULL")
        off, off_in = _warp_device(frames, maps, offset=1)
        SM.same(off, want, what + ", bases offset by one byte")
        SM.same(off_in, want_in, what + ", bases offset by one byte: inside")
        lib, lib_in = _planar(frames, maps)
        SM.same(got, lib, what + ": the library's planar warp of every plane")
        SM.same(got_in, lib_in, what + ": the planar warp's inside")
        for f, k in enumerate(keys):
            seen[k] = (got[f], got_in[f], frames[f])
    tag = "affine: " if kind == "perspective" else ""
    out, ins, src = seen[tag + "identity"]
    assert np.array_equal(out, src) and (ins == 1).all(), "the identity returns the frames' bytes"
    out, ins, src = seen[tag + "integer shift"]
    assert np.array_equal(out[1:, :W - 1], src[:H - 1, 1:]) and not out[0].any() and not out[:, W - 1].any()
    for k in ("all outside", "NaN coefficient"):
        out, ins, _ = seen[tag + k]
        assert not out.any() and not ins.any(), k
    if kind == "perspective":
        ins = seen["w changes sign"][1]
        assert ins[:, 0].all() and not ins[:, W - 1].any()
        # third row (0, 0, 1): the packed affine warp's bytes
        keys = [k for k in named if k.startswith("affine: ")][:3]
        maps9 = np.stack([named[k] for k in keys])
        a, a_in = _warp_device(frames, np.ascontiguousarray(maps9[:, :6]))
        p, p_in = _warp_device(frames, maps9)
        SM.same(p, a, "third row (0, 0, 1) against the packed affine warp")
        SM.same(p_in, a_in, "third row (0, 0, 1) against the packed affine warp: inside")


@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_the_frame_loop_above_the_grid_limit(kind):
    """F = 65 537 frames of 2 x 2 x 3 under integer shifts that differ from frame to frame"""
    F = 65537
    frames = CM.random_frames(F, 2, 2, 3, 1)
    f = np.arange(F)
    dx, dy = f % 3 - 1, (f // 3) % 3 - 1
    maps = np.zeros((F, 6))
    maps[:, 0] = maps[:, 4] = 1.0
    maps[:, 2], maps[:, 5] = dx, dy
    # an integer shift copies pixel (y + dy, x + dx) where it exists and writes 0 elsewhere
    want, want_in = np.zeros_like(frames), np.zeros((F, 2, 2), np.uint8)
    for y in range(2):
        for x in range(2):
            ok = (y + dy >= 0) & (y + dy <= 1) & (x + dx >= 0) & (x + dx <= 1)
            want[ok, y, x] = frames[f[ok], (y + dy)[ok], (x + dx)[ok]]
            want_in[ok, y, x] = 1
    head = CM.warp_affine(frames[:18], maps[:18])
    SM.same(want[:18], head[0], "the shortcut against the model")
    SM.same(want_in[:18], head[1], "the shortcut against the model: inside")
    if kind == "perspective":
        maps = np.concatenate([maps, np.tile([0.0, 0.0, 1.0], (F, 1))], 1)
    got, got_in = _warp_device(frames, maps)
    SM.same(got, want, "65 537 frames")
    SM.same(got_in, want_in, "65 537 frames: inside")


@pytest.mark.parametrize("channels", [3, 4])
def test_the_last_pixel_of_the_last_frame(channels):
    """random frames in an allocation of exactly F H W C bytes, under maps whose taps include the last pixel of every frame.
    (That no load leaves the frames is shown by the tap loads themselves, DESIGN.md section 4, not by this test.)"""
    import lucas_kanade_core as K

    H, W = 5, 7
    frames = CM.random_frames(2, H, W, channels, 9)
    for m in (CM.affine_maps(H, W)["identity"], np.array([1.0, 0, 0.5, 0, 1, 0.5]), np.array([1.0, 0, 0.5, 0, 1, 0.0])):
        maps = np.tile(m, (2, 1))
        want, want_in = CM.warp_affine(frames, maps)
        assert want_in.any()
        got, got_in = _warp_device(frames, maps)
        SM.same(got, want, f"map {m.tolist()}")
        SM.same(got_in, want_in, f"map {m.tolist()}: inside")
        maps9 = np.stack([CM.as_homography(m)] * 2)
        SM.same(_warp_device(frames, maps9)[0], want, f"map {m.tolist()}, perspective")
        out, ins = K.warp_affine(frames, maps, return_inside=True)
        SM.same(out, want, "the Python wrapper")
        assert ins.dtype == bool and np.array_equal(ins, want_in.astype(bool))


def test_the_host_warp_in_chunks_equals_the_model():
    import lucas_kanade_core as K

    F, H, W = 70, 6, 12   # two chunks
    frames = CM.random_frames(F, H, W, 3, 4)
    maps = np.stack([CM.rotation(H, W, 0.5 * f, 1.0 + 0.002 * f) for f in range(F)])
    want, want_in = CM.warp_affine(frames[60:], maps[60:])
    out, ins = K.warp_affine(frames, maps, return_inside=True)
    SM.same(out[60:], want, "across the chunk boundary")
    assert np.array_equal(ins[60:], want_in.astype(bool))
    maps9 = np.stack([CM.as_homography(m) for m in maps])
    SM.same(K.warp_perspective(frames, maps9), out, "the perspective host form under third rows (0, 0, 1)")


# ---------------------------------------------------------------------------------------------------------------------
# the offline stabiliser
# ---------------------------------------------------------------------------------------------------------------------
def _scene_args(r=None):
    s = SCENE
    w = SM.weights(s["r"], s["sigma"]) if r is None else SM.weights(r)
    return (s["K"], s["D"], s["q"], s["md"], s["family"], s["hyps"], s["thr"], s["seed"], w)


def _sequence_packed(frames, order, K, D, q, md, family, hyps, thr, seed, w, levels=3, win=5, iters=3):
    """the C entry point, every output preset with bytes that it must overwrite"""
    import _oflk

    frames = np.ascontiguousarray(frames)
    T, H, W, C = frames.shape
    out = np.full(frames.shape, 77, np.uint8)
    corr, model = np.full((T, 6), -7.0, np.float32), np.full((T - 1, 6), -7.0, np.float32)
    counts, held = np.full((T - 1, 3), -3, np.int32), np.full(T - 1, 9, np.uint8)
    w = np.ascontiguousarray(w, np.float64)
    _oflk.check(_oflk.lib().oflk_stabilize_sequence_packed(
        frames.ctypes.data, T, H, W, C, CM.ORDERS[order], levels, win, iters, 0.01, 0.5, 4.0, q, md, K, D, family, hyps, thr, seed,
        _oflk._f64(w), len(w) - 1, out.ctypes.data, _oflk.ptr(corr), _oflk.ptr(model), counts.ctypes.data_as(_oflk._i32p),
        held.ctypes.data))
    return out, corr, model, counts, held


def _check_sequence(frames, order, args, what, **kw):
    """the packed call against the grey call on the library's luma and the packed warp under the trajectory's maps"""
    import _oflk
    import lucas_kanade_core as K

    got = _sequence_packed(frames, order, *args, **kw)
    grey = K.rgb_to_luma(frames, order)
    SM.same(grey, CM.luma(frames, order), f"{what}: the library's luma")
    want = _sequence(grey, *args, **kw)
    for g, x, name in zip(got[1:], want[1:], ("correction", "model", "counts", "held")):
        SM.same(g, x, f"{what}: {name}")
    w = args[-1]
    _, mp, _ = _oflk.stabilize_trajectory_host(want[2], want[3], len(frames), np.ascontiguousarray(w, np.float64))
    SM.same(got[0], K.warp_affine(frames, mp), f"{what}: out against the packed warp under the trajectory's maps")
    SM.same(got[0][..., 0], K.warp_affine(np.ascontiguousarray(frames[..., 0]), mp), f"{what}: plane 0 against the planar warp")
    return got, want, mp


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("channels", [3, 4])
def test_the_colour_sequence_call_is_the_grey_call_on_the_luma_and_the_packed_warp(channels, order):
    grey, _ = SM.jitter_scene(0)
    frames = CM.coloured(grey, channels)
    got, want, mp = _check_sequence(frames, order, _scene_args(), f"{channels} channels, {order}")
    assert (got[0] != frames).any() and want[3][:, 2].sum() >= 10, "the frames are moved, most steps are fitted"
    SM.same(got[0], CM.warp_affine(frames, mp)[0], "out against the model's warp")
    lum = CM.luma(frames, order)
    assert all((lum != frames[..., c]).any() for c in range(channels)), "the luma is none of the planes"


def test_a_colour_sequence_across_the_chunks():
    """T = 70 frames of 24 x 32: the luma pass and the warp cross a 64-frame chunk, the tracking pass a 64-pair chunk"""
    grey, _ = SM.jitter_scene(9, T=70, H=24, W=32)
    frames = CM.coloured(grey, 3)
    _, want, _ = _check_sequence(frames, "bgr", (16, 8, 0.05, 3.0, MM.SIMILARITY, 32, 1.0, 2, SM.weights(5)), "70 frames", levels=2)
    assert want[3][:, 2].sum() > 35, "most steps are fitted"


def test_the_python_sequence_call_takes_colour_and_keeps_refining():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    grey, _ = SM.jitter_scene(0)
    frames = CM.coloured(grey, 3)
    s = SCENE
    kw = dict(model="translation", radius=s["r"], sigma=s["sigma"], hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"],
              quality_level=s["q"], min_distance=s["md"])
    got = P.lucas_kanade_pyramidal_sequence_stabilize(frames, s["K"], s["D"], order="bgr", **kw)
    raw = _sequence_packed(frames, "bgr", *_scene_args())
    assert got.frames.shape == frames.shape and got.frames.dtype == np.uint8
    SM.same(got.frames, raw[0], "frames")
    SM.same(got.correction, raw[1].reshape(-1, 2, 3), "correction")
    lum = K.rgb_to_luma(frames, "bgr")
    for it in (0, 2):
        c = P.lucas_kanade_pyramidal_sequence_stabilize(frames, s["K"], s["D"], order="bgr", refine_iterations=it, **kw)
        g = P.lucas_kanade_pyramidal_sequence_stabilize(lum, s["K"], s["D"], refine_iterations=it, **kw)
        SM.same(c.correction, g.correction, f"refine_iterations={it}: correction")
        SM.same(c.model, g.model, f"refine_iterations={it}: model")
        assert np.array_equal(c.status, g.status) and np.array_equal(c.held, g.held)
        mp = K.stabilize_trajectory(g.model, g.status, s["r"], s["sigma"]).map
        SM.same(c.frames, K.warp_affine(frames, mp), f"refine_iterations={it}: frames")


# ---------------------------------------------------------------------------------------------------------------------
# the online stabiliser
# ---------------------------------------------------------------------------------------------------------------------
def _stabilizer(shape, K, D, q, md, family, hyps, thr, seed, w, order="rgb"):
    import _oflk

    channels = shape[2] if len(shape) == 3 else 0
    return _oflk.Stabilizer(0, shape[0], shape[1], True, K, D, family, w, hyps, thr, seed, 3, 5, 3, quality_level=q, min_distance=md,
                            channels=channels, order=CM.ORDERS[order])


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


def _stream_device(st, frames):
    """the same through push_device / flush_device on a side stream; d_out and d_inside keep their preset until an emission"""
    import torch

    T, r = len(frames), st.radius
    side = torch.cuda.Stream()
    s = side.cuda_stream
    d_frames = torch.from_numpy(frames).to("cuda:0")
    d_out = torch.full((r,) + frames.shape[1:], 77, dtype=torch.uint8, device="cuda:0")
    d_ins = torch.full((r,) + frames.shape[1:3], 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out, corr, ins = [], [], []
    grown = None
    for t in range(T):
        e = st.push_device(d_frames[t].data_ptr(), d_out.data_ptr(), d_ins.data_ptr(), s)
        side.synchronize()
        assert e == (t - r if t >= r else -1)
        grown = st.workspace_bytes if grown is None else grown
        assert st.workspace_bytes == grown > 0, "no later push allocates"
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


@pytest.mark.parametrize("channels,order", [(3, "rgb"), (4, "bgr")])
def test_colour_pushes_and_a_flush_equal_the_colour_sequence_call(channels, order):
    import _oflk

    grey, _ = SM.jitter_scene(0)
    frames = CM.coloured(grey, channels)
    T, H, W, C = frames.shape
    args = _scene_args()
    assert SCENE["r"] == 3
    want = _sequence_packed(frames, order, *args)
    _, mp, _ = _oflk.stabilize_trajectory_host(want[2], want[3], T, args[-1])
    want_in = CM.warp_affine(frames, mp)[1]
    host, dev = _stabilizer(frames.shape[1:], *args, order=order), _stabilizer(frames.shape[1:], *args, order=order)
    try:
        assert host.workspace_bytes == 0
        out, corr, ins = _stream_host(host, frames)
        SM.same(out, want[0], "push: frames")
        SM.same(corr, want[1], "push: correction")
        SM.same(ins, want_in, "push: inside")
        assert ins.any() and not ins.all(), "the border is marked"
        d_out, d_corr, d_ins, grown = _stream_device(dev, frames)
        SM.same(d_out, want[0], "push_device: frames")
        SM.same(d_corr, want[1], "push_device: correction")
        SM.same(d_ins, want_in, "push_device: inside")
        assert host.workspace_bytes == grown + (1 + C) * H * W, "the host forms add one staged frame and one mask"
        assert grown >= (SCENE["r"] + 1) * H * W * C + H * W, "the delay line holds packed frames, and there is a luma plane"
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


def test_a_grey_stabiliser_before_and_after_a_colour_one_is_what_it_was():
    grey, _ = SM.jitter_scene(0)
    frames = CM.coloured(grey, 3)
    args = _scene_args()
    want = _sequence(grey, *args)
    before, colour, after = _stabilizer(grey.shape[1:], *args), _stabilizer(frames.shape[1:], *args), None
    try:
        got = [before.push(np.ascontiguousarray(f)) for f in grey[:7]]
        _stream_host(colour, frames)
        got += [before.push(np.ascontiguousarray(f)) for f in grey[7:]]
        rest = before.flush()
        out = np.stack([g[1] for g in got if g[0] >= 0] + list(rest[1]))
        corr = np.stack([g[2] for g in got if g[0] >= 0] + list(rest[2]))
        SM.same(out, want[0], "a grey stabiliser around a colour one: out")
        SM.same(corr, want[1], "a grey stabiliser around a colour one: correction")
        after = _stabilizer(grey.shape[1:], *args)
        o, c, _ = _stream_host(after, grey)
        SM.same(o, want[0], "a grey stabiliser made after a colour one: out")
        SM.same(c, want[1], "a grey stabiliser made after a colour one: correction")
    finally:
        for x in (before, colour, after):
            if x is not None:
                x.close()


def test_the_python_class_takes_colour_frames():
    import lucas_kanade_pyramidal as P

    grey, _ = SM.jitter_scene(0)
    frames = CM.coloured(grey, 3)
    s = SCENE
    kw = dict(model="translation", radius=s["r"], sigma=s["sigma"], hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"],
              quality_level=s["q"], min_distance=s["md"])
    want = P.lucas_kanade_pyramidal_sequence_stabilize(frames, s["K"], s["D"], order="bgr", **kw)
    with P.OnlineStabilizer(frames.shape[1:], s["K"], s["D"], inside=True, order="bgr", **kw) as st:
        got = [e for e in (st.push(f) for f in frames) if e is not None] + st.flush()
    assert [g.index for g in got] == list(range(len(frames)))
    assert got[0].frame.shape == frames.shape[1:] and got[0].inside.shape == frames.shape[1:3] and got[0].inside.dtype == bool
    SM.same(np.stack([g.frame for g in got]), want.frames, "frames")
    SM.same(np.stack([g.correction for g in got]), want.correction, "correction")


# ---------------------------------------------------------------------------------------------------------------------
# the mosaic
# ---------------------------------------------------------------------------------------------------------------------
def test_the_colour_mosaic_is_the_planar_composite_of_every_channel_under_the_luma_chain():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P
    import mosaic_model as M

    T, H, W, step = 6, 96, 128, 5
    image = M.smooth_field(H + 8, W + step * (T - 1) + 8, 3)
    colour = CM.coloured(image, 3)
    frames = np.stack([M.pan_frames(np.ascontiguousarray(colour[..., c]), T, H, W, step, 0, 4, 4)[0] for c in range(3)], -1)
    kw = dict(max_corners=300, detect_every=4, hypotheses=128, seed=5, anchor=2, blend="feather")
    got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, order="bgr", **kw)
    grey = P.lucas_kanade_pyramidal_sequence_mosaic(K.rgb_to_luma(frames, "bgr"), **kw)
    chain = K.mosaic_chain(grey.model, grey.status, (H, W), anchor=2)
    assert got.origin == grey.origin == chain.origin and got.canvas.shape == grey.canvas.shape + (3,)
    SM.same(got.count, grey.count, "count")
    assert not grey.dropped.any() and grey.count.max() == T
    for c in range(3):
        want = K.mosaic_composite(np.ascontiguousarray(frames[..., c]), chain.from_anchor, chain.canvas_shape, chain.origin,
                                  chain.dropped, "feather")
        SM.same(got.canvas[..., c], want, f"canvas, plane {c}")
    both, cnt = K.mosaic_composite(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", return_count=True)
    SM.same(both, got.canvas, "mosaic_composite of the colour frames")
    SM.same(cnt, grey.count, "mosaic_composite's count")
