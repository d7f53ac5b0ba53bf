"""CPU tests of colour video: the statement (tests/colour_model.py) against independently written forms, and every colour
wrapper's and host form's refusals, which come before any device call (so they are the same with and without a GPU)."""
import ctypes

import numpy as np
import pytest

import colour_model as CM
import homography_model as HM
import stabilize_model as SM


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def _sweep():
    """every (R, G, B) with each value in 0, 5, 10 .. 255 and the neighbours of the ends: (N, 3) uint8"""
    v = np.unique(np.concatenate([np.arange(0, 256, 5), [1, 2, 253, 254, 255]])).astype(np.uint8)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    return np.stack([r.ravel(), g.ravel(), b.ravel()], -1)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("channels", [3, 4])
def test_the_luma_model_equals_a_form_written_another_way(order, channels):
    """the other form: the weighted sum as an exact float64 fraction of 256, rounded half up by floor(x + 0.5) -- every value
    involved is a multiple of 1/256 below 2^53, so float64 holds it exactly; and Python integers on a few triples"""
    rgb = _sweep()
    px = rgb if order == "rgb" else rgb[:, ::-1]
    if channels == 4:
        px = np.concatenate([px, np.random.default_rng(0).integers(0, 256, (len(px), 1), dtype=np.uint8)], -1)
    got = CM.luma(np.ascontiguousarray(px), order)
    r, g, b = (rgb[:, k].astype(np.float64) for k in range(3))
    want = np.floor((77.0 * r + 150.0 * g + 29.0 * b) / 256.0 + 0.5)
    assert got.dtype == np.uint8 and got.shape == (len(rgb),)
    assert np.array_equal(got.astype(np.float64), want)
    assert want.min() >= 0 and want.max() <= 255, "the luma never leaves [0, 255]"
    for i in range(0, len(rgb), 997):
        R, G, B = (int(x) for x in rgb[i])
        assert int(got[i]) == (77 * R + 150 * G + 29 * B + 128) // 256


def test_grey_input_returns_itself_and_the_weights_sum_to_256():
    assert sum(CM.WEIGHTS) == 256
    g = np.arange(256, dtype=np.uint8)
    for order in CM.ORDERS:
        for c in CM.CHANNELS:
            px = np.stack([g] * 3 + [255 - g] * (c - 3), -1)
            assert np.array_equal(CM.luma(px, order), g), (order, c)
    assert int(CM.luma(np.uint8([[255, 255, 255]]))[0]) == 255 and int(CM.luma(np.uint8([[0, 0, 0]]))[0]) == 0


def test_the_orders_differ_exactly_by_the_swap_of_bytes_0_and_2():
    px = CM.random_frames(1, 5, 7, 4, 3)
    swapped = px.copy()
    swapped[..., [0, 2]] = px[..., [2, 0]]
    assert np.array_equal(CM.luma(px, "rgb"), CM.luma(swapped, "bgr"))
    assert (CM.luma(px, "rgb") != CM.luma(px, "bgr")).any()


@pytest.mark.parametrize("channels", [3, 4])
def test_the_packed_warp_model_is_the_planar_models_plane_by_plane(channels):
    H, W = 7, 13
    frames = CM.random_frames(3, H, W, channels, 11)
    maps = np.stack([CM.affine_maps(H, W)[k] for k in ("half-pixel shift", "rotation 7 deg, scale 1.1", "NaN coefficient")])
    out, ins = CM.warp_affine(frames, maps)
    assert out.shape == frames.shape and out.dtype == np.uint8 and ins.shape == (3, H, W)
    for c in range(channels):
        want, want_in = SM.warp(np.ascontiguousarray(frames[..., c]), maps)
        SM.same(out[..., c], want, f"affine, plane {c}")
        SM.same(ins, want_in, f"affine, inside against plane {c}'s")
    assert not ins[2].any() and not out[2].any() and ins[0].any() and not ins[0].all()
    pm = CM.perspective_maps(H, W)
    maps9 = np.stack([pm["mild homography"], pm["w changes sign"], pm["affine: rotation 7 deg, scale 1.1"]])
    out9, ins9 = CM.warp_perspective(frames, maps9)
    for c in range(channels):
        want, want_in = HM.warp(np.ascontiguousarray(frames[..., c]), maps9)
        SM.same(out9[..., c], want, f"perspective, plane {c}")
        SM.same(ins9, want_in, f"perspective, inside against plane {c}'s")
    assert ins9[1][:, 0].all() and not ins9[1][:, W // 2 + 1:].any(), "w changes sign inside the frame"
    SM.same(out9[2], CM.warp_affine(frames[2:], maps9[2, :6][None])[0][0], "third row (0, 0, 1): the affine bytes")


# ---------------------------------------------------------------------------------------------------------------------
# refusals, before any device call
# ---------------------------------------------------------------------------------------------------------------------
def _seq_tail(w):
    """the arguments of oflk_stabilize_sequence_u8 between the shape and `out`: valid ones"""
    import _oflk

    return (1, 5, 3, 0.01, 0.5, 4.0, 0.05, 5.0, 16, 4, 0, 32, 1.0, 0, _oflk._f64(w), len(w) - 1)


def test_every_c_entry_point_refuses_bad_colour_arguments_before_any_device_call():
    import _oflk

    L = _oflk.lib()
    INV, UNS = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED
    H, W, C = 32, 32, 3
    buf = np.zeros(2 * H * W * 4, np.uint8)
    out = np.zeros_like(buf)
    m = np.zeros(18, np.float64)
    p, o = buf.ctypes.data, out.ctypes.data
    w = SM.weights(1)
    # luma: (frames, F, H, W, channels, order, luma)
    for fn, tail in ((L.oflk_luma_u8, (None,)), (L.oflk_luma_u8_host, ())):
        for args in ((p, 2, H, W, 2, 0, o), (p, 2, H, W, 5, 0, o), (p, 2, H, W, 1, 0, o), (p, 2, H, W, C, 2, o), (p, 2, H, W, C, -1, o),
                     (None, 2, H, W, C, 0, o), (p, 2, H, W, C, 0, None), (p, 2, 1, W, C, 0, o), (p, 2, H, 1, C, 0, o), (p, 0, H, W, C, 0, o)):
            assert fn(*args, *tail) == INV, (fn, args)
        assert fn(p, 1, 32768, 32768, C, 0, o, *tail) == UNS, "2^30 pixels"
        assert fn(p, 1, 30000, 30000, C, 0, o, *tail) == UNS, "fewer than 2^30 pixels, 2^31 bytes or more"
    # warps: (frames, F, H, W, channels, map, out, inside)
    for fn, tail in ((L.oflk_warp_affine_packed, (None,)), (L.oflk_warp_perspective_packed, (None,)),
                     (L.oflk_warp_affine_packed_host, ()), (L.oflk_warp_perspective_packed_host, ())):
        mp = m.ctypes.data if tail else _oflk._f64(m)
        for args in ((p, 2, H, W, 2, mp, o, None), (p, 2, H, W, 5, mp, o, None), (None, 2, H, W, C, mp, o, None),
                     (p, 2, H, W, C, None, o, None), (p, 2, H, W, C, mp, None, None), (p, 2, 1, W, C, mp, o, None),
                     (p, 2, H, 1, C, mp, o, None), (p, 0, H, W, C, mp, o, None)):
            assert fn(*args, *tail) == INV, (fn, args)
        assert fn(p, 1, 32768, 32768, 4, mp, o, None, *tail) == UNS
        assert fn(p, 1, 30000, 30000, C, mp, o, None, *tail) == UNS
    assert L.oflk_warp_affine_packed(p, 2, H, W, C, m.ctypes.data + 4, o, None, None) == INV, "d_map not 8-byte aligned"
    # the sequence call: (frames, T, H, W, channels, order, ..., out, correction, model, counts, held)
    seq = L.oflk_stabilize_sequence_packed
    rest = (None, None, None, None)
    for head in ((p, 2, H, W, 2, 0), (p, 2, H, W, C, 2), (None, 2, H, W, C, 0), (p, 1, H, W, C, 0), (p, 2, 1, W, C, 0)):
        assert seq(*head, *_seq_tail(w), o, *rest) == INV, head
    assert seq(p, 2, H, W, C, 0, *_seq_tail(w), None, *rest) == INV, "NULL out"
    assert seq(p, 2, 30000, 30000, C, 0, *_seq_tail(w), o, *rest) == UNS
    bad = list(_seq_tail(w))
    bad[9] = 0   # detect_every
    assert seq(p, 2, H, W, C, 0, *bad, o, *rest) == INV, "what the grey call refuses"
    # the stabiliser: (st, device, H, W, channels, order, ...)
    h = ctypes.c_void_p()
    create = L.oflk_stabilizer_create_packed
    for head in ((0, H, W, 2, 0), (0, H, W, 5, 0), (0, H, W, C, 2), (0, 1, W, C, 0)):
        assert create(ctypes.byref(h), *head, *_seq_tail(w)) == INV and not h.value, head
    assert create(None, 0, H, W, C, 0, *_seq_tail(w)) == INV
    assert create(ctypes.byref(h), 0, 30000, 30000, C, 0, *_seq_tail(w)) == UNS and not h.value
    # creation makes no device call: a packed stabiliser exists without a GPU, holds nothing, and refuses NULL frames
    assert create(ctypes.byref(h), 0, H, W, 4, 1, *_seq_tail(w)) == 0 and h.value
    try:
        assert L.oflk_stabilizer_workspace_bytes(h) == 0 and L.oflk_stabilizer_lag(h) == 1 and L.oflk_stabilizer_frame_index(h) == -1
        e = ctypes.c_int(5)
        assert L.oflk_stabilizer_push(h, None, o, None, None, ctypes.byref(e)) == INV and e.value == -1
    finally:
        L.oflk_stabilizer_destroy(h)


def test_every_python_wrapper_refuses_bad_colour_input_before_any_device_call():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    rgb = CM.random_frames(3, 8, 8, 3, 0)
    ident = np.tile(SM.IDENTITY, (3, 1))
    ident9 = np.tile(CM.as_homography(SM.IDENTITY), (3, 1))
    bad_frames = [rgb.astype(np.float32), CM.random_frames(3, 8, 8, 4, 0)[..., :2], np.zeros((3, 8, 8, 5), np.uint8),
                  np.zeros((3, 1, 8, 3), np.uint8), np.zeros((0, 8, 8, 3), np.uint8)]
    for f in bad_frames:
        with pytest.raises(ValueError):
            K.rgb_to_luma(f)
        with pytest.raises(ValueError):
            K.warp_affine(f, ident[:len(f)])
        with pytest.raises(ValueError):
            K.warp_perspective(f, ident9[:len(f)])
        with pytest.raises(ValueError):
            K.mosaic_composite(f, ident9[:len(f)], (8, 8))
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_stabilize(f, 16, 4)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_mosaic(f, 16, 4)
    for call in (lambda: K.rgb_to_luma(rgb, order="gbr"), lambda: K.rgb_to_luma(rgb, order=0), lambda: K.rgb_to_luma(rgb[0, 0]),
                 lambda: K.rgb_to_luma(np.zeros((2, 3, 8, 8, 3), np.uint8)), lambda: K.warp_affine(rgb, ident[:2]),
                 lambda: K.warp_affine(rgb, ident9), lambda: K.warp_perspective(rgb, ident),
                 lambda: P.lucas_kanade_pyramidal_sequence_stabilize(rgb, 16, 4, order="yuv"),
                 lambda: P.lucas_kanade_pyramidal_sequence_stabilize(rgb[:1], 16, 4),
                 lambda: P.lucas_kanade_pyramidal_sequence_mosaic(rgb, 16, 4, order="yuv"),
                 lambda: P.OnlineStabilizer((8, 8, 2), 16, order="rgb"), lambda: P.OnlineStabilizer((8, 8, 5), 16, order="rgb"),
                 lambda: P.OnlineStabilizer((8, 8, 3), 16, order="yuv"),
                 lambda: P.OnlineStabilizer((32, 32, 3), 16, order="rgb", dtype=np.float32),
                 lambda: P.OnlineStabilizer((8, 8, 3, 1), 16, order="rgb"),
                 lambda: P.OnlineStabilizer((32, 32, 3), 16)):   # colour needs its order spelled out
        with pytest.raises(ValueError):
            call()
    with P.OnlineStabilizer((32, 32, 3), 16, radius=2, num_levels=1, order="rgb") as st:   # no device call so far
        assert st.shape == (32, 32, 3) and st.lag == 2 and st.frame_index == -1
        with pytest.raises(ValueError):
            st.push(np.zeros((32, 32), np.uint8))
        with pytest.raises(ValueError):
            st.push(np.zeros((32, 32, 4), np.uint8))


def test_a_4d_float32_array_is_refused_and_a_3d_array_still_goes_to_the_grey_path(monkeypatch):
    import _oflk
    import lucas_kanade_core as K

    calls = []

    def grey(frames, maps, inside=False):
        calls.append(("grey", frames.shape, maps.shape))
        return np.zeros_like(frames), np.zeros(frames.shape, np.uint8)

    def packed(frames, maps, inside=False):
        calls.append(("packed", frames.shape, maps.shape))
        return np.zeros_like(frames), np.zeros(frames.shape[:3], np.uint8)

    monkeypatch.setattr(_oflk, "warp_affine_host", grey)
    monkeypatch.setattr(_oflk, "warp_packed_host", packed)
    # (3, 8, 3): three grey frames of 8 x 3, not one colour frame
    a3 = np.zeros((3, 8, 3), np.uint8)
    out, ins = K.warp_affine(a3, np.tile(SM.IDENTITY, (3, 1)), return_inside=True)
    assert out.shape == (3, 8, 3) and ins.shape == (3, 8, 3) and ins.dtype == bool
    K.warp_perspective(a3.astype(np.float32), np.tile(CM.as_homography(SM.IDENTITY), (3, 1)))
    K.warp_affine(a3[0], SM.IDENTITY)
    assert calls == [("grey", (3, 8, 3), (3, 6)), ("grey", (3, 8, 3), (3, 9)), ("grey", (1, 8, 3), (1, 6))]
    del calls[:]
    a4 = np.zeros((2, 8, 8, 3), np.uint8)
    out, ins = K.warp_affine(a4, np.tile(SM.IDENTITY, (2, 1)), return_inside=True)
    assert out.shape == a4.shape and ins.shape == (2, 8, 8) and ins.dtype == bool
    assert K.warp_perspective(np.zeros((2, 8, 8, 4), np.uint8), np.tile(CM.as_homography(SM.IDENTITY), (2, 1))).shape == (2, 8, 8, 4)
    assert calls == [("packed", (2, 8, 8, 3), (2, 6)), ("packed", (2, 8, 8, 4), (2, 9))]
    del calls[:]
    for f in (a4.astype(np.float32), a4.astype(np.float64), a4.astype(np.uint16)):
        with pytest.raises(ValueError, match="uint8"):
            K.warp_affine(f, np.tile(SM.IDENTITY, (2, 1)))
        with pytest.raises(ValueError, match="uint8"):
            K.warp_perspective(f, np.tile(CM.as_homography(SM.IDENTITY), (2, 1)))
    assert calls == []


def test_without_a_gpu_the_colour_calls_fail_loudly():
    """no quiet CPU path: with valid arguments and no device the colour calls raise OFLK_ERR_NO_DEVICE"""
    import _oflk
    import lucas_kanade_core as K

    if _oflk.device_count() > 0:
        pytest.skip("a GPU is visible here")
    rgb = CM.random_frames(2, 8, 8, 3, 0)
    for call in (lambda: K.rgb_to_luma(rgb), lambda: K.warp_affine(rgb, np.tile(SM.IDENTITY, (2, 1)))):
        with pytest.raises(_oflk.OflkError) as e:
            call()
        assert e.value.code == _oflk.OFLK_ERR_NO_DEVICE
