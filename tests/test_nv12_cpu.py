"""CPU tests of NV12 video: the statement (tests/nv12_model.py) against its consequences and against an independently written
form of the chroma map, and every NV12 wrapper's and host form's refusals, which come before any device call (so they are the
same with and without a GPU)."""
import ctypes

import numpy as np
import pytest

import nv12_model as NM
import stabilize_model as SM

SITINGS = sorted(NM.SITINGS)


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("siting", SITINGS)
def test_the_identity_returns_every_byte_with_inside_all_1(siting):
    H, W = 6, 10
    frames = NM.random_frames(2, H, W, 1)
    ident = np.tile(SM.IDENTITY, (2, 1))
    for what, (out, ins) in (("affine", NM.warp_affine(frames, ident, siting)),
                             ("perspective", NM.warp_perspective(frames, NM.as_homography(ident), siting))):
        SM.same(out, frames, f"{what}, {siting}")
        assert ins.shape == (2, H, W) and ins.dtype == np.uint8 and (ins == 1).all(), (what, siting)


@pytest.mark.parametrize("siting", SITINGS)
def test_a_third_row_0_0_1_returns_the_affine_bytes(siting):
    H, W = 8, 12
    frames = NM.random_frames(2, H, W, 2)
    for name, maps in NM.affine_maps(H, W).items():
        want, want_in = NM.warp_affine(frames, maps, siting)
        got, got_in = NM.warp_perspective(frames, NM.as_homography(maps), siting)
        SM.same(got, want, f"{name}, {siting}")
        SM.same(got_in, want_in, f"{name}, {siting}: inside")
        for f in range(2):
            SM.same(NM.chroma_map(NM.as_homography(maps[f]), siting)[:6], NM.chroma_map(maps[f], siting), f"{name}: mc")


@pytest.mark.parametrize("kind", ["affine", "perspective"])
@pytest.mark.parametrize("siting", SITINGS)
def test_an_even_translation_shifts_y_by_it_and_uv_by_half_of_it(siting, kind):
    """the map takes an output pixel to its source: (x, y) -> (x + 4, y - 2), so out[y][x] = in[y - 2][x + 4] where that
    lies in the frame; zeros (Y) and 128s (U, V) fill the uncovered margin"""
    H, W, dx, dy = 8, 12, 4, -2
    frames = NM.random_frames(1, H, W, 3)
    m = np.array([[1.0, 0, dx, 0, 1, dy]])
    out, ins = NM.warp_affine(frames, m, siting) if kind == "affine" else NM.warp_perspective(frames, NM.as_homography(m), siting)
    y, uv = NM.planes(frames)
    oy, ouv = NM.planes(out)
    want_y, want_in = np.zeros_like(y), np.zeros_like(y)
    want_y[:, -dy:, :W - dx] = y[:, :H + dy, dx:]
    want_in[:, -dy:, :W - dx] = 1
    want_uv = np.full_like(uv, 128)
    want_uv[:, -dy // 2:, :(W - dx) // 2] = uv[:, :(H + dy) // 2, dx // 2:]
    SM.same(oy, want_y, "Y")
    SM.same(ins, want_in, "inside")
    SM.same(ouv, want_uv, "UV")


@pytest.mark.parametrize("siting", SITINGS)
def test_the_affine_chroma_map_is_the_luma_map_between_the_two_conversions(siting):
    """the other form: the luma position of chroma sample (i, j), mapped, converted back, in float64.  On maps whose
    coefficients are halves and quarters every product and sum is exact in both forms, so the two agree to the bit"""
    sx, sy = NM.SITINGS[siting]
    i, j = np.meshgrid(np.arange(9, dtype=np.float64), np.arange(7, dtype=np.float64))
    for m in ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [1.25, -0.5, 3.75, 0.25, 0.75, -6.5], [0.5, 0.25, -1.25, -0.75, 1.5, 2.0],
              [-1.0, 2.0, 0.5, 0.5, -0.25, 100.25]):
        m = np.array(m)
        mc = NM.chroma_map(m, siting)
        x, y = 2.0 * i + sx, 2.0 * j + sy
        xs, ys = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        want_x, want_y = (xs - sx) / 2.0, (ys - sy) / 2.0
        got_x, got_y = SM.coordinates(mc, 7, 9)
        SM.same(got_x, want_x, f"x under {m.tolist()}")
        SM.same(got_y, want_y, f"y under {m.tolist()}")


def test_outside_chroma_is_128_and_outside_luma_is_0():
    H, W = 6, 8
    frames = NM.random_frames(1, H, W, 4)
    out, ins = NM.warp_affine(frames, np.array([[1.0, 0, 4.0 * W, 0, 1, 0]]))
    oy, ouv = NM.planes(out)
    assert not ins.any() and not oy.any() and (ouv == 128).all()
    out, ins = NM.warp_affine(frames, np.array([[1.0, np.nan, 0, 0, 1, 0]]))
    oy, ouv = NM.planes(out)
    assert not ins.any() and not oy.any() and (ouv == 128).all(), "a NaN coefficient is outside everywhere"


def test_planes_and_from_planes_are_inverse_views():
    import lucas_kanade_pyramidal as P

    x = NM.random_frames(3, 6, 10, 5)
    y, uv = P.nv12_planes(x)
    assert y.shape == (3, 6, 10) and uv.shape == (3, 3, 5, 2)
    assert np.shares_memory(y, x) and np.shares_memory(uv, x), "views, not copies"
    flat = x.reshape(3, -1)
    assert np.array_equal(y.reshape(3, -1), flat[:, :60]) and np.array_equal(uv.reshape(3, -1), flat[:, 60:])
    assert uv[1, 2, 3, 0] == flat[1, 60 + 2 * 10 + 6] and uv[1, 2, 3, 1] == flat[1, 60 + 2 * 10 + 7], "U at byte 0, V at byte 1"
    SM.same(P.nv12_from_planes(y, uv), x, "round trip")
    y1, uv1 = P.nv12_planes(x[0])
    assert y1.shape == (6, 10) and uv1.shape == (3, 5, 2)
    SM.same(P.nv12_from_planes(y1, uv1), x[0], "round trip of one frame")
    my, muv = NM.planes(x)
    SM.same(my, y, "the model's planes")
    SM.same(muv, uv, "the model's planes")


# ---------------------------------------------------------------------------------------------------------------------
# refusals, before any device call
# ---------------------------------------------------------------------------------------------------------------------
def _seq_tail(w):
    """the arguments of oflk_stabilize_sequence_u8 between the shape and `out`: valid ones"""
    import _oflk

    return (1, 5, 3, 0.01, 0.5, 4.0, 0.05, 5.0, 16, 4, 0, 32, 1.0, 0, _oflk._f64(w), len(w) - 1)


def test_every_c_entry_point_refuses_bad_nv12_arguments_before_any_device_call():
    import _oflk

    L = _oflk.lib()
    INV, UNS = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED
    H, W = 32, 32
    buf = np.zeros(2 * H * W * 3 // 2, np.uint8)
    out = np.zeros_like(buf)
    m = np.zeros(18, np.float64)
    p, o = buf.ctypes.data, out.ctypes.data
    w = SM.weights(1)
    assert _oflk.OFLK_SITING_LEFT == 0 and _oflk.OFLK_SITING_CENTER == 1
    # the frame size: 0 for a shape the calls refuse
    fb = L.oflk_nv12_frame_bytes
    assert fb(H, W) == H * W * 3 // 2 and fb(4, 4) == 24 and fb(1080, 1920) == 3110400
    for h, ww in ((3, 4), (4, 3), (2, 4), (4, 2), (5, 8), (8, 5), (0, 4), (-2, 4), (32768, 32768)):
        assert fb(h, ww) == 0, (h, ww)
    # warps: (frames, F, H, W, siting, map, out, inside)
    for fn, tail in ((L.oflk_warp_affine_nv12, (None,)), (L.oflk_warp_perspective_nv12, (None,)),
                     (L.oflk_warp_affine_nv12_host, ()), (L.oflk_warp_perspective_nv12_host, ())):
        mp = m.ctypes.data if tail else _oflk._f64(m)
        for args in ((p, 2, 31, W, 0, mp, o, None), (p, 2, H, 31, 0, mp, o, None), (p, 2, 2, W, 0, mp, o, None),
                     (p, 2, H, 2, 0, mp, o, None), (p, 2, H, W, 2, mp, o, None), (p, 2, H, W, -1, mp, o, None),
                     (p, 0, H, W, 0, mp, o, None), (None, 2, H, W, 0, mp, o, None), (p, 2, H, W, 0, None, o, None),
                     (p, 2, H, W, 1, mp, None, None)):
            assert fn(*args, *tail) == INV, (fn, args)
        assert fn(p, 1, 32768, 32768, 0, mp, o, None, *tail) == UNS, "2^30 pixels"
    assert L.oflk_warp_affine_nv12(p, 2, H, W, 0, m.ctypes.data + 4, o, None, None) == INV, "d_map not 8-byte aligned"
    assert L.oflk_warp_perspective_nv12(p, 2, H, W, 0, m.ctypes.data + 4, o, None, None) == INV, "d_map not 8-byte aligned"
    # the sequence call: (frames, T, H, W, siting, ..., out, correction, model, counts, held)
    seq = L.oflk_stabilize_sequence_nv12
    rest = (None, None, None, None)
    for head in ((p, 2, 31, W, 0), (p, 2, H, 30 + 1, 0), (p, 2, 2, W, 0), (p, 2, H, W, 2), (None, 2, H, W, 0), (p, 1, H, W, 0)):
        assert seq(*head, *_seq_tail(w), o, *rest) == INV, head
    assert seq(p, 2, H, W, 0, *_seq_tail(w), None, *rest) == INV, "NULL out"
    assert seq(p, 2, 32768, 32768, 0, *_seq_tail(w), o, *rest) == UNS
    bad = list(_seq_tail(w))
    bad[9] = 0   # detect_every
    assert seq(p, 2, H, W, 0, *bad, o, *rest) == INV, "what the grey call refuses"
    # the stabiliser: (st, device, H, W, siting, ...)
    h = ctypes.c_void_p()
    create = L.oflk_stabilizer_create_nv12
    for head in ((0, 31, W, 0), (0, H, 31, 0), (0, 2, W, 0), (0, H, W, 2), (0, H, W, -1)):
        assert create(ctypes.byref(h), *head, *_seq_tail(w)) == INV and not h.value, head
    assert create(None, 0, H, W, 0, *_seq_tail(w)) == INV
    bad = list(_seq_tail(w))
    bad[10] = 7   # model
    assert create(ctypes.byref(h), 0, H, W, 0, *bad) == INV and not h.value, "what the grey form refuses"
    # creation makes no device call: an NV12 stabiliser exists without a GPU, holds nothing, and refuses NULL frames
    assert create(ctypes.byref(h), 0, H, W, 1, *_seq_tail(w)) == 0 and h.value
    try:
        assert L.oflk_stabilizer_workspace_bytes(h) == 0 and L.oflk_stabilizer_lag(h) == 1 and L.oflk_stabilizer_frame_index(h) == -1
        e = ctypes.c_int(5)
        assert L.oflk_stabilizer_push(h, None, o, None, None, ctypes.byref(e)) == INV and e.value == -1
    finally:
        L.oflk_stabilizer_destroy(h)


def test_every_python_wrapper_refuses_bad_nv12_input_before_any_device_call():
    import lucas_kanade_pyramidal as P

    good = NM.random_frames(3, 8, 8, 0)   # (3, 12, 8)
    ident = np.tile(SM.IDENTITY, (3, 1))
    ident9 = NM.as_homography(ident)
    bad_frames = [good.astype(np.float32),
                  np.zeros((3, 10, 8), np.uint8),    # a height that is not 3H/2
                  np.zeros((3, 11, 8), np.uint8),
                  np.zeros((3, 12, 7), np.uint8),    # odd W
                  np.zeros((3, 3, 8), np.uint8),     # H = 2
                  np.zeros((3, 12, 2), np.uint8),    # W = 2
                  np.zeros((0, 12, 8), np.uint8),
                  np.zeros((3, 12, 8, 1), np.uint8)]
    for f in bad_frames:
        for call in (lambda: P.nv12_planes(f), lambda: P.warp_affine_nv12(f, ident[:len(f)]),
                     lambda: P.warp_perspective_nv12(f, ident9[:len(f)]),
                     lambda: P.lucas_kanade_pyramidal_sequence_stabilize_nv12(f, 16, 4)):
            with pytest.raises(ValueError):
                call()
    # an odd H: its 3H/2 is no integer, so such a frame cannot be written as (3H/2, W); the planes refuse it
    with pytest.raises(ValueError):
        P.nv12_from_planes(np.zeros((2, 5, 8), np.uint8), np.zeros((2, 2, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        P.nv12_from_planes(np.zeros((2, 6, 7), np.uint8), np.zeros((2, 3, 3, 2), np.uint8))
    with pytest.raises(ValueError):
        P.nv12_from_planes(np.zeros((2, 6, 8), np.uint8), np.zeros((2, 3, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        P.nv12_from_planes(np.zeros((2, 6, 8), np.float32), np.zeros((2, 3, 4, 2), np.uint8))
    for call in (lambda: P.warp_affine_nv12(good, ident, siting="right"), lambda: P.warp_affine_nv12(good, ident, siting=0),
                 lambda: P.warp_affine_nv12(good, ident[:2]), lambda: P.warp_affine_nv12(good, ident9),
                 lambda: P.warp_perspective_nv12(good, ident),
                 lambda: P.lucas_kanade_pyramidal_sequence_stabilize_nv12(good, 16, 4, siting="top"),
                 lambda: P.lucas_kanade_pyramidal_sequence_stabilize_nv12(good[:1], 16, 4),
                 lambda: P.lucas_kanade_pyramidal_sequence_stabilize_nv12(good, 16, 4, refine_iterations=-1),
                 lambda: P.OnlineStabilizer((32, 32), 16, layout="nv21"), lambda: P.OnlineStabilizer((32, 32), 16, layout="nv12", siting="top"),
                 lambda: P.OnlineStabilizer((31, 32), 16, layout="nv12"), lambda: P.OnlineStabilizer((32, 30 + 1), 16, layout="nv12"),
                 lambda: P.OnlineStabilizer((48, 32, 1), 16, layout="nv12"), lambda: P.OnlineStabilizer((32, 32), 16, layout="nv12", order="rgb"),
                 lambda: P.OnlineStabilizer((32, 32), 16, layout="nv12", dtype=np.float32)):
        with pytest.raises(ValueError):
            call()
    with P.OnlineStabilizer((32, 32), 16, radius=2, num_levels=1, layout="nv12", siting="center") as st:   # no device call so far
        assert st.shape == (48, 32) and st.lag == 2 and st.frame_index == -1
        with pytest.raises(ValueError):
            st.push(np.zeros((32, 32), np.uint8))
        with pytest.raises(ValueError):
            st.push(np.zeros((32, 32, 3), np.uint8))
    with P.OnlineStabilizer((32, 32), 16, radius=2, num_levels=1) as st:   # layout=None: the grey stabiliser it always was
        assert st.shape == (32, 32)
        with pytest.raises(ValueError):
            st.push(np.zeros((48, 32), np.uint8))


def test_a_3d_array_is_never_guessed_to_be_nv12(monkeypatch):
    import _oflk
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    calls = []

    def grey(frames, maps, inside=False):
        calls.append(("grey", frames.shape, maps.shape))
        return np.zeros_like(frames), np.zeros(frames.shape, np.uint8)

    def nv12(frames, maps, siting=0, inside=False):
        calls.append(("nv12", frames.shape, maps.shape, siting))
        return np.zeros_like(frames), np.zeros((frames.shape[0], 2 * frames.shape[1] // 3, frames.shape[2]), np.uint8)

    monkeypatch.setattr(_oflk, "warp_affine_host", grey)
    monkeypatch.setattr(_oflk, "warp_nv12_host", nv12)
    a = np.zeros((2, 12, 8), np.uint8)
    K.warp_affine(a, np.tile(SM.IDENTITY, (2, 1)))
    out, ins = P.warp_affine_nv12(a, np.tile(SM.IDENTITY, (2, 1)), "center", return_inside=True)
    assert out.shape == (2, 12, 8) and ins.shape == (2, 8, 8) and ins.dtype == bool
    out = P.warp_perspective_nv12(a[0], NM.as_homography(SM.IDENTITY))
    assert out.shape == (12, 8)
    assert calls == [("grey", (2, 12, 8), (2, 6)), ("nv12", (2, 12, 8), (2, 6), 1), ("nv12", (1, 12, 8), (1, 9), 0)]


def test_without_a_gpu_the_nv12_calls_fail_loudly():
    """no quiet CPU path: with valid arguments and no device the NV12 calls raise OFLK_ERR_NO_DEVICE"""
    import _oflk
    import lucas_kanade_pyramidal as P

    if _oflk.device_count() > 0:
        pytest.skip("a GPU is visible here")
    x = NM.random_frames(2, 8, 8, 0)
    for call in (lambda: P.warp_affine_nv12(x, np.tile(SM.IDENTITY, (2, 1))),
                 lambda: P.warp_perspective_nv12(x, NM.as_homography(np.tile(SM.IDENTITY, (2, 1))))):
        with pytest.raises(_oflk.OflkError) as e:
            call()
        assert e.value.code == _oflk.OFLK_ERR_NO_DEVICE
