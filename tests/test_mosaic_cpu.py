"""CPU tests of the video mosaic: the statement (tests/mosaic_model.py) against exact scenes, the perspective warp's statement
and independent restatements, and what the library and the Python wrappers refuse without a device.  No GPU is used."""
import ctypes

import numpy as np
import pytest

import homography_model as HM
import mosaic_model as M

# Measured with the committed model (the figure is in DESIGN.md section 2); the gate is four times the measured worst.
CHAIN_ROUND_TRIP = 7.88e-13   # worst |P_t o Q_t - I| over 130 frames: 129 planted homographies and planted_steps seeds 0 .. 3, three anchors

BLENDS = [M.MEAN, M.FEATHER, M.FIRST, M.LAST]


def translations(steps):
    return np.array([M.translation(dx, dy) for dx, dy in steps], np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchor", [0, 3, 6])
def test_integer_translations_chain_exactly(anchor):
    H, W = 9, 13
    steps = [(3, 0), (-2, 1), (5, -4), (0, 0), (7, 2), (-1, -1)]   # frame s to frame s + 1
    P, Q, box, held, dropped = M.chain(translations(steps), None, 7, anchor, H, W, 1000.0)
    pos = np.concatenate([[(0, 0)], np.cumsum(steps, 0)])   # anchor-0 coordinates to frame t's: + pos[t]
    for t in range(7):
        d = pos[t] - pos[anchor]
        assert np.array_equal(P[t], M.translation(d[0], d[1])) and np.array_equal(Q[t], M.translation(-d[0], -d[1])), t
        assert np.array_equal(box[t], [-d[0], -d[1], W - 1 - d[0], H - 1 - d[1]]), t
    assert not held.any() and not dropped.any()
    off = pos - pos[anchor]
    x0, y0, Wc, Hc = M.canvas(box, dropped)
    assert (x0, y0) == (int((-off[:, 0]).min()), int((-off[:, 1]).min()))
    assert (Wc, Hc) == (int((-off[:, 0]).max()) + W - x0, int((-off[:, 1]).max()) + H - y0)


def test_one_frame_is_its_own_canvas():
    P, Q, box, held, dropped = M.chain(np.zeros((0, 9), np.float32), None, 1, 0, 6, 8, 1.0)   # an extent under the frame: the anchor stays
    assert np.array_equal(P[0], M.IDENTITY) and np.array_equal(Q[0], M.IDENTITY) and held.size == 0 and not dropped[0]
    assert np.array_equal(box[0], [0, 0, 7, 5]) and M.canvas(box, dropped) == (0, 0, 8, 6)


def test_held_steps_are_the_identity():
    model = translations([(2, 0)] * 5)
    model[1, 4] = np.nan                       # a coefficient that is not finite
    model[2] = [1, 2, 0, 2, 4, 0, 0, 0, 1]     # singular: the adjugate's last entry is 1*4 - 2*2 = 0
    counts = np.ones((5, 3), np.int32)
    counts[3, 2] = 0                           # no model was found
    P, Q, box, held, dropped = M.chain(model, counts, 6, 0, 8, 8, 100.0)
    assert held.tolist() == [0, 1, 1, 1, 0] and not dropped.any()
    want = [0, 2, 2, 2, 2, 4]
    for t in range(6):
        assert np.array_equal(P[t], M.translation(want[t], 0)) and np.array_equal(Q[t], M.translation(-want[t], 0))
    # the same with the anchor at the far end: the held steps are the identity in both directions
    P, Q, box, held2, dropped = M.chain(model, counts, 6, 5, 8, 8, 100.0)
    assert np.array_equal(held2, held)
    for t in range(6):
        assert np.array_equal(P[t], M.translation(want[t] - 4, 0))


def drop_case(cause):
    """seven steps of a pan by 2 with one bad step (index 4, between frames 4 and 5); H = W = 17"""
    model = translations([(2, 0)] * 7)
    if cause == "w":           # B_4 = [1 0 0; 0 1 0; -1/8 0 1]: the corner x = 16 gets w = -1
        model[4] = [1, 0, 0, 0, 1, 0, 0.125, 0, 1]
    elif cause == "finite":    # P_5 = A_4 o P_4 with P_4's shift 8 and A_4's row (-1/8, 0, 1): the last entry is 0
        model[4] = [1, 0, 0, 0, 1, 0, -0.125, 0, 1]
    else:                      # a jump past the extent
        model[4] = M.translation(500, 0)
    return model


@pytest.mark.parametrize("cause", ["w", "finite", "extent"])
def test_each_drop_cause_drops_the_tail_and_never_the_anchor(cause):
    model = drop_case(cause)
    P, Q, box, held, dropped = M.chain(model, None, 8, 0, 17, 17, 100.0)
    assert dropped.tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and not held.any()
    assert np.isnan(box[5:]).all() and np.isfinite(box[:5]).all()
    X, Y, w = M.corners(Q[5], 17, 17)
    if cause == "w":
        assert np.isfinite(P[5]).all() and np.isfinite(Q[5]).all() and np.isfinite(X).all() and (w <= 0).any()
    elif cause == "finite":
        assert not np.isfinite(P[5]).all()
    else:
        assert np.isfinite(P[5]).all() and (w > 0).all() and np.abs(X).max() > 100.0
    # frames 6 and 7 are fine on their own and go with frame 5: the chain runs through it
    assert M.canvas(box, dropped) == (-8, 0, 25, 17)
    # anchored in the middle, only the side beyond the bad step goes; anchored beyond it, the other side
    if cause != "finite":   # that zero needs the shift of 8 that frame 4 has from frame 0
        assert M.chain(model, None, 8, 3, 17, 17, 100.0)[4].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    back = M.chain(model, None, 8, 6, 17, 17, 100.0)[4].tolist()
    assert back[5:] == [0, 0, 0]
    if cause == "extent":   # the jump is as long backwards; the projective steps are harmless read from the other side
        assert back[:5] == [1, 1, 1, 1, 1]
    # the anchor itself is never dropped, whatever the extent
    assert M.chain(model, None, 8, 5, 17, 17, 1.0)[4].tolist() == [1, 1, 1, 1, 1, 0, 1, 1]


def test_the_two_chains_invert_each_other_within_the_gate():
    worst = 0.0
    scenes = [np.tile(HM.planted_homography().astype(np.float32), (129, 1))] + [M.planted_steps(129, s) for s in range(4)]
    for steps in scenes:
        for anchor in (0, 64, 129):
            P, Q, _, held, _ = M.chain(steps, None, 130, anchor, 1080, 1920, 1e9)
            assert not held.any()
            worst = max(worst, max(np.abs(M.compose(P[t], Q[t]) - M.IDENTITY).max() for t in range(130)))
    print(f"worst |P o Q - I| = {worst:.3g}")
    assert worst <= 4 * CHAIN_ROUND_TRIP


def test_the_inverse_is_an_inverse_and_the_composition_a_product():
    rng = np.random.default_rng(5)
    for s in range(20):
        steps = M.planted_steps(2, s, scale=3.0)
        a, b, held = M.step(steps, None, 0)
        assert not held
        A, B = a.reshape(3, 3), b.reshape(3, 3)
        assert np.abs(A @ B / (A @ B)[2, 2] - np.eye(3)).max() < 1e-12
        c, _, _ = M.step(steps, None, 1)
        ref = A @ c.reshape(3, 3)
        assert np.allclose(M.compose(a, c).reshape(3, 3), ref / ref[2, 2], rtol=1e-13, atol=1e-13)
    assert rng is not None


# ---------------------------------------------------------------------------------------------------------------------
# accumulate and resolve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("blend", BLENDS)
def test_one_frame_on_its_own_canvas_is_the_perspective_warp(blend, u8):
    rng = np.random.default_rng(3)
    H, W = 19, 23
    frame = rng.integers(0, 256, (1, H, W)).astype(np.uint8) if u8 else (rng.random((1, H, W)) * 255).astype(np.float32)
    for m in [HM.planted_homography() * [1, 1, 0.01, 1, 1, 0.01, 1, 1, 1], M.translation(2.5, -1.25), M.translation(0, 0),
              np.array([1.1, 0.02, -3.0, -0.03, 0.9, 2.0, 1e-3, -2e-3, 1.0])]:
        want, inside = HM.warp(frame, m[None])
        out, count = M.composite(frame, m[None], None, 0, 0, H, W, blend)
        assert out.dtype == frame.dtype and out.tobytes() == want[0].tobytes()
        assert np.array_equal(count, inside[0].astype(np.int32))
        assert inside.any()


def test_the_feathered_single_sample_is_the_sample():
    """f32((g s) / g) == s for float32 s and the weights the feather forms: what the test above rests on"""
    rng = np.random.default_rng(0)
    s = (rng.standard_normal(200000) * 10.0 ** rng.uniform(-30, 30, 200000)).astype(np.float32).astype(np.float64)
    g = rng.uniform(0.0, 2000.0, 200000) + 1.0
    assert np.array_equal(((g * s) / g).astype(np.float32), s.astype(np.float32))


def pan_scene(u8=True):
    image = M.smooth_field(40, 90, 11)
    if not u8:
        image = image.astype(np.float32) * np.float32(0.37)
    return image, M.pan_frames(image, 7, 21, 30, 9, 2, 3, 1)


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("blend", BLENDS)
def test_an_integer_pan_gives_the_source_image_back(blend, u8):
    image, (frames, maps) = pan_scene(u8)
    Hc, Wc = image.shape
    out, count = M.composite(frames, maps, None, 0, 0, Hc, Wc, blend)
    cover = np.zeros((Hc, Wc), np.int32)
    for f in range(7):
        cover[1 + 2 * f:1 + 2 * f + 21, 3 + 9 * f:3 + 9 * f + 30] += 1
    assert np.array_equal(count, cover) and cover.max() >= 3 and (cover == 0).any()
    assert np.array_equal(out[cover > 0], image[cover > 0]) and (out[cover == 0] == 0).all()
    # a negative origin: the same picture on a canvas that begins left of and above the image
    out2, count2 = M.composite(frames, maps, None, -4, -2, Hc + 2, Wc + 4, blend)
    assert np.array_equal(out2[2:, 4:], out) and np.array_equal(count2[2:, 4:], count) and not count2[:2].any() and not count2[:, :4].any()


def test_the_mean_of_equal_values_is_the_value():
    for k in (2, 3, 7, 129):
        frames = np.tile(np.arange(12, dtype=np.uint8).reshape(1, 3, 4) * 21, (k, 1, 1))
        out, count = M.composite(frames, np.tile(M.IDENTITY, (k, 1)), None, 0, 0, 3, 4, M.MEAN)
        assert np.array_equal(out, frames[0]) and (count == k).all()
        f32 = (frames.astype(np.float32) + np.float32(0.1)) / np.float32(3)
        assert np.array_equal(M.composite(f32, np.tile(M.IDENTITY, (k, 1)), None, 0, 0, 3, 4, M.MEAN)[0], f32[0])


def test_first_and_last_differ_where_frames_disagree():
    H, W = 6, 8
    frames = np.stack([np.full((H, W), 10 * (f + 1), np.uint8) for f in range(3)])
    maps = np.stack([M.translation(-3 * f, 0) for f in range(3)])   # frame f covers canvas columns 3 f .. 3 f + 7
    first, count = M.composite(frames, maps, None, 0, 0, H, 14, M.FIRST)
    last, _ = M.composite(frames, maps, None, 0, 0, H, 14, M.LAST)
    assert first[0].tolist() == [10] * 8 + [20] * 3 + [30] * 3
    assert last[0].tolist() == [10] * 3 + [20] * 3 + [30] * 8
    assert np.array_equal(first != last, count > 1)
    # skip flags take a frame out of every mode
    skipped, c2 = M.composite(frames, maps, np.array([0, 1, 0], np.uint8), 0, 0, H, 14, M.LAST)
    assert skipped[0].tolist() == [10] * 6 + [30] * 8 and c2.max() == 2


@pytest.mark.parametrize("blend", BLENDS)
def test_accumulation_cut_anywhere_equals_the_uncut_call(blend):
    rng = np.random.default_rng(8)
    frames = (rng.random((5, 11, 14)) * 255).astype(np.float32)
    maps = np.stack([HM.planted_homography() * [1, 1, 0.01, 1, 1, 0.01, 1, 1, 1] + M.translation(-2.3 * f, 0.7 * f) - M.IDENTITY
                     for f in range(5)])
    whole = M.composite(frames, maps, None, -3, -2, 18, 30, blend)
    assert whole[1].max() >= 4
    for k in range(6):
        cut = M.composite(frames, maps, None, -3, -2, 18, 30, blend, cuts=(k,))
        assert cut[0].tobytes() == whole[0].tobytes() and np.array_equal(cut[1], whole[1]), k
    two = M.composite(frames, maps, None, -3, -2, 18, 30, blend, cuts=(1, 3))
    assert two[0].tobytes() == whole[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the library and the wrappers, without a device
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ["oflk_mosaic_chain", "oflk_mosaic_chain_host", "oflk_mosaic_canvas", "oflk_mosaic_state_bytes", "oflk_mosaic_accumulate",
           "oflk_mosaic_resolve", "oflk_mosaic_composite_host", "oflk_mosaic_composite_host_u8", "oflk_mosaic_sequence",
           "oflk_mosaic_sequence_u8"]


def test_the_library_exports_the_entry_points():
    import _oflk

    L = _oflk.lib()
    for name in SYMBOLS:
        assert name in _oflk.SIGNATURES and hasattr(L, name), name


def test_the_state_covers_what_it_represents():
    import _oflk

    for Hc, Wc in [(1, 1), (1, 5), (17, 63), (16, 64), (1080, 4993)]:
        got = _oflk.mosaic_state_bytes(Hc, Wc)
        assert got >= Hc * Wc * 20 and got % 256 == 0 and got <= Hc * (Wc + 3) * 20 + 3 * 256
    for Hc, Wc in [(0, 4), (4, 0), (-1, -1), (1 << 15, 1 << 15)]:
        assert _oflk.mosaic_state_bytes(Hc, Wc) == 0


def test_the_canvas_is_the_statement_s():
    import _oflk

    rng = np.random.default_rng(2)
    for _ in range(50):
        T = int(rng.integers(1, 9))
        lo = rng.uniform(-300, 300, (T, 2))
        box = np.concatenate([lo, lo + rng.uniform(1, 200, (T, 2))], 1)
        if rng.random() < 0.5:
            box = np.round(box)   # integers: floor and ceil on the value itself
        dropped = (rng.random(T) < 0.3).astype(np.uint8)
        dropped[int(rng.integers(T))] = 0
        box[dropped != 0] = np.nan
        assert _oflk.mosaic_canvas(box, dropped) == M.canvas(box, dropped)
    L = _oflk.lib()
    v = [ctypes.c_int() for _ in range(4)]
    refs = [ctypes.byref(c) for c in v]
    one = np.array([[0.0, 0.0, 4.0, 4.0]])
    bp, flag = one.ctypes.data_as(_oflk._f64p), np.zeros(1, np.uint8)
    assert L.oflk_mosaic_canvas(bp, flag.ctypes.data, 1, *refs) == 0
    assert L.oflk_mosaic_canvas(bp, flag.ctypes.data, 0, *refs) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_mosaic_canvas(None, flag.ctypes.data, 1, *refs) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_mosaic_canvas(bp, None, 1, *refs) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_mosaic_canvas(bp, flag.ctypes.data, 1, None, *refs[1:]) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_mosaic_canvas(bp, np.ones(1, np.uint8).ctypes.data, 1, *refs) == _oflk.OFLK_ERR_INVALID   # every frame dropped
    nan = np.array([[0.0, np.nan, 4.0, 4.0]])
    assert L.oflk_mosaic_canvas(nan.ctypes.data_as(_oflk._f64p), flag.ctypes.data, 1, *refs) == _oflk.OFLK_ERR_INVALID
    far = np.array([[0.0, 0.0, 2.0 ** 31, 4.0]])
    assert L.oflk_mosaic_canvas(far.ctypes.data_as(_oflk._f64p), flag.ctypes.data, 1, *refs) == _oflk.OFLK_ERR_UNSUPPORTED


def test_refusals_come_before_any_device_call():
    """every refusal is decided on the host: this runs without a GPU, with pointers that are never dereferenced"""
    import _oflk

    L = _oflk.lib()
    P, WS = 0x10000, 0x20000   # 8-byte and 256-byte aligned addresses, never read
    big = 1 << 40
    INVALID, UNSUPPORTED = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED

    def chain(model=P, counts=None, T=3, anchor=0, H=8, W=8, extent=64.0, fr=P, to=P, box=P, held=None, dropped=P):
        return L.oflk_mosaic_chain(model, counts, T, anchor, H, W, extent, fr, to, box, held, dropped, None)

    for kw in [dict(T=0), dict(anchor=-1), dict(anchor=3), dict(H=1), dict(W=1), dict(extent=0.0), dict(extent=-1.0),
               dict(extent=float("nan")), dict(extent=float("inf")), dict(model=None), dict(fr=None), dict(to=None), dict(box=None),
               dict(dropped=None), dict(fr=P + 4), dict(to=P + 4), dict(box=P + 4), dict(T=1, anchor=1, model=None)]:
        assert chain(**kw) == INVALID, kw
        assert L.oflk_last_error()

    need = _oflk.mosaic_state_bytes(20, 30)

    def acc(frames=P, u8=0, F=2, H=8, W=8, maps=P, skip=None, x0=0, y0=0, Hc=20, Wc=30, blend=0, state=WS, nbytes=big):
        return L.oflk_mosaic_accumulate(frames, u8, F, H, W, maps, skip, x0, y0, Hc, Wc, blend, state, nbytes, None)

    for kw in [dict(F=0), dict(H=1), dict(W=1), dict(Hc=0), dict(Wc=0), dict(blend=-1), dict(blend=4), dict(frames=None), dict(maps=None),
               dict(state=None), dict(maps=P + 4), dict(frames=P + 2), dict(state=WS + 128), dict(nbytes=need - 1), dict(nbytes=0)]:
        assert acc(**kw) == INVALID, kw
    assert acc(H=1 << 15, W=1 << 15) == UNSUPPORTED and acc(Hc=1 << 15, Wc=1 << 15) == UNSUPPORTED
    assert acc(Hc=1 << 15, Wc=1 << 15, u8=1, frames=P + 1) == UNSUPPORTED

    def res(state=WS, Hc=20, Wc=30, u8=0, out=P, count=None):
        return L.oflk_mosaic_resolve(state, Hc, Wc, u8, out, count, None)

    for kw in [dict(Hc=0), dict(Wc=-3), dict(state=None), dict(out=None), dict(state=WS + 64), dict(out=P + 2), dict(count=P + 2)]:
        assert res(**kw) == INVALID, kw
    assert res(Hc=1 << 15, Wc=1 << 15) == UNSUPPORTED

    fr, m = np.zeros((1, 4, 4), np.float32), np.zeros((1, 9))
    out = np.zeros((4, 4), np.float32)
    mp = m.ctypes.data_as(_oflk._f64p)
    for fn, a, o in ((L.oflk_mosaic_composite_host, _oflk.ptr(fr), _oflk.ptr(out)),
                     (L.oflk_mosaic_composite_host_u8, fr.ctypes.data, out.ctypes.data)):
        for args in [(None, 1, 4, 4, mp, None, 0, 0, 4, 4, 0, o, None), (a, 0, 4, 4, mp, None, 0, 0, 4, 4, 0, o, None),
                     (a, 1, 1, 4, mp, None, 0, 0, 4, 4, 0, o, None), (a, 1, 4, 1, mp, None, 0, 0, 4, 4, 0, o, None),
                     (a, 1, 4, 4, None, None, 0, 0, 4, 4, 0, o, None), (a, 1, 4, 4, mp, None, 0, 0, 0, 4, 0, o, None),
                     (a, 1, 4, 4, mp, None, 0, 0, 4, 0, 0, o, None), (a, 1, 4, 4, mp, None, 0, 0, 4, 4, 7, o, None),
                     (a, 1, 4, 4, mp, None, 0, 0, 4, 4, 0, None, None)]:
            assert fn(*args) == INVALID, args
        assert fn(a, 1, 1 << 15, 1 << 15, mp, None, 0, 0, 4, 4, 0, o, None) == UNSUPPORTED
        assert fn(a, 1, 4, 4, mp, None, 0, 0, 1 << 15, 1 << 15, 0, o, None) == UNSUPPORTED

    model, counts = np.zeros((2, 9), np.float32), np.zeros((2, 3), np.int32)
    f9, box = np.zeros((3, 9)), np.zeros((3, 4))
    drop = np.zeros(3, np.uint8)

    def chost(model=model, T=3, anchor=0, H=8, W=8, extent=64.0, fr=f9, box=box, drop=drop):
        return L.oflk_mosaic_chain_host(None if model is None else _oflk.ptr(model), counts.ctypes.data_as(_oflk._i32p), T, anchor, H, W,
                                        extent, None if fr is None else fr.ctypes.data_as(_oflk._f64p), f9.ctypes.data_as(_oflk._f64p),
                                        None if box is None else box.ctypes.data_as(_oflk._f64p), None,
                                        None if drop is None else drop.ctypes.data)

    for kw in [dict(T=0), dict(anchor=3), dict(anchor=-1), dict(H=1), dict(W=0), dict(extent=0.0), dict(extent=float("inf")),
               dict(model=None), dict(fr=None), dict(box=None), dict(drop=None)]:
        assert chost(**kw) == INVALID, kw

    frames = np.zeros((3, 32, 32), np.float32)
    canvas = np.zeros(4, np.int32)

    def seq(fn=L.oflk_mosaic_sequence, frames=frames, T=3, H=32, W=32, levels=2, win=5, iters=3, alpha=0.01, beta=0.5, res_=4.0, q=0.01,
            md=4.0, K=50, every=4, hyps=16, thr=1.0, anchor=0, extent=256.0, blend=1, out=out, cap=16, canvas=canvas):
        u8 = fn is L.oflk_mosaic_sequence_u8
        fp = None if frames is None else (frames.ctypes.data if u8 else _oflk.ptr(frames))
        op = None if out is None else (out.ctypes.data if u8 else _oflk.ptr(out))
        return fn(fp, T, H, W, levels, win, iters, alpha, beta, res_, q, md, K, every, hyps, thr, 0, anchor, extent, blend, op, cap,
                  None if canvas is None else canvas.ctypes.data_as(_oflk._i32p), None, None, None, None, None, None)

    for fn in (L.oflk_mosaic_sequence, L.oflk_mosaic_sequence_u8):
        for kw in [dict(T=1), dict(frames=None), dict(out=None), dict(canvas=None), dict(H=1), dict(W=1), dict(anchor=3), dict(anchor=-1),
                   dict(extent=0.0), dict(extent=float("nan")), dict(blend=4), dict(blend=-1), dict(hyps=0), dict(thr=0.0), dict(every=0),
                   dict(K=0), dict(q=-1.0), dict(alpha=-1.0), dict(res_=float("nan")), dict(levels=0), dict(iters=0)]:
            assert seq(fn=fn, **kw) == INVALID, kw
        assert seq(fn=fn, H=1 << 15, W=1 << 15) == UNSUPPORTED


def test_python_arguments_are_checked_before_the_library_is_asked():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    model = np.tile(np.eye(3, dtype=np.float32), (3, 1, 1))
    for kw in [dict(shape=(8,)), dict(shape=(1, 8)), dict(shape=(8, 1)), dict(anchor=4), dict(anchor=-1), dict(anchor=1.5), dict(anchor=True),
               dict(extent=0), dict(extent=float("nan")), dict(extent=float("inf")), dict(status=np.ones(2)),
               dict(model=np.zeros((3, 2, 3), np.float32)), dict(model=np.zeros((3, 6), np.float32))]:
        args = dict(model=model, status=None, shape=(8, 8))
        args.update(kw)
        with pytest.raises(ValueError):
            K.mosaic_chain(**args)
    fr = np.zeros((2, 6, 7), np.float32)
    maps = np.tile(np.eye(3), (2, 1, 1))
    for kw in [dict(maps=np.eye(3)), dict(maps=np.zeros((2, 6))), dict(maps=np.zeros((2, 2, 3))), dict(canvas_shape=(0, 4)), dict(canvas_shape=(4,)),
               dict(canvas_shape=(1 << 15, 1 << 15)), dict(origin=(0,)), dict(origin=(0.5, 0)), dict(origin=(2 ** 31, 0)), dict(skip=np.zeros(3)),
               dict(blend="median"), dict(blend=0), dict(frames=fr[:, :1]), dict(frames=fr[:, :, :1]), dict(frames=np.zeros((2, 2, 6, 7)))]:
        args = dict(frames=fr, maps=maps, canvas_shape=(6, 7))
        args.update(kw)
        with pytest.raises(ValueError):
            K.mosaic_composite(**args)
    seq = np.zeros((3, 32, 32), np.uint8)
    for kw in [dict(anchor=3), dict(anchor=-1), dict(anchor=0.5), dict(blend="max"), dict(extent=0), dict(max_pixels=0), dict(max_pixels=2.5),
               dict(hypotheses=0), dict(threshold=0), dict(seed=-1), dict(detect_every=0), dict(max_corners=0), dict(frames=seq[:1]),
               dict(frames=seq[:, :1]), dict(num_levels=0)]:
        args = dict(frames=seq)
        args.update(kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_mosaic(**args)
    assert P.mosaic_chain is K.mosaic_chain and P.mosaic_composite is K.mosaic_composite and P.MosaicChain is K.MosaicChain
    assert P.Mosaic._fields == ("canvas", "count", "origin", "to_anchor", "held", "dropped", "model", "status")
    assert K.MosaicChain._fields == ("from_anchor", "to_anchor", "box", "held", "dropped", "origin", "canvas_shape")
