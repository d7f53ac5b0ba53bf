"""CPU tests of temporal denoising: what the statement of tests/denoise_model.py means on scenes with a known answer (the
quality scenes' flows are the CPU oracle's, on the noisy frames), and the refusals and the marshalling of the C ABI and of
the Python tier, all made before any device call.  The kernel is held to the statement in tests/test_gpu_denoise.py."""
import numpy as np
import pytest

import denoise_model as M
import flow_median_model as FMM
import interp_model as IM
from test_python_marshalling_cpu import StubLib, recorded


def _zero_flows(T, H, W):
    return [np.zeros((T - 1, H, W), np.float32) for _ in range(4)]


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_static_frames_come_back_and_every_neighbour_counts(R):
    rng = np.random.default_rng(0)
    T, H, W = 7, 9, 11
    still = np.rint(rng.random((H, W)) * 255)
    for dtype in (np.float32, np.uint8):
        frames = np.repeat(still[None], T, axis=0).astype(dtype)
        out, count = M.denoise(frames, *_zero_flows(T, H, W), strength=30.0, radius=R)
        assert out.dtype == dtype and np.array_equal(out, frames)
        for t in range(T):
            assert (count[t] == min(R, t) + min(R, T - 1 - t)).all()


@pytest.mark.parametrize("d", [1, 3, -2])
def test_whole_pixel_pan_with_planted_flows_is_exact(d):
    """frame t is frame 0 moved by t d px along x, F = (d, 0), G = (-d, 0): every chain steps on whole pixels that show the
    pixel's own value, so R |d| px away from the border every frame comes back exactly and every neighbour counts"""
    rng = np.random.default_rng(1)
    T, H, W, R = 6, 12, 48, 2
    base = np.rint(rng.random((H, W)) * 255)
    m = R * abs(d)
    F = np.full((T - 1, H, W), d, np.float32)
    z = np.zeros_like(F)
    for dtype in (np.float32, np.uint8):
        frames = np.stack([np.roll(base, t * d, axis=1) for t in range(T)]).astype(dtype)
        out, count = M.denoise(frames, F, z, -F, z, strength=30.0, radius=R)
        assert np.array_equal(out[:, :, m:W - m], frames[:, :, m:W - m])
        for t in range(T):
            assert (count[t, :, m:W - m] == min(R, t) + min(R, T - 1 - t)).all()
        # at the border a chain leaves the frame and ends there
        edge = count[R, :, W - abs(d):] if d > 0 else count[R, :, :abs(d)]
        assert (edge < 2 * R).all()


def test_a_neighbour_at_exactly_the_strength_is_not_counted():
    H, W, s = 4, 5, 30.0
    for dtype in (np.float32, np.uint8):
        for delta, n in ((s, 0), (-s, 0), (s - 1, 1), (1 - s, 1), (s + 1, 0)):
            frames = np.stack([np.full((H, W), 100.0), np.full((H, W), 100.0 + delta)]).astype(dtype)
            out, count = M.denoise(frames, *_zero_flows(2, H, W), strength=s, radius=1)
            assert (count == n).all(), (delta, n)
            if n == 0:
                assert np.array_equal(out, frames)
            else:
                assert (np.abs(out.astype(np.float64) - frames) > 0).all()   # the neighbour pulled the value


def test_non_finite_neighbours_are_skipped_and_a_nan_centre_comes_out_as_it_is():
    T, H, W = 3, 8, 9
    frames = np.full((T, H, W), 50.0, np.float32)
    frames[2] = 56.0
    frames[0, 2, 2], frames[0, 5, 6], frames[2, 5, 2] = np.nan, np.inf, -np.inf
    frames[1, 1, 7] = np.nan
    frames[1, 6, 4] = np.inf
    out, count = M.denoise(frames, *_zero_flows(T, H, W), strength=30.0, radius=1)
    w = np.float32(1) - np.float32(36) / np.float32(900)
    only_next = (np.float32(50) + w * np.float32(56)) / (np.float32(1) + w)   # frame 0's value is skipped
    for y, x in ((2, 2), (5, 6)):
        assert count[1, y, x] == 1 and out[1, y, x] == only_next
    assert count[1, 5, 2] == 1 and out[1, 5, 2] == np.float32(50)                 # frame 2's value is skipped
    assert count[1, 0, 0] == 2
    assert np.isnan(out[1, 1, 7]) and out[1, 1, 7].view(np.uint32) == frames[1, 1, 7].view(np.uint32) and count[1, 1, 7] == 0
    assert out[1, 6, 4] == np.inf and count[1, 6, 4] == 0
    # as neighbours of frames 0 and 2 the non-finite centres are skipped too
    assert count[0, 1, 7] == 0 and out[0, 1, 7] == 50.0 and count[2, 6, 4] == 0 and out[2, 6, 4] == 56.0


# ---- quality: the oracle's flows on the noisy frames ---------------------------------------------------------------------
def _denoised(oracle, clean):
    """(noisy frames, the statement's result at the defaults of the Python tier: median 9, beta 4.0, R = 2, strength 3 sigma)"""
    noisy = M.noisy(clean)
    flows = [FMM.median(f, 9) for f in IM.oracle_flows(oracle, noisy)]
    out, _ = M.denoise(noisy, *flows, strength=3 * M.SIGMA, radius=2, alpha=0.01, beta=4.0)
    return noisy, out


@pytest.mark.parametrize("pan", [(0, 0), (3, 1)], ids=str)
def test_pan_scenes_come_out_cleaner_than_they_went_in(oracle, pan):
    """denoise_model.pan_sequence (7 frames of 96 x 128 under a pan, Gaussian noise of sigma 10), the oracle's flows of the
    noisy frames at 3 levels, window 5, 3 iterations through the 9 x 9 median: the mean squared error against the clean
    frames, 12 px inside the border and relative to the noisy input's, is below 1, and on the moving scene also below that of
    the average of five frames where they lie.  Measured (statement / average in place): pan (0, 0): 0.307 / 0.255;
    pan (3, 1): 0.339 / 0.978 (all 7 frames count: one at an end of the sequence has fewer than four neighbours)."""
    clean = M.pan_sequence(*pan)
    noisy, out = _denoised(oracle, clean)
    err = M.relative_error(out, clean, noisy)
    avg = M.relative_error(M.average_in_place(noisy), clean, noisy)
    print(f"pan {pan}: statement {err:.3f}, average in place {avg:.3f} of the input's error")
    assert err < 1.0
    if pan != (0, 0):
        assert err < avg


def test_a_crossing_rectangle_is_not_smeared(oracle):
    """denoise_model.mover_sequence: a rectangle crossing a static background at 9 px a frame.  Both in the region the
    rectangle touches and in the background the error is below the input's.  Measured (statement / average in place):
    touched 0.512 / 6.206, background 0.367 / 0.255."""
    clean, touched = M.mover_sequence()
    noisy, out = _denoised(oracle, clean)
    avg = M.average_in_place(noisy)
    for name, mask in (("touched", touched), ("background", ~touched)):
        err, a = M.relative_error(out, clean, noisy, mask), M.relative_error(avg, clean, noisy, mask)
        print(f"mover, {name}: statement {err:.3f}, average in place {a:.3f} of the input's error")
        assert err < 1.0, name


# ---- refusals ------------------------------------------------------------------------------------------------------------
T, H, W = 3, 6, 8
FRAMES = {"f32": np.zeros((T, H, W), np.float32), "u8": np.zeros((T, H, W), np.uint8)}
FLOWS = [np.zeros((T - 1, H, W), np.float32) for _ in range(4)]

BAD = [
    (dict(radius=0), "radius must be an integer in [1, 4]"),
    (dict(radius=5), "radius must be an integer in [1, 4]"),
    (dict(radius=1.5), "radius must be an integer in [1, 4]"),
    (dict(radius=True), "radius must be an integer in [1, 4]"),
    (dict(strength=0.0), "strength must be finite and > 0"),
    (dict(strength=-3.0), "strength must be finite and > 0"),
    (dict(strength=np.nan), "strength must be finite and > 0"),
    (dict(strength=np.inf), "strength must be finite and > 0"),
    (dict(strength=1e39), "strength must be finite and > 0"),
    (dict(alpha=-1.0), "alpha and beta must be finite and >= 0"),
    (dict(beta=np.inf), "alpha and beta must be finite and >= 0"),
    (dict(beta=np.nan), "alpha and beta must be finite and >= 0"),
]


@pytest.mark.parametrize("px", ["f32", "u8"])
@pytest.mark.parametrize("kw,msg", BAD, ids=[str(sorted(k.items())) for k, _ in BAD])
def test_python_refusals_need_no_device(monkeypatch, px, kw, msg):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    kw = {"strength": 30.0, **kw}
    with pytest.raises(ValueError) as e:
        P.denoise_frames(FRAMES[px], *FLOWS, **kw)
    assert msg in str(e.value)
    with pytest.raises(ValueError) as e:
        P.lucas_kanade_pyramidal_sequence_denoise(FRAMES[px], **kw)
    assert msg in str(e.value)
    assert stub.calls == []


def test_python_refuses_a_bad_median_and_frames_and_flows_that_do_not_fit(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    for k in (1, 4, 11, 5.0, True):
        with pytest.raises(ValueError, match="flow_median must be 0, 3, 5, 7 or 9"):
            P.lucas_kanade_pyramidal_sequence_denoise(FRAMES["u8"], 30.0, flow_median=k)
    with pytest.raises(ValueError, match="at least 2 frames"):
        P.lucas_kanade_pyramidal_sequence_denoise(FRAMES["u8"][:1], 30.0)
    with pytest.raises(ValueError, match="at least 2 frames"):
        P.denoise_frames(FRAMES["u8"][:1], *[f[:0] for f in FLOWS], 30.0)
    with pytest.raises(ValueError, match="every flow must have shape"):
        P.denoise_frames(FRAMES["f32"], FLOWS[0], FLOWS[1], FLOWS[2], FLOWS[3][:1], 30.0)
    with pytest.raises(ValueError, match="expected a"):
        P.denoise_frames(np.zeros((T, H, W, 3), np.uint8), *FLOWS, 30.0)   # packed colour is not in scope
    assert stub.calls == []


def test_python_marshals_the_settings_in_the_c_order(monkeypatch):
    import lucas_kanade_pyramidal as P

    a = float(np.float32(0.01))
    assert recorded(monkeypatch, lambda: P.lucas_kanade_pyramidal_sequence_denoise(FRAMES["u8"], 30.0)) == [
        f"oflk_denoise_sequence_u8(ptr, {T}, {H}, {W}, 3, 5, 3, {a!r}, 4.0, 9, 2, 30.0, ptr, NULL)"]
    assert recorded(monkeypatch, lambda: P.lucas_kanade_pyramidal_sequence_denoise(
        FRAMES["f32"], 7.5, radius=4, alpha=0.25, beta=0.5, flow_median=0, num_levels=2, window_size=7, num_iterations=1,
        return_count=True)) == [f"oflk_denoise_sequence(ptr, {T}, {H}, {W}, 2, 7, 1, 0.25, 0.5, 0, 4, 7.5, ptr, ptr)"]
    assert recorded(monkeypatch, lambda: P.denoise_frames(FRAMES["f32"], *FLOWS, 30.0)) == [
        f"oflk_denoise_frames_host(ptr, {T - 1}, {H}, {W}, ptr, ptr, ptr, ptr, {a!r}, 4.0, 2, 30.0, ptr, NULL)"]
    assert recorded(monkeypatch, lambda: P.denoise_frames(FRAMES["u8"], *FLOWS, strength=12.0, radius=1, alpha=0.0, beta=1.0,
                                                          return_count=True)) == [
        f"oflk_denoise_frames_host_u8(ptr, {T - 1}, {H}, {W}, ptr, ptr, ptr, ptr, 0.0, 1.0, 1, 12.0, ptr, ptr)"]


def test_python_returns_the_frames_shape_and_type(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    monkeypatch.setattr(_oflk, "_lib", StubLib())
    for px, dtype in (("f32", np.float32), ("u8", np.uint8)):
        out = P.lucas_kanade_pyramidal_sequence_denoise(FRAMES[px], 30.0)
        assert out.shape == (T, H, W) and out.dtype == dtype
        out, count = P.denoise_frames(list(FRAMES[px]), *FLOWS, 30.0, return_count=True)
        assert out.shape == count.shape == (T, H, W) and out.dtype == dtype and count.dtype == np.uint8


def _c_calls():
    """every C entry point of the feature as call(**overrides) -> return code, on valid small arguments"""
    import _oflk

    L = _oflk.lib()

    def make(name, u8, seq):
        def call(**kw):
            a = dict(frames=FRAMES["u8" if u8 else "f32"], T=T, H=H, W=W, levels=2, window=5, iters=2, alpha=0.01, beta=4.0,
                     flow_median=0, radius=2, strength=30.0, flows=FLOWS, count=np.zeros((T, H, W), np.uint8))
            a["out"] = np.zeros((T, H, W), a["frames"].dtype)
            a.update(kw)
            p = lambda x: None if x is None else (_oflk.pix(x) if x.dtype != np.uint8 else x.ctypes.data)
            if seq:
                return getattr(L, name)(p(a["frames"]), a["T"], a["H"], a["W"], a["levels"], a["window"], a["iters"], a["alpha"],
                                        a["beta"], a["flow_median"], a["radius"], a["strength"], p(a["out"]), p(a["count"]))
            fl = [None if f is None else _oflk.ptr(f) for f in a["flows"]]
            return getattr(L, name)(p(a["frames"]), a["T"] - 1, a["H"], a["W"], *fl, a["alpha"], a["beta"], a["radius"], a["strength"],
                                    p(a["out"]), p(a["count"]))
        return call

    return {"sequence": make("oflk_denoise_sequence", False, True), "sequence_u8": make("oflk_denoise_sequence_u8", True, True),
            "host": make("oflk_denoise_frames_host", False, False), "host_u8": make("oflk_denoise_frames_host_u8", True, False)}


C_BAD = [
    ("radius 0", dict(radius=0)), ("radius 5", dict(radius=5)), ("radius -1", dict(radius=-1)),
    ("strength 0", dict(strength=0.0)), ("strength < 0", dict(strength=-30.0)), ("strength NaN", dict(strength=float("nan"))),
    ("strength inf", dict(strength=float("inf"))), ("alpha < 0", dict(alpha=-0.5)), ("alpha inf", dict(alpha=float("inf"))),
    ("beta < 0", dict(beta=-1.0)), ("beta NaN", dict(beta=float("nan"))), ("NULL out", dict(out=None)),
    ("NULL frames", dict(frames=None)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)),
]


@pytest.mark.parametrize("what,kw", C_BAD, ids=[w for w, _ in C_BAD])
def test_c_refusals_come_before_any_device_call(what, kw):
    """OFLK_ERR_INVALID with or without a device: a call that reached the device would answer OFLK_ERR_NO_DEVICE here, or run"""
    import _oflk

    for name, call in _c_calls().items():
        assert call(**kw) == _oflk.OFLK_ERR_INVALID, (name, what, _oflk.lib().oflk_last_error())


def test_c_refusals_of_single_forms():
    import _oflk

    calls = _c_calls()
    inv = _oflk.OFLK_ERR_INVALID
    for name in ("sequence", "sequence_u8"):   # what oflk_pyramidal_sequence_fb_median refuses, with its codes
        assert calls[name](T=1) == inv
        assert calls[name](levels=0) == inv
        for k in (1, 4, 11, -3):
            assert calls[name](flow_median=k) == inv
        assert calls[name](H=1 << 23) == _oflk.OFLK_ERR_UNSUPPORTED
        assert calls[name](H=1 << 15, W=1 << 15) == _oflk.OFLK_ERR_UNSUPPORTED
    for name in ("host", "host_u8"):
        assert calls[name](T=1) == inv   # B = 0
        assert calls[name](H=1 << 23) == _oflk.OFLK_ERR_UNSUPPORTED
        for i in range(4):
            assert calls[name](flows=[None if k == i else f for k, f in enumerate(FLOWS)]) == inv, (name, i)
    # an output that overlaps the frames: its first byte on the frames' last byte, and its last on their first
    for name, call in calls.items():
        fr = FRAMES["u8" if name.endswith("u8") else "f32"]
        buf = np.zeros(fr.size * 2, fr.dtype)
        assert call(frames=buf[:fr.size].reshape(fr.shape), out=buf[fr.size - 1:]) == inv, name
        assert call(frames=buf[fr.size - 1:2 * fr.size - 1].reshape(fr.shape), out=buf) == inv, name
        assert call(frames=buf[:fr.size].reshape(fr.shape), out=buf[:fr.size]) == inv, name


def test_a_valid_call_gets_past_the_refusals():
    """the arguments the refusal tests vary are valid as they stand: the call answers OFLK_ERR_NO_DEVICE without a device and
    runs with one"""
    import _oflk

    want = _oflk.OFLK_OK if _oflk.device_count() > 0 else _oflk.OFLK_ERR_NO_DEVICE
    for name, call in _c_calls().items():
        assert call() == want, (name, _oflk.lib().oflk_last_error())
