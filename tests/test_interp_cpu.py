"""CPU tests of frame interpolation: what the statement of tests/interp_model.py means on scenes with a known answer (the
flows are the CPU oracle's), and the refusals of the C ABI and of the Python tier, all made before any device call.  The
kernel is held to the statement in tests/test_gpu_interp.py."""
import numpy as np
import pytest

import fb_model as FM
import interp_model as M
from test_python_marshalling_cpu import StubLib, recorded


def test_zero_flows_give_the_cross_fade_and_status_3():
    rng = np.random.default_rng(0)
    H, W = 13, 17
    z = np.zeros((H, W), np.float32)
    for dtype in (np.float32, np.uint8):
        A, B = (rng.random((2, H, W)) * 255).astype(dtype)
        for tau in (0.5, 1 / 3, 0.25, 2.0 ** -20, 1 - 2.0 ** -20):
            out, status = M.interpolate_pair(A, B, z, z, z, z, tau)
            want = M.cross_fade(A, B, tau)
            want = np.rint(want).astype(np.uint8) if dtype == np.uint8 else want
            assert out.dtype == dtype and np.array_equal(out.view(np.uint8), want.view(np.uint8))
            assert (status == 3).all()


@pytest.mark.parametrize("d", [1, 3, -2])
def test_whole_pixel_shift_with_planted_flows_is_exact(d):
    """B is A moved by 2d px along x, F = (2d, 0), G = (-2d, 0), tau = 0.5: both sides solve to whole pixels and sample the
    same value, so away from the border the result is A moved by d, exactly"""
    rng = np.random.default_rng(1)
    H, W = 20, 40
    A = (rng.random((H, W)) * 255).astype(np.float32)
    B = np.roll(A, 2 * d, axis=1)
    mid = np.roll(A, d, axis=1)
    F = np.full((H, W), 2 * d, np.float32)
    z = np.zeros((H, W), np.float32)
    m = 2 * abs(d)
    for frames in ((A, B), (np.rint(A).astype(np.uint8), np.rint(B).astype(np.uint8))):
        for refine in (1, 2, 4):
            out, status = M.interpolate_pair(*frames, F, z, -F, z, 0.5, refine=refine)
            want = np.rint(mid).astype(np.uint8) if out.dtype == np.uint8 else mid
            assert np.array_equal(out[:, m:W - m], want[:, m:W - m])
            assert (status[:, m:W - m] == 3).all()
            assert (status[:, :abs(d)] != 3).all() and (status[:, W - abs(d):] != 3).all()   # a side leaves the frame


PANS = [(3, 1), (6, -2)]


@pytest.mark.parametrize("pan", PANS, ids=str)
def test_pan_scenes_beat_the_cross_fade(oracle, pan):
    """interp_model.pan_scene (96 x 128, a multi-octave texture under a pan, the true middle frame known), the oracle's flows
    at 3 levels, window 5, 3 iterations, tau = 0.5: the mean absolute error 12 px inside the border is smaller than the
    cross-fade's, which is what a caller has without the feature.  Measured (grey levels, statement / cross-fade):
    pan (3, 1): 0.71 / 2.11, a ratio of 0.34; pan (6, -2): 1.98 / 5.43, a ratio of 0.37."""
    A, mid, B = M.pan_scene(*pan)
    uf, vf, ub, vb = M.oracle_flows(oracle, np.stack([A, B]))
    out, status = M.interpolate_pair(A, B, uf[0], vf[0], ub[0], vb[0], 0.5)
    inner = (slice(12, -12), slice(12, -12))
    err = np.abs(out - mid)[inner].mean()
    fade = np.abs(M.cross_fade(A, B, 0.5) - mid)[inner].mean()
    print(f"pan {pan}: statement {err:.2f}, cross-fade {fade:.2f}, ratio {err / fade:.3f}")
    assert err < fade
    assert (status[inner] == 3).mean() > 0.5


def test_occluder_scene_reaches_every_blend_branch(oracle):
    frames, _ = FM.occluder_scene(T=3)
    flows = M.oracle_flows(oracle, frames)
    new, status = M.interpolate(frames, *flows, [0.5], refine=2)
    counts = np.bincount(status.ravel(), minlength=4)
    print("status counts of codes 0 .. 3:", counts.tolist())
    assert len(counts) == 4 and (counts > 0).all()
    assert counts[3] > 0.7 * status.size
    assert np.bincount(status[0].ravel(), minlength=4).tolist() == [1349, 237, 249, 10453]   # pair 0, as the prototype counted
    assert np.isfinite(new).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------
T, H, W = 3, 6, 8
FRAMES = {"f32": np.zeros((T, H, W), np.float32), "u8": np.zeros((T, H, W), np.uint8)}
FLOWS = [np.zeros((T - 1, H, W), np.float32) for _ in range(4)]

BAD = [
    (dict(taus=[]), "taus must be 1 to 16 values"),
    (dict(taus=[0.5] * 17), "taus must be 1 to 16 values"),
    (dict(taus=[[0.5]]), "taus must be 1 to 16 values"),
    (dict(taus=[0.0]), "every tau must be finite and strictly between 0 and 1"),
    (dict(taus=[0.5, 1.0]), "every tau must be finite and strictly between 0 and 1"),
    (dict(taus=[np.nan]), "every tau must be finite and strictly between 0 and 1"),
    (dict(taus=[-0.25]), "every tau must be finite and strictly between 0 and 1"),
    (dict(refine=0), "refine must be an integer in [1, 8]"),
    (dict(refine=9), "refine must be an integer in [1, 8]"),
    (dict(refine=1.5), "refine must be an integer in [1, 8]"),
    (dict(refine=True), "refine must be an integer in [1, 8]"),
    (dict(alpha=-1.0), "alpha and beta must be finite and >= 0"),
    (dict(beta=np.inf), "alpha and beta must be finite and >= 0"),
]


@pytest.mark.parametrize("px", ["f32", "u8"])
@pytest.mark.parametrize("kw,msg", BAD, ids=[str(sorted(k.items())) for k, _ in BAD])
def test_python_refusals_need_no_device(monkeypatch, px, kw, msg):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    with pytest.raises(ValueError) as e:
        P.interpolate_frames(FRAMES[px], *FLOWS, **kw)
    assert msg in str(e.value)
    with pytest.raises(ValueError) as e:
        P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES[px], **kw)
    assert msg in str(e.value)
    assert stub.calls == []


@pytest.mark.parametrize("factor", [1, 0, 18, 2.5, True])
def test_python_refuses_a_bad_factor(monkeypatch, factor):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    with pytest.raises(ValueError, match="factor must be an integer"):
        P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["u8"], factor=factor)
    assert stub.calls == []


def test_python_refuses_frames_and_flows_that_do_not_fit(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    with pytest.raises(ValueError, match="at least 2 frames"):
        P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["u8"][:1])
    with pytest.raises(ValueError, match="every flow must have shape"):
        P.interpolate_frames(FRAMES["f32"], FLOWS[0], FLOWS[1], FLOWS[2], FLOWS[3][:1])
    assert stub.calls == []


def test_python_marshals_factor_and_taus(monkeypatch):
    """factor = k stands for j / k formed in float64; explicit taus override it; the settings go down in the C order"""
    import _oflk
    import lucas_kanade_pyramidal as P

    seen = {}

    class Lib(StubLib):
        def __getattr__(self, name):
            fn = StubLib.__getattr__(self, name)

            def call(*args):
                if name.startswith("oflk_interpolate_sequence"):
                    seen[name] = (args[1:10], [args[10][j] for j in range(args[11])])
                return fn(*args)
            return call

    monkeypatch.setattr(_oflk, "_lib", Lib())
    r = P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["u8"], factor=4, num_levels=2, window_size=7, num_iterations=1, refine=3)
    assert seen["oflk_interpolate_sequence_u8"] == ((T, H, W, 2, 7, 1, float(np.float32(0.01)), 0.5, 3), [0.25, 0.5, 0.75])
    assert r.frames.shape == ((T - 1) * 3 + T, H, W) and r.frames.dtype == np.uint8
    assert r.new.shape == r.status.shape == (T - 1, 3, H, W) and r.status.dtype == np.uint8
    P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["f32"], factor=3)
    assert seen["oflk_interpolate_sequence"][1] == [np.float64(1) / np.float64(3), np.float64(2) / np.float64(3)]
    P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["f32"], factor=7, taus=[0.1])
    assert seen["oflk_interpolate_sequence"][1] == [0.1]
    assert recorded(monkeypatch, lambda: P.interpolate_frames(FRAMES["f32"], *FLOWS)) == [
        f"oflk_interpolate_frames_host(ptr, 2, {H}, {W}, ptr, ptr, ptr, ptr, {float(np.float32(0.01))!r}, 0.5, 2, ptr, 1, ptr, NULL)"]
    assert recorded(monkeypatch, lambda: P.interpolate_frames(FRAMES["u8"], *FLOWS, taus=[0.25, 0.5], return_status=True)) == [
        f"oflk_interpolate_frames_host_u8(ptr, 2, {H}, {W}, ptr, ptr, ptr, ptr, {float(np.float32(0.01))!r}, 0.5, 2, ptr, 2, ptr, ptr)"]


def _c_calls():
    """every C entry point of the feature as call(**overrides) -> return code, on valid small arguments"""
    import ctypes

    import _oflk

    L = _oflk.lib()
    f64p = ctypes.POINTER(ctypes.c_double)

    def make(name, u8, seq):
        def call(**kw):
            a = dict(frames=FRAMES["u8" if u8 else "f32"], T=T, H=H, W=W, levels=2, window=5, iters=2, alpha=0.01, beta=0.5,
                     refine=2, taus=np.array([0.5]), n=1, flows=FLOWS, status=np.zeros((T - 1, 4, H, W), np.uint8))
            a["out"] = np.zeros((T - 1, 4, H, W), a["frames"].dtype)
            a.update(kw)
            p = lambda x: None if x is None else (x if isinstance(x, int) else _oflk.pix(x) if x.dtype != np.uint8 else x.ctypes.data)
            taus = None if a["taus"] is None else np.ascontiguousarray(a["taus"], np.float64).ctypes.data_as(f64p)
            cfg = (a["alpha"], a["beta"], a["refine"], taus, a["n"])
            fl = [None if f is None else _oflk.ptr(f) for f in a["flows"]]
            if seq:
                return getattr(L, name)(p(a["frames"]), a["T"], a["H"], a["W"], a["levels"], a["window"], a["iters"], *cfg,
                                        p(a["out"]), p(a["status"]))
            if name == "oflk_interpolate_frames":   # host addresses stand in: every refusal comes before they are used
                fr = a["frames"] if a["frames"] is None else a["frames"].ctypes.data
                out = a["out"] if a["out"] is None else a["out"].ctypes.data
                return L.oflk_interpolate_frames(fr, int(u8), a["T"] - 1, a["H"], a["W"], *(None if f is None else f.ctypes.data for f in a["flows"]),
                                                 *cfg, out, None, None)
            return getattr(L, name)(p(a["frames"]), a["T"] - 1, a["H"], a["W"], *fl, *cfg, p(a["out"]), p(a["status"]))
        return call

    return {"sequence": make("oflk_interpolate_sequence", False, True), "sequence_u8": make("oflk_interpolate_sequence_u8", True, True),
            "host": make("oflk_interpolate_frames_host", False, False), "host_u8": make("oflk_interpolate_frames_host_u8", True, False),
            "device": make("oflk_interpolate_frames", False, False), "device_u8": make("oflk_interpolate_frames", True, False)}


C_BAD = [
    ("n = 0", dict(n=0)), ("n = 17", dict(n=17, taus=np.full(17, 0.5))), ("tau = 0", dict(taus=np.array([0.0]))),
    ("tau = 1", dict(taus=np.array([1.0]))), ("tau NaN", dict(taus=np.array([np.nan]))), ("tau inf", dict(taus=np.array([np.inf]))),
    ("second tau", dict(taus=np.array([0.5, -0.5]), n=2)), ("refine 0", dict(refine=0)), ("refine 9", dict(refine=9)),
    ("NULL taus", dict(taus=None)), ("NULL out", dict(out=None)), ("alpha < 0", dict(alpha=-0.5)), ("beta NaN", dict(beta=float("nan"))),
    ("H = 0", dict(H=0)), ("NULL frames", dict(frames=None)),
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
    for name in ("sequence", "sequence_u8"):   # what oflk_pyramidal_sequence_fb refuses, with its codes
        assert calls[name](T=1) == inv
        assert calls[name](levels=0) == inv
        assert calls[name](H=1 << 23) == _oflk.OFLK_ERR_UNSUPPORTED
    for name in ("host", "host_u8", "device", "device_u8"):
        assert calls[name](T=1) == inv   # B = 0
        for i in range(4):
            assert calls[name](flows=[None if k == i else f for k, f in enumerate(FLOWS)]) == inv, (name, i)
    # an output that overlaps the frames: its first byte on the frames' last byte, and the frames inside the output
    for name, call in calls.items():
        fr = FRAMES["u8" if name.endswith("u8") else "f32"]
        buf = np.zeros(fr.size * 4, fr.dtype)
        inside = buf[fr.size:2 * fr.size].reshape(fr.shape)
        assert call(frames=inside, out=buf, n=4, taus=np.full(4, 0.5)) == inv, name   # 8 planes out, the frames at 3 .. 5
        assert call(frames=buf[:fr.size].reshape(fr.shape), out=buf[fr.size - 1:]) == inv, name
