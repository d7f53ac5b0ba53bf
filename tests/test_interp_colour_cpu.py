"""CPU tests of frame interpolation on colour and NV12 video: what the statement of tests/interp_colour_model.py means on
scenes with a known answer, and the refusals of the six C entry points and of the Python tier, all made before any device
call.  The kernels are held to the statement in tests/test_gpu_interp_colour.py."""
import ctypes
import math

import numpy as np
import pytest

import interp_colour_model as CM
import interp_colour_scenes as CS
import interp_model as M
import nv12_model as NM
from test_python_marshalling_cpu import StubLib, recorded

TAUS = [0.5, 1 / 3, 2.0 ** -20]


def _flows(B, H, W, seed, amp=3.0):
    """finite flows of a few px, roughly consistent, some points leaving the frame at the border"""
    rng = np.random.default_rng(seed)
    f = (rng.random((4, B, H, W)) * 2 - 1) * amp
    f[2:] = -f[:2] + 0.1 * f[2:]
    return [np.ascontiguousarray(a, np.float32) for a in f]


@pytest.mark.parametrize("C", [3, 4])
def test_packed_model_is_the_grey_model_per_channel(C):
    B, H, W = 2, 9, 14
    frames = np.random.default_rng(C).integers(0, 256, (B + 1, H, W, C), dtype=np.uint8)
    flows = _flows(B, H, W, seed=1)
    new, status = CM.interpolate_packed(frames, *flows, TAUS, refine=2)
    assert new.shape == (B, len(TAUS), H, W, C) and new.dtype == np.uint8 and status.shape == (B, len(TAUS), H, W)
    for c in range(C):
        want = M.interpolate(np.ascontiguousarray(frames[..., c]), *flows, TAUS, refine=2)
        assert np.array_equal(new[..., c], want[0]) and np.array_equal(status, want[1])
    assert len(np.unique(status)) > 1


@pytest.mark.parametrize("siting", ["left", "center"])
def test_nv12_model_y_plane_is_the_grey_model_on_the_y_planes(siting):
    B, H, W = 2, 10, 12
    frames = NM.random_frames(B + 1, H, W, seed=2)
    flows = _flows(B, H, W, seed=3)
    new, status = CM.interpolate_nv12(frames, *flows, TAUS, siting)
    assert new.shape == (B, len(TAUS), 3 * H // 2, W) and new.dtype == np.uint8
    want = M.interpolate(np.ascontiguousarray(NM.planes(frames)[0]), *flows, TAUS)
    assert np.array_equal(new[:, :, :H], want[0]) and np.array_equal(status, want[1])


@pytest.mark.parametrize("siting", ["left", "center"])
def test_zero_flows_give_the_chroma_cross_fade_and_status_3(siting):
    """cx = 0.5 ((2 i + sx) - sx) = i exactly, for both sitings: every chroma sample is its own cross-fade"""
    B, H, W = 1, 8, 12
    frames = NM.random_frames(B + 1, H, W, seed=4)
    z = [np.zeros((B, H, W), np.float32)] * 4
    taus = [0.5, 1 / 3, 0.25, 2.0 ** -20, 1 - 2.0 ** -20]
    new, status = CM.interpolate_nv12(frames, *z, taus, siting)
    assert (status == 3).all()
    uv = NM.planes(frames)[1]
    for j, tau in enumerate(taus):
        want = np.rint(M.cross_fade(uv[0], uv[1], tau)).astype(np.uint8)
        assert np.array_equal(NM.planes(new[0, j:j + 1])[1][0], want)
        assert np.array_equal(new[0, j, :H], np.rint(M.cross_fade(frames[0, :H], frames[1, :H], tau)).astype(np.uint8))


@pytest.mark.parametrize("siting", ["left", "center"])
def test_constant_chroma_stays_constant_no_green_at_the_edge(siting):
    """U = 90, V = 200 in both frames under any finite flows: every chroma byte of the output is 90 or 200, its own plane's
    value.  The clamp's test: the same sampling without the clamp reads the cval 0 past the chroma plane's last row and
    column (and, for sy = 0.5, before its first row) and fails"""
    B, H, W = 2, 12, 16
    y = np.random.default_rng(5).integers(0, 256, (B + 1, H, W), dtype=np.uint8)
    uv = np.empty((B + 1, H // 2, W // 2, 2), np.uint8)
    uv[..., 0], uv[..., 1] = 90, 200
    frames = NM.from_planes(y, uv)
    flows = _flows(B, H, W, seed=6, amp=0.9)   # sub-pixel: points stay inside the luma frame but leave the chroma plane
    for k in range(4):
        flows[k][1] *= 6.0   # a pair with larger motion
    new, _ = CM.interpolate_nv12(frames, *flows, TAUS, siting)
    got = NM.planes(new.reshape((-1,) + new.shape[2:]))[1]
    assert (got[..., 0] == 90).all() and (got[..., 1] == 200).all()
    bare, _ = CM.interpolate_nv12(frames, *flows, TAUS, siting, clamped=False)
    bad = NM.planes(bare.reshape((-1,) + bare.shape[2:]))[1]
    assert ((bad[..., 0] != 90) | (bad[..., 1] != 200)).any(), "the scene does not reach past the chroma plane"
    inner = bad[:, 1:-1, 1:-1]
    assert (inner[..., 0] == 90).all() and (inner[..., 1] == 200).all()   # only the plane's border differs


@pytest.mark.parametrize("pan", [(3, 1), (6, -2)], ids=str)
def test_colour_pan_chroma_beats_the_cross_fade(oracle, pan):
    """A colour pan (three interp_model.pan_scene textures as R, G, B, 96 x 128) as NV12 (BT.601, box-averaged chroma, so the
    siting is "center"), the oracle's flows on the Y planes at 3 levels, window 5, 3 iterations, tau = 0.5: on each of U and V
    the mean absolute error against the true middle frame's chroma, 6 chroma px inside the border, is below the cross-fade's.
    Measured (chroma levels, statement / cross-fade): pan (3, 1): U 0.72 / 1.09, ratio 0.66, V 0.71 / 1.08, ratio 0.66;
    pan (6, -2): U 1.29 / 2.58, ratio 0.50, V 1.41 / 2.90, ratio 0.49.  The frames are bytes here (the grey test's are
    float32, ratios 0.34 and 0.37): the flows are tracked on a rounded Y that mixes the three textures, and both errors
    include the rounding of the chroma bytes."""
    A, mid, B = CS.colour_pan(*pan)
    frames, _ = CS.to_nv12(np.stack([A, B]))
    _, (_, mu, mv) = CS.to_nv12(mid[None])
    ys = np.ascontiguousarray(NM.planes(frames)[0], np.float32)
    uf, vf, ub, vb = M.oracle_flows(oracle, ys)
    new, _ = CM.interpolate_nv12(frames, uf, vf, ub, vb, [0.5], "center")
    got = NM.planes(new[0])[1][0].astype(np.float64)
    uv = NM.planes(frames)[1]
    fade = M.cross_fade(uv[0], uv[1], 0.5).astype(np.float64)
    inner = (slice(6, -6), slice(6, -6))
    for c, (name, truth) in enumerate((("U", mu[0]), ("V", mv[0]))):
        err = np.abs(got[..., c] - truth)[inner].mean()
        ref = np.abs(fade[..., c] - truth)[inner].mean()
        print(f"pan {pan} {name}: statement {err:.2f}, cross-fade {ref:.2f}, ratio {err / ref:.3f}")
        assert err < ref


# ---- the Python tier ---------------------------------------------------------------------------------------------------
T, H, W = 3, 6, 8
RGB = np.zeros((T, H, W, 3), np.uint8)
NV12 = np.zeros((T, 3 * H // 2, W), np.uint8)
FLOWS = [np.zeros((T - 1, H, W), np.float32) for _ in range(4)]
A01 = float(np.float32(0.01))


def test_python_marshals_both_layouts(monkeypatch):
    import lucas_kanade_pyramidal as P

    assert recorded(monkeypatch, lambda: P.interpolate_frames(RGB, *FLOWS, taus=[0.25, 0.5], return_status=True)) == [
        f"oflk_interpolate_frames_packed_host(ptr, 2, {H}, {W}, 3, ptr, ptr, ptr, ptr, {A01!r}, 0.5, 2, ptr, 2, ptr, ptr)"]
    assert recorded(monkeypatch, lambda: P.interpolate_frames_nv12(NV12, *FLOWS, siting="center")) == [
        f"oflk_interpolate_frames_nv12_host(ptr, 2, {H}, {W}, 1, ptr, ptr, ptr, ptr, {A01!r}, 0.5, 2, ptr, 1, ptr, NULL)"]
    bgra = np.zeros((T, H, W, 4), np.uint8)
    assert recorded(monkeypatch, lambda: P.lucas_kanade_pyramidal_sequence_interpolate(bgra, factor=3, order="bgr")) == [
        f"oflk_interpolate_sequence_packed(ptr, {T}, {H}, {W}, 4, 1, 3, 5, 3, {A01!r}, 0.5, 2, ptr, 2, ptr, ptr)"]
    assert recorded(monkeypatch, lambda: P.lucas_kanade_pyramidal_sequence_interpolate_nv12(NV12, num_levels=2)) == [
        f"oflk_interpolate_sequence_nv12(ptr, {T}, {H}, {W}, 0, 2, 5, 3, {A01!r}, 0.5, 2, ptr, 1, ptr, ptr)"]


def test_python_result_shapes_without_a_device(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    monkeypatch.setattr(_oflk, "_lib", StubLib())
    r = P.lucas_kanade_pyramidal_sequence_interpolate(RGB, factor=4)
    assert r.frames.shape == ((T - 1) * 3 + T, H, W, 3) and r.new.shape == (T - 1, 3, H, W, 3) and r.status.shape == (T - 1, 3, H, W)
    r = P.lucas_kanade_pyramidal_sequence_interpolate_nv12(NV12, factor=2)
    assert r.frames.shape == ((T - 1) + T, 3 * H // 2, W) and r.new.shape == (T - 1, 1, 3 * H // 2, W)
    assert r.status.shape == (T - 1, 1, H, W) and r.frames.dtype == r.new.dtype == r.status.dtype == np.uint8
    new, st = P.interpolate_frames(RGB, *FLOWS, return_status=True)
    assert new.shape == (T - 1, 1, H, W, 3) and st.shape == (T - 1, 1, H, W)
    assert P.interpolate_frames_nv12(NV12, *FLOWS, taus=[0.2, 0.4]).shape == (T - 1, 2, 3 * H // 2, W)


def test_python_refusals_need_no_device(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    f32 = RGB.astype(np.float32)
    for call in (lambda: P.interpolate_frames(f32, *FLOWS), lambda: P.lucas_kanade_pyramidal_sequence_interpolate(f32)):
        with pytest.raises(ValueError, match="colour frames must be uint8"):   # the colour warps' error
            call()
    with pytest.raises(ValueError, match="3 or 4 interleaved channels"):
        P.interpolate_frames(np.zeros((T, H, W, 2), np.uint8), *FLOWS)
    with pytest.raises(ValueError, match="order must be one of"):
        P.lucas_kanade_pyramidal_sequence_interpolate(RGB, order="gbr")
    with pytest.raises(ValueError, match="siting must be one of"):
        P.interpolate_frames_nv12(NV12, *FLOWS, siting="top")
    with pytest.raises(ValueError, match="siting must be one of"):
        P.lucas_kanade_pyramidal_sequence_interpolate_nv12(NV12, siting=1)
    with pytest.raises(ValueError, match="3H/2 rows"):
        P.interpolate_frames_nv12(np.zeros((T, 10, W), np.uint8), *FLOWS)
    with pytest.raises(ValueError, match="NV12 frames must be uint8"):
        P.lucas_kanade_pyramidal_sequence_interpolate_nv12(NV12.astype(np.float32))
    with pytest.raises(ValueError, match="at least 2 frames"):
        P.lucas_kanade_pyramidal_sequence_interpolate(RGB[:1])
    with pytest.raises(ValueError, match="at least 2 frames"):
        P.lucas_kanade_pyramidal_sequence_interpolate_nv12(NV12[:1])
    with pytest.raises(ValueError, match="every flow must have shape"):
        P.interpolate_frames(RGB, FLOWS[0], FLOWS[1], FLOWS[2], FLOWS[3][:1])
    with pytest.raises(ValueError, match="every flow must have shape"):
        P.interpolate_frames_nv12(NV12, FLOWS[0][:, :3], *FLOWS[1:])
    with pytest.raises(ValueError, match="every tau must be finite"):
        P.interpolate_frames_nv12(NV12, *FLOWS, taus=[1.0])
    with pytest.raises(ValueError, match="refine must be an integer"):
        P.lucas_kanade_pyramidal_sequence_interpolate(RGB, refine=0)
    assert stub.calls == []


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -4
BUF = np.zeros(T * 16 * 16 * 4, np.uint8)                   # frames of every layout up to 16 x 16; never read
OUTBUF = np.zeros((T - 1) * 4 * 16 * 16 * 4, np.uint8)

# fault -> (the arguments it sets, code, a piece of oflk_last_error)
FAULTS = {
    "channels=5": (dict(layout=5), INVALID, "channels must be 3 or 4"),
    "order=9": (dict(order=9), INVALID, "order must be"),
    "siting=9": (dict(layout=9), INVALID, "siting must be"),
    "H=5": (dict(H=5), INVALID, "NV12 frames need even H and W >= 4"),
    "W=2 nv12": (dict(W=2), INVALID, "NV12 frames need even H and W >= 4"),
    "T=1": (dict(T=1), INVALID, ">= "),
    "H=1": (dict(H=1), INVALID, "H and W must be >= 2"),
    "W=1": (dict(W=1), INVALID, "H and W must be >= 2"),
    "frames NULL": (dict(frames=None), INVALID, "NULL input or output argument"),
    "out NULL": (dict(out=None), INVALID, "NULL input or output argument"),
    "2^30 pixels": (dict(H=1 << 15, W=1 << 15), UNSUPPORTED, "2^30 pixels"),
    "H=2^23": (dict(H=1 << 23, W=4), UNSUPPORTED, "2^23 rows or columns"),
    "2^31 packed bytes": (dict(H=30000, W=30000), UNSUPPORTED, "packed frames of 2^31 bytes"),
    "uf NULL": (dict(null_flow=0), INVALID, "NULL flow argument"),
    "vb NULL": (dict(null_flow=3), INVALID, "NULL flow argument"),
    "levels=0": (dict(levels=0), INVALID, "levels must be"),
    "n=0": (dict(n=0), INVALID, "n must be in [1, 16]"),
    "n=17": (dict(n=17, taus=np.full(17, 0.5)), INVALID, "n must be in [1, 16]"),
    "taus NULL": (dict(taus=None), INVALID, "NULL taus"),
    "tau=0": (dict(taus=np.array([0.0])), INVALID, "taus[0] must be finite"),
    "tau=1": (dict(taus=np.array([1.0])), INVALID, "taus[0] must be finite"),
    "tau NaN": (dict(taus=np.array([math.nan])), INVALID, "taus[0] must be finite"),
    "second tau": (dict(taus=np.array([0.5, math.inf]), n=2), INVALID, "taus[1] must be finite"),
    "refine=0": (dict(refine=0), INVALID, "refine must be in [1, 8]"),
    "refine=9": (dict(refine=9), INVALID, "refine must be in [1, 8]"),
    "alpha=-1": (dict(alpha=-1.0), INVALID, "alpha and beta must be finite"),
    "beta=inf": (dict(beta=math.inf), INVALID, "alpha and beta must be finite"),
    "out on the frames' last byte": (dict(overlap="last"), INVALID, "the output overlaps the frames"),
    "frames inside out": (dict(overlap="inside"), INVALID, "the output overlaps the frames"),
}
_SETTINGS = ["n=0", "taus NULL", "tau=0", "refine=0", "alpha=-1", "out on the frames' last byte"]
_MORE = ["n=17", "tau=1", "tau NaN", "second tau", "refine=9", "beta=inf", "frames inside out", "out NULL"]
# per call: (layout kind, sequence call, device pointers, the checks in the order they are made, further faults)
CALLS = {
    "oflk_interpolate_frames_packed": ("packed", False, True, ["channels=5", "T=1", "H=1", "frames NULL", "2^30 pixels", "H=2^23",
                                                               "2^31 packed bytes", "uf NULL"] + _SETTINGS, _MORE + ["vb NULL", "W=1"]),
    "oflk_interpolate_frames_packed_host": ("packed", False, False, ["channels=5", "T=1", "H=1", "frames NULL", "2^30 pixels", "H=2^23",
                                                                    "2^31 packed bytes", "uf NULL"] + _SETTINGS, _MORE + ["vb NULL", "W=1"]),
    "oflk_interpolate_sequence_packed": ("packed", True, False, ["channels=5", "order=9", "T=1", "H=1", "frames NULL", "2^30 pixels",
                                                                 "H=2^23", "2^31 packed bytes", "levels=0"] + _SETTINGS, _MORE + ["W=1"]),
    "oflk_interpolate_frames_nv12": ("nv12", False, True, ["H=5", "siting=9", "T=1", "frames NULL", "2^30 pixels", "H=2^23", "uf NULL"]
                                     + _SETTINGS, _MORE + ["vb NULL", "W=2 nv12"]),
    "oflk_interpolate_frames_nv12_host": ("nv12", False, False, ["H=5", "siting=9", "T=1", "frames NULL", "2^30 pixels", "H=2^23",
                                                                "uf NULL"] + _SETTINGS, _MORE + ["vb NULL", "W=2 nv12"]),
    "oflk_interpolate_sequence_nv12": ("nv12", True, False, ["H=5", "siting=9", "T=1", "frames NULL", "2^30 pixels", "H=2^23",
                                                             "levels=0"] + _SETTINGS, _MORE + ["W=2 nv12"]),
}


def _call(name, *faults):
    import _oflk

    kind, seq, device, _, _ = CALLS[name]
    a = dict(frames=BUF, out=OUTBUF, T=T, H=6, W=8, layout=3 if kind == "packed" else 0, order=0, levels=2, window=5, iters=2,
             alpha=0.01, beta=0.5, refine=2, taus=np.array([0.5]), n=1, null_flow=None, overlap=None)
    for f in faults:
        a.update(FAULTS[f][0])
    fb = a["H"] * a["W"] * a["layout"] if kind == "packed" else a["H"] * a["W"] * 3 // 2
    addr = lambda x: None if x is None else x.ctypes.data   # host addresses stand in for device ones: every case is refused
    frames, out = addr(a["frames"]), addr(a["out"])
    if a["overlap"] == "last" and frames is not None:
        out = frames + a["T"] * fb - 1
    elif a["overlap"] == "inside" and frames is not None:
        out, frames = frames, frames + fb   # the frames begin one frame into the output
        a = dict(a, n=4, taus=np.full(4, 0.5)) if a["n"] == 1 and a["taus"] is not None else a
    taus = None if a["taus"] is None else np.ascontiguousarray(a["taus"], np.float64)
    cfg = (a["alpha"], a["beta"], a["refine"], None if taus is None else taus.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a["n"])
    L = _oflk.lib()
    fn = getattr(L, name)
    status = OUTBUF.ctypes.data
    if seq:
        lay = (a["layout"], a["order"]) if kind == "packed" else (a["layout"],)
        rc = fn(frames, a["T"], a["H"], a["W"], *lay, a["levels"], a["window"], a["iters"], *cfg, out, status)
    else:
        flow = np.zeros(4, np.float32)   # never read: every case is refused
        fl = [None if a["null_flow"] == i else (flow.ctypes.data if device else _oflk.ptr(flow)) for i in range(4)]
        rc = fn(frames, a["T"] - 1, a["H"], a["W"], a["layout"], *fl, *cfg, out, status, *((None,) if device else ()))
    return rc, L.oflk_last_error().decode()


def _usable(name, fault):
    return not (fault == "order=9" and not CALLS[name][1])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_c_refusals_come_before_any_device_call(name):
    """every fault alone: its code and text, with or without a device (a call that reached the device would answer
    OFLK_ERR_NO_DEVICE here, or run on arrays of the wrong size)"""
    _, _, _, order, more = CALLS[name]
    for fault in order + more:
        rc, text = _call(name, fault)
        assert rc == FAULTS[fault][1] and FAULTS[fault][2] in text, (name, fault, rc, text)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_c_refusals_keep_their_order(name):
    """each fault of the call's order together with every later one that sets other arguments: the earlier check answers"""
    order = CALLS[name][3]
    for i, first in enumerate(order):
        for second in order[i + 1:]:
            if set(FAULTS[first][0]) & set(FAULTS[second][0]):
                continue
            if "overlap" in FAULTS[second][0] and "frames" in FAULTS[first][0]:
                continue
            rc, text = _call(name, second, first)
            assert rc == FAULTS[first][1] and FAULTS[first][2] in text, (name, first, second, rc, text)


def test_the_new_symbols_are_declared_and_exported():
    import _oflk

    from pathlib import Path

    header = (Path(__file__).resolve().parents[1] / "include" / "oflk.h").read_text()
    L = _oflk.lib()
    for name in CALLS:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
        assert f"int {name}(" in header
    n_args = {n: len(getattr(L, n).argtypes) for n in CALLS}
    assert n_args == {"oflk_interpolate_frames_packed": 17, "oflk_interpolate_frames_nv12": 17,
                      "oflk_interpolate_frames_packed_host": 16, "oflk_interpolate_frames_nv12_host": 16,
                      "oflk_interpolate_sequence_packed": 16, "oflk_interpolate_sequence_nv12": 15}
