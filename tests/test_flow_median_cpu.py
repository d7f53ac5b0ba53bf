"""CPU tests of the median filter of dense flows: the statement of tests/flow_median_model.py against SciPy and against its
own order, what it does to flows with a known answer and to the interpolation of the pan scenes (the flows are the CPU
oracle's), and the refusals and the marshalling of the C ABI and of the Python tier, all made before any device call.  The
kernel is held to the statement in tests/test_gpu_flow_median.py."""
import ctypes

import numpy as np
import pytest

import flow_median_model as FMM
import interp_model as M
from mosaic_median_model import key
from test_python_marshalling_cpu import StubLib, recorded

SIZES = FMM.SIZES


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (2, 3), (9, 9), (37, 53)], ids=str)
def test_statement_equals_scipy_on_finite_planes(H, W, size):
    """values, not bits: SciPy does not order -0 below +0"""
    from scipy.ndimage import median_filter

    rng = np.random.default_rng(H * 100 + W + size)
    for p in (rng.standard_normal((H, W)).astype(np.float32), FMM.quantised_planes(1, H, W, seed=size)[0]):
        got = FMM.median_plane(p, size)
        assert got.dtype == np.float32 and got.shape == (H, W)
        assert np.array_equal(got, median_filter(p, size=size, mode="nearest"))


@pytest.mark.parametrize("size", SIZES)
def test_specials_follow_the_statements_own_order(size):
    """-NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN: a plain Python sort by key on a handful of pixels"""
    H, W = 11, 13
    p = FMM.special_planes(1, H, W, seed=size)[0]
    got = FMM.median_plane(p, size).view(np.uint32)
    r = size // 2
    bits = p.view(np.uint32)
    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (5, 6), (1, 11), (9, 2), (4, 0), (10, 7)]:
        window = [int(bits[min(max(y + j, 0), H - 1), min(max(x + i, 0), W - 1)]) for j in range(-r, r + 1) for i in range(-r, r + 1)]
        window.sort(key=lambda b: int(key(np.array([b], np.uint32).view(np.float32))[0]))
        assert int(got[y, x]) == window[size * size // 2], (y, x)
    order = np.array([0xFFC00000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000], np.uint32)
    k = key(order.view(np.float32)).astype(np.int64)
    assert (np.diff(k) > 0).all()
    special = set(int(b) for b in FMM.SPECIALS.view(np.uint32))
    assert set(int(b) for b in got.ravel()) & special   # a special value is the middle of some window ...
    assert not np.isin(got, bits, invert=True).any()     # ... and every result is one of the inputs, bit for bit


@pytest.mark.parametrize("size", SIZES)
def test_planar_flow_comes_back_bit_for_bit_inside(size):
    """a x + b y + c in small dyadic numbers is exact in float32, and the window is symmetric about its centre value: the
    values pair off around it, so it is the middle one"""
    H, W = 21, 27
    r = size // 2
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for a, b, c in ((0.25, -0.5, 3.0), (0.0, 0.125, -1.0), (-0.375, 0.0, 0.0), (0.0, 0.0, -0.0)):
        p = (np.float32(a) * x + np.float32(b) * y + np.float32(c)).astype(np.float32)
        got = FMM.median_plane(p, size)
        inner = (slice(r, H - r), slice(r, W - r))
        assert np.array_equal(got[inner].view(np.uint32), p[inner].view(np.uint32))


@pytest.mark.parametrize("size", SIZES)
def test_isolated_outliers_leave_a_constant_flow_constant(size):
    """clusters of (size^2 - 1) / 2 outliers, each inside a size x size cell, the cells 2 size apart: a window reaches one
    cell at most, so it holds at most (size^2 - 1) / 2 outliers, and some window holds exactly that many"""
    H, W = 40, 44
    c = np.float32(1.75)
    half = (size * size - 1) // 2
    p = np.full((H, W), c, np.float32)
    rng = np.random.default_rng(size)
    for y0 in range(size, H - size, 2 * size):
        for x0 in range(size, W - size, 2 * size):
            cells = rng.permutation(size * size)[:half]   # a cluster inside one size x size cell, 2 size apart from the next
            p[y0 + cells // size, x0 + cells % size] = rng.choice(np.float32([1e30, -1e30, np.inf, -np.inf, np.nan, 100.0]), half)
    k = FMM.window_keys(p, size)
    assert ((k != key(c)).sum(0).max()) == half
    got = FMM.median_plane(p, size)
    assert np.array_equal(got.view(np.uint32), np.full((H, W), c, np.float32).view(np.uint32))


PANS = [(3, 1), (6, -2)]


@pytest.mark.parametrize("pan", PANS, ids=str)
def test_pan_scenes_gain_from_the_median(oracle, pan):
    """interp_model.pan_scene, the oracle's flows at 3 levels, window 5, 3 iterations, tau = 0.5, the flows put through the
    statement at sizes 5 and 9: the mean absolute error against the true middle frame, 12 px inside the border, is strictly
    smaller than with the unfiltered flows, and the share of status 3 larger.  Measured (error / share of status 3, no filter,
    5 x 5, 9 x 9): pan (3, 1): 0.709 / 0.802, 0.630 / 0.897, 0.566 / 0.919; pan (6, -2): 1.981 / 0.627, 1.592 / 0.717,
    1.372 / 0.763: 11 - 31 % lower error."""
    A, mid, B = M.pan_scene(*pan)
    flows = [f[0] for f in M.oracle_flows(oracle, np.stack([A, B]))]
    inner = (slice(12, -12), slice(12, -12))

    def measure(fl):
        out, status = M.interpolate_pair(A, B, *fl, 0.5)
        return float(np.abs(out - mid)[inner].mean()), float((status[inner] == 3).mean())

    err0, share0 = measure(flows)
    print(f"pan {pan}: no filter {err0:.3f} / {share0:.3f}")
    for size in (5, 9):
        err, share = measure([FMM.median_plane(f, size) for f in flows])
        print(f"pan {pan}: {size} x {size} {err:.3f} / {share:.3f}, error ratio {err / err0:.3f}")
        assert err < err0
        assert share > share0


# ---- refusals ------------------------------------------------------------------------------------------------------------
T, H, W = 3, 6, 8
FRAMES = {"f32": np.zeros((T, H, W), np.float32), "u8": np.zeros((T, H, W), np.uint8),
          "colour": np.zeros((T, H, W, 3), np.uint8), "nv12": np.zeros((T, 3 * H // 2, W), np.uint8)}
BAD_MEDIANS = [1, 2, 4, 6, 11, -3, 5.0, True, "5", None]


def _python_sequence_calls():
    import lucas_kanade_pyramidal as P

    return {"fb f32": lambda **kw: P.lucas_kanade_pyramidal_sequence_fb(FRAMES["f32"], **kw),
            "fb u8": lambda **kw: P.lucas_kanade_pyramidal_sequence_fb(FRAMES["u8"], **kw),
            "interpolate f32": lambda **kw: P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["f32"], **kw),
            "interpolate u8": lambda **kw: P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["u8"], **kw),
            "interpolate colour": lambda **kw: P.lucas_kanade_pyramidal_sequence_interpolate(FRAMES["colour"], order="bgr", **kw),
            "interpolate nv12": lambda **kw: P.lucas_kanade_pyramidal_sequence_interpolate_nv12(FRAMES["nv12"], **kw)}


@pytest.mark.parametrize("bad", BAD_MEDIANS, ids=repr)
def test_python_refuses_a_bad_flow_median(monkeypatch, bad):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    for name, call in _python_sequence_calls().items():
        with pytest.raises(ValueError, match="flow_median must be 0, 3, 5, 7 or 9"):
            call(flow_median=bad)
    with pytest.raises(ValueError, match="size must be 3, 5, 7 or 9"):
        P.median_filter_flow(np.zeros((2, H, W), np.float32), size=bad)
    assert stub.calls == []


def test_python_refuses_arrays_that_are_no_planes(monkeypatch):
    import _oflk
    import lucas_kanade_pyramidal as P

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    for bad in (np.zeros(5, np.float32), np.float32(1.0), np.zeros((2, 0, 4), np.float32)):
        with pytest.raises(ValueError, match=r"\(\.\.\., H, W\) array of flow planes"):
            P.median_filter_flow(bad)
    with pytest.raises(ValueError, match="size must be 3, 5, 7 or 9"):
        P.median_filter_flow(np.zeros((H, W), np.float32), size=0)
    assert stub.calls == []


def test_python_marshalling(monkeypatch):
    """flow_median = 0 records the call that is made without the keyword; 5 records the _median name with 5 in the C order"""
    import lucas_kanade_pyramidal as P

    a = repr(float(np.float32(0.01)))
    today = {
        "fb f32": f"oflk_pyramidal_sequence_fb(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr)",
        "fb u8": f"oflk_pyramidal_sequence_fb_u8(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr)",
        "interpolate f32": f"oflk_interpolate_sequence(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, 2, ptr, 1, ptr, ptr)",
        "interpolate u8": f"oflk_interpolate_sequence_u8(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, 2, ptr, 1, ptr, ptr)",
        "interpolate colour": f"oflk_interpolate_sequence_packed(ptr, {T}, {H}, {W}, 3, 1, 3, 5, 3, {a}, 0.5, 2, ptr, 1, ptr, ptr)",
        "interpolate nv12": f"oflk_interpolate_sequence_nv12(ptr, {T}, {H}, {W}, 0, 3, 5, 3, {a}, 0.5, 2, ptr, 1, ptr, ptr)",
    }
    median = {
        "fb f32": f"oflk_pyramidal_sequence_fb_median(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, 5, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr)",
        "fb u8": f"oflk_pyramidal_sequence_fb_median_u8(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, 5, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr)",
        "interpolate f32": f"oflk_interpolate_sequence_median(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, 2, ptr, 1, 5, ptr, ptr)",
        "interpolate u8": f"oflk_interpolate_sequence_median_u8(ptr, {T}, {H}, {W}, 3, 5, 3, {a}, 0.5, 2, ptr, 1, 5, ptr, ptr)",
        "interpolate colour": f"oflk_interpolate_sequence_packed_median(ptr, {T}, {H}, {W}, 3, 1, 3, 5, 3, {a}, 0.5, 2, ptr, 1, 5, ptr, ptr)",
        "interpolate nv12": f"oflk_interpolate_sequence_nv12_median(ptr, {T}, {H}, {W}, 0, 3, 5, 3, {a}, 0.5, 2, ptr, 1, 5, ptr, ptr)",
    }
    for name, call in _python_sequence_calls().items():
        assert recorded(monkeypatch, call) == [today[name]], name
        assert recorded(monkeypatch, lambda: call(flow_median=0)) == [today[name]], name
        assert recorded(monkeypatch, lambda: call(flow_median=np.int64(0))) == [today[name]], name
        assert recorded(monkeypatch, lambda: call(flow_median=5)) == [median[name]], name
        assert recorded(monkeypatch, lambda: call(flow_median=np.int32(5))) == [median[name]], name
    planes = np.zeros((2, 4, H, W), np.float64)
    assert recorded(monkeypatch, lambda: P.median_filter_flow(planes)) == [f"oflk_flow_median_host(ptr, ptr, 8, {H}, {W}, 5)"]
    assert recorded(monkeypatch, lambda: P.median_filter_flow(planes[0, 0], size=9)) == [f"oflk_flow_median_host(ptr, ptr, 1, {H}, {W}, 9)"]
    monkeypatch.undo()


def _c_calls():
    """every C entry point of the feature as call(**overrides) -> return code, on valid small arguments"""
    import _oflk

    L = _oflk.lib()
    f64p = ctypes.POINTER(ctypes.c_double)
    P_ = 2

    def planes(host):
        def call(**kw):
            a = dict(inp=np.zeros((P_, H, W), np.float32), out=np.zeros((P_, H, W), np.float32), P=P_, H=H, W=W, size=5)
            a.update(kw)
            if host:
                p = lambda x: None if x is None else _oflk.ptr(x)
                return L.oflk_flow_median_host(p(a["inp"]), p(a["out"]), a["P"], a["H"], a["W"], a["size"])
            p = lambda x: None if x is None else x.ctypes.data   # host addresses stand in: every refusal comes before they are used
            return L.oflk_flow_median(p(a["inp"]), p(a["out"]), a["P"], a["H"], a["W"], a["size"], None)
        return call

    def sequence(name, kind, layout_args):
        def call(**kw):
            fr = FRAMES[kind]
            a = dict(frames=fr, T=T, H=H, W=W, levels=2, flow_median=5, out=np.zeros((T - 1, 1) + fr.shape[1:], fr.dtype))
            a.update(kw)
            p = lambda x: None if x is None else (_oflk.ptr(x) if x.dtype == np.float32 else x.ctypes.data)
            fl = [np.zeros((T - 1, H, W), np.float32) for _ in range(6)]
            if "fb" in name:
                return getattr(L, name)(p(a["frames"]), a["T"], a["H"], a["W"], a["levels"], 5, 2, 0.01, 0.5, a["flow_median"],
                                        *(_oflk.ptr(f) for f in fl), None, None)
            taus = np.array([0.5]).ctypes.data_as(f64p)
            return getattr(L, name)(p(a["frames"]), a["T"], a["H"], a["W"], *layout_args, a["levels"], 5, 2, 0.01, 0.5, 2, taus, 1,
                                    a["flow_median"], p(a["out"]), None)
        return call

    return {"planes": {"device": planes(False), "host": planes(True)},
            "sequences": {"fb": sequence("oflk_pyramidal_sequence_fb_median", "f32", ()),
                          "fb_u8": sequence("oflk_pyramidal_sequence_fb_median_u8", "u8", ()),
                          "interp": sequence("oflk_interpolate_sequence_median", "f32", ()),
                          "interp_u8": sequence("oflk_interpolate_sequence_median_u8", "u8", ()),
                          "packed": sequence("oflk_interpolate_sequence_packed_median", "colour", (3, 0)),
                          "nv12": sequence("oflk_interpolate_sequence_nv12_median", "nv12", (0,))}}


def test_c_refusals_of_the_plane_forms_come_before_any_device_call():
    """OFLK_ERR_INVALID with or without a device: a call that reached the device would answer OFLK_ERR_NO_DEVICE here, or run"""
    import _oflk

    inv = _oflk.OFLK_ERR_INVALID
    for name, call in _c_calls()["planes"].items():
        err = lambda: (name, _oflk.lib().oflk_last_error())
        assert call(inp=None) == inv, err()
        assert call(out=None) == inv, err()
        assert call(P=0) == inv and call(P=-1) == inv, err()
        for size in (0, 1, 2, 4, 6, 8, 10, 11, -5):
            assert call(size=size) == inv, (size, err())
        assert call(H=0) == inv and call(W=0) == inv, err()
        assert call(H=1 << 23) == _oflk.OFLK_ERR_UNSUPPORTED and call(H=1 << 15, W=1 << 15) == _oflk.OFLK_ERR_UNSUPPORTED, err()
        # an output that overlaps the input: its first byte on the input's last byte, its first value on the input's last one,
        # the input starting inside the output (the two are of one size, so neither can lie within the other short of being
        # it), and in place
        n = 2 * H * W
        buf = np.zeros(3 * n, np.float32)
        assert call(inp=buf[:n], out=buf.view(np.uint8)[4 * n - 1:8 * n - 1].view(np.float32)) == inv, err()
        assert call(inp=buf[:n], out=buf[n - 1:2 * n - 1]) == inv, err()
        assert call(inp=buf[n // 2:n // 2 + n], out=buf[:n]) == inv, err()
        assert call(inp=buf[:n], out=buf[:n]) == inv, err()
        assert b"overlaps" in _oflk.lib().oflk_last_error()
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert _oflk.lib().oflk_flow_median_tile(None, ctypes.byref(tw)) == inv
    assert _oflk.lib().oflk_flow_median_tile(ctypes.byref(th), None) == inv
    th, tw = _oflk.flow_median_tile()
    assert th >= 1 and tw >= 1 and th * tw == 256   # a block of 256 lanes, one output pixel a lane


def test_c_refusals_of_the_sequence_forms_come_before_any_device_call():
    import _oflk

    inv = _oflk.OFLK_ERR_INVALID
    for name, call in _c_calls()["sequences"].items():
        err = lambda: (name, _oflk.lib().oflk_last_error())
        for bad in (1, 2, 4, 6, 8, 10, 11, -3):
            assert call(flow_median=bad) == inv, (bad, err())
            assert b"flow_median must be 0, 3, 5, 7 or 9" in _oflk.lib().oflk_last_error()
        for k in (0, 3, 5, 7, 9):   # what the unfiltered call refuses, with its codes, whatever the setting
            assert call(flow_median=k, T=1) == inv, (k, err())
            assert call(flow_median=k, frames=None) == inv, (k, err())
            assert call(flow_median=k, levels=0) == inv, (k, err())
            assert call(flow_median=k, H=1 << 23) == _oflk.OFLK_ERR_UNSUPPORTED, (k, err())
        if "fb" not in name:
            assert call(out=None) == inv, err()
