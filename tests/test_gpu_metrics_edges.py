"""GPU tests of the masked flow metrics against their statement (tests/metrics_model.py) on the scenes of
tests/metrics_scenes.py: rectangle edges and NumPy slice semantics, every element summed once, NaN / inf / overflow /
subnormal values and the "nothing moves" branch, 4K and 8K sums, 300 and 65 537 pairs.

One rule per output (`_compare`): both NaN, or the same infinity, or the same exact 0.0, or finite and at most ONE float32
ulp apart.  The ulp is derived: the model's five sums are exact; the device adds n non-negative float64 terms, so its sum is
within (n - 1) * 2^-53 <= 3.7e-9 relative of the exact one for n <= 3.3e7 -- below half a float32 ulp -- so after the
rounding to float32 the two differ by at most one ulp, and only where the exact mean lies within 3.7e-9 relative of a
rounding tie (the square root halves it for rmse; the float64 acos of the device and of libm add about 1e-15).  Each test
prints how many outputs were equal and how many one ulp off.

The device result is also held to the reference's own numbers (tests/golden/reference_metrics.json) by the derived bound
of metrics_model.reference_bound; tests/test_metrics_cpu.py shows that it is the scenes, not that bound, that catch a
mistake.  No scene reads outside the flow planes."""
import ctypes
import math

import numpy as np
import pytest

import metrics_model as M
import metrics_scenes as S

pytestmark = pytest.mark.gpu

FIX = S.fixture()
TERM = FIX["arccos_deg_term_error"]
_F64P = ctypes.POINTER(ctypes.c_double)


def _compare(dev, model, what, tally):
    """the rule above on (B, 5) arrays; tally = [equal, one ulp off]"""
    dev, model = np.asarray(dev, np.float64), np.asarray(model, np.float64)
    assert dev.shape == model.shape, (what, dev.shape, model.shape)
    for b in range(dev.shape[0]):
        for k, d, m in zip(M.KEYS, dev[b], model[b]):
            assert float(np.float32(d)) == d or math.isnan(d), (what, b, k, d, "not a float32 value")
            if M.kind(m) != "finite" or M.kind(d) != "finite":
                assert M.kind(d) == M.kind(m), (what, b, k, d, m)
                tally[0] += 1
                continue
            ulps = M.ulps_apart(d, m)
            assert ulps <= 1, (what, b, k, d, m, ulps)
            tally[ulps] += 1


def _against_reference(dev, name, what):
    entry = FIX["scenes"][name]
    for row, b in zip(entry["metrics"], S.fixture_pairs(name, FIX)):
        for k, d, ref in zip(M.KEYS, dev[b], row):
            assert M.agrees_with_reference(float(d), ref, entry["n"], k, TERM), (what, b, k, float(d), ref)


def _flow_metrics(u, v, ut, vt, region):
    """oflk_flow_metrics on host arrays: (B, 5)"""
    import _oflk

    B, H, W = u.shape
    out = np.full((B, 5), -7.0, np.float64)
    _oflk.check(_oflk.lib().oflk_flow_metrics(_oflk.ptr(u), _oflk.ptr(v), B, H, W, _oflk.ptr(ut), _oflk.ptr(vt), *region,
                                              out.ctypes.data_as(_F64P)))
    return out


class _Dev:
    """device memory through the HIP runtime liboflk is linked to; `skew` floats past the allocation's 256-byte alignment"""

    def __init__(self, arr, skew=0):
        import _oflk

        _oflk.lib()
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.base = ctypes.c_void_p()
        arr = np.ascontiguousarray(arr)
        assert self.hip.hipMalloc(ctypes.byref(self.base), ctypes.c_size_t(arr.nbytes + 4 * skew)) == 0
        self.ptr = self.base.value + 4 * skew
        assert self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(arr.nbytes), 1) == 0
        self.shape, self.dtype = arr.shape, arr.dtype

    def to_host(self):
        out = np.empty(self.shape, self.dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipFree(self.base) == 0


def _plan_metrics(u, v, ut, vt, region, stream=0, skew=0, repeat=1):
    """oflk_plan_metrics on device-resident copies of the scene: list of `repeat` (B, 5) results"""
    import _oflk

    B, H, W = u.shape
    du, dv = _Dev(u, skew), _Dev(v, skew)
    plan = _oflk.Plan(0, B, H, W, 1, 5, 0)
    try:
        return [plan.metrics(du.ptr, dv.ptr, ut, vt, region, stream) for _ in range(repeat)]
    finally:
        plan.close()
        du.free()
        dv.free()


def _same_bytes(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


@pytest.mark.parametrize("family", ("edges", "once", "values", "noise", "sizes"))
def test_both_entry_points_equal_the_statement(family):
    """every scene of the family through oflk_flow_metrics and (all but the 65 537-pair batch) oflk_plan_metrics: the rule
    against the model, the derived bound against the reference's numbers, and the two entry points the same bytes"""
    tally = [0, 0]
    for name in S.SCENES:
        if S.FAMILY[name] != family:
            continue
        u, v, ut, vt, region = S.checked_scene(name, FIX)
        model = M.batch_metrics(u, v, ut, vt, region)
        dev = _flow_metrics(u, v, ut, vt, region)
        _compare(dev, model, name + " (flow_metrics)", tally)
        _against_reference(dev, name, name)
        if name != S.MANY:
            got = _plan_metrics(u, v, ut, vt, region)[0]
            assert _same_bytes(got, dev), (name, got, dev)
    print(f"{family}: {tally[0]} outputs equal to the statement, {tally[1]} one float32 ulp off")
    assert tally[0] > 0


def test_the_scenes_that_name_the_old_kernel_s_mistakes():
    """the values the issue of this test names, spelled out: a NaN or infinite flow value inside the region makes aae NaN
    (a clip by fmaxf / fminf made it finite); zero truth, zero prediction and one NaN pixel make aae NaN (an fmax over
    |pred| made it 0.0)"""
    u, v, ut, vt, region = S.scene("values/special_inside")
    dev = _flow_metrics(u, v, ut, vt, region)
    for b, (plane, val) in enumerate(S.SPECIALS):
        if not math.isfinite(val):
            assert math.isnan(dev[b, 4]), (b, plane, val, dev[b])
    u, v, ut, vt, region = S.scene("values/zero_truth")
    dev = _flow_metrics(u, v, ut, vt, region)
    assert dev[0, 4] == 0.0 and math.isnan(dev[1, 4]) and dev[2, 4] == 0.0 and dev[3, 4] == 0.0, dev[:, 4]


@pytest.mark.parametrize("name", ("noise/240x320_border", "once/spikes", "values/special_inside", "edges/67x91/negative"))
def test_plan_metrics_on_a_stream_on_skewed_planes_and_twice(name):
    """a non-default stream, planes one float past 16-byte alignment, two calls in a row: the bytes of the plain call"""
    import _oflk

    u, v, ut, vt, region = S.scene(name)
    plain = _plan_metrics(u, v, ut, vt, region)[0]
    tally = [0, 0]
    _compare(plain, M.batch_metrics(u, v, ut, vt, region), name, tally)
    _oflk.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    try:
        for skew in (0, 1):
            for got in _plan_metrics(u, v, ut, vt, region, stream=stream.value, skew=skew, repeat=2):
                assert _same_bytes(got, plain), (name, skew, got, plain)
        for got in _plan_metrics(u, v, ut, vt, region, skew=1, repeat=2):
            assert _same_bytes(got, plain), (name, got, plain)
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def test_plan_metrics_after_a_pyramidal_pass_of_the_same_plan():
    """the plan's own flows, then a scene's planes, reduced by the plan that has just run a pyramidal pass"""
    import _oflk
    from oflk_synth import synth_pair

    B, H, W = 3, 120, 160
    pairs = [synth_pair(H, W, i, dx=1.0 + i, dy=-0.5 * i) for i in range(B)]
    prev, curr = _Dev(np.stack([a for a, _ in pairs])), _Dev(np.stack([b for _, b in pairs]))
    du, dv = _Dev(np.zeros((B, H, W), np.float32)), _Dev(np.zeros((B, H, W), np.float32))
    ut = np.array([1.0 + i for i in range(B)], np.float32)
    vt = np.array([-0.5 * i for i in range(B)], np.float32)
    su, sv = S.noisy((B, H, W), 21, (0.0, 0.0))
    su[1, 50, 60] = np.nan
    eu, ev = _Dev(su), _Dev(sv)
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    try:
        plan.pyramidal(prev.ptr, curr.ptr, du.ptr, dv.ptr, 0)
        got = plan.metrics(du.ptr, dv.ptr, ut, vt, (10, -10, 10, -10), 0)
        other = plan.metrics(eu.ptr, ev.ptr, ut, vt, (-H - 5, H // 2, 3, W + 9), 0)
        again = plan.metrics(du.ptr, dv.ptr, ut, vt, (10, -10, 10, -10), 0)
        hu, hv = du.to_host(), dv.to_host()
    finally:
        plan.close()
        for buf in (prev, curr, du, dv, eu, ev):
            buf.free()
    tally = [0, 0]
    _compare(got, M.batch_metrics(hu, hv, ut, vt, (10, -10, 10, -10)), "plan flows", tally)
    _compare(other, M.batch_metrics(su, sv, ut, vt, (-H - 5, H // 2, 3, W + 9)), "scene planes", tally)
    assert math.isnan(other[1, 0]) and math.isnan(other[1, 4]) and np.isfinite(other[[0, 2]]).all()
    assert _same_bytes(got, again)
    print(f"after a pyramidal pass: {tally[0]} equal, {tally[1]} one ulp off")


@pytest.mark.parametrize("name", ("once/spikes", "values/special_inside", "values/zero_truth", "sizes/B300_33x40"))
def test_a_batched_call_equals_pair_by_pair_calls_byte_for_byte(name):
    """the host adds each pair's 64 block partials in a fixed order, so a pair's numbers do not depend on its batch"""
    u, v, ut, vt, region = S.scene(name)
    batched = _flow_metrics(u, v, ut, vt, region)
    for b in range(u.shape[0]):
        one = _flow_metrics(u[b:b + 1], v[b:b + 1], ut[b:b + 1], vt[b:b + 1], region)
        assert _same_bytes(one[0], batched[b]), (name, b, one[0], batched[b])


@pytest.mark.parametrize("scene", ("big", "steep"))
def test_verifier_verdicts_on_non_finite_flows_do_not_depend_on_where_the_metrics_are_reduced(scene):
    """frames that make NaN (`big`) and +inf (`steep`) flows inside the test region (tests/range_scenes.py): verify_pattern(device_metrics=True) gives every metric the
    class, and every finite metric the value within the reference bound, that the NumPy reduction gives, and so the status"""
    import generate_test_suite as G
    import optical_flow_verifier as V
    import range_scenes as R
    from conftest import PRODUCT

    cfg = V.load_config(PRODUCT / "verification_config.yaml")
    p, c = R.scene(scene, "tm")
    data = {"frame_prev": p, "frame_curr": c, "metadata": {"motion_parameters": G.TEST_PATTERNS["translate_medium"].to_dict()}}
    with np.errstate(all="ignore"):
        host = V.verify_pattern("translate_medium", data, cfg, verbose=False, device_metrics=False)
        dev = V.verify_pattern("translate_medium", data, cfg, verbose=False, device_metrics=True)
    n = host["num_test_pixels"]
    classes = set()
    for key in ("single_scale", "pyramidal"):
        for k in M.KEYS:
            h, d = host[key]["metrics"][k], dev[key]["metrics"][k]
            classes.add(M.kind(h))
            assert M.agrees_with_reference(d, h if math.isfinite(h) else repr(h), n, k, TERM), (scene, key, k, d, h)
        assert dev[key]["status"] == host[key]["status"], (scene, key)
    assert classes & {"nan", "+inf"}, (scene, classes)   # the scene did bring a non-finite metric


def test_invalid_arguments_are_refused_before_anything_is_launched():
    import _oflk

    L = _oflk.lib()
    u, v, ut, vt, region = S.scene("noise/33x40_row")
    B, H, W = u.shape
    out = np.full((B, 5), -7.0, np.float64)
    o = out.ctypes.data_as(_F64P)
    pu, pv, put, pvt = _oflk.ptr(u), _oflk.ptr(v), _oflk.ptr(ut), _oflk.ptr(vt)
    bad = [(None, pv, B, H, W, put, pvt, o), (pu, None, B, H, W, put, pvt, o), (pu, pv, B, H, W, None, pvt, o),
           (pu, pv, B, H, W, put, None, o), (pu, pv, B, H, W, put, pvt, None)]
    bad += [(pu, pv, b, h, w, put, pvt, o) for b, h, w in ((0, H, W), (-1, H, W), (B, 0, W), (B, -3, W), (B, H, 0), (B, H, -1))]
    for a in bad:
        rc = L.oflk_flow_metrics(a[0], a[1], a[2], a[3], a[4], a[5], a[6], *region, a[7])
        assert rc == _oflk.OFLK_ERR_INVALID, (a[2:5], rc)
    d = _Dev(u)
    plan = _oflk.Plan(0, B, H, W, 1, 5, 0)
    try:
        assert L.oflk_plan_metrics(None, d.ptr, d.ptr, put, pvt, *region, o, None) == _oflk.OFLK_ERR_INVALID
        for a in ((None, d.ptr, put, pvt, o), (d.ptr, None, put, pvt, o), (d.ptr, d.ptr, None, pvt, o),
                  (d.ptr, d.ptr, put, None, o), (d.ptr, d.ptr, put, pvt, None)):
            assert L.oflk_plan_metrics(plan._h, a[0], a[1], a[2], a[3], *region, a[4], None) == _oflk.OFLK_ERR_INVALID
    finally:
        plan.close()
        d.free()
    assert (out == -7.0).all()   # nothing was written
