"""The metrics statement (tests/metrics_model.py) on the CPU: its rectangle rule against Python's slices, its numbers against
the reference's (tests/golden/reference_metrics.json) on every scene of tests/metrics_scenes.py, and -- because the bound to
the reference is loose (float32 pairwise means against exact ones) -- a check that each scene does what it was built for:
the kernel mistake it names, applied to the model, moves some output at least TEN times the GPU test's tolerance (one
float32 ulp), or changes its class (finite / NaN / inf / exact 0).  No GPU."""
import math

import numpy as np
import pytest

import metrics_model as M
import metrics_scenes as S

FIX = S.fixture()
TERM = FIX["arccos_deg_term_error"]


def test_rectangle_rule_is_the_slice_rule():
    for n in range(1, 7):
        for a in range(-n - 2, n + 3):
            for b in range(-n - 2, n + 3):
                r = range(n)[a:b]
                lo, hi = M.bound(a, n), M.bound(b, n)
                assert max(hi - lo, 0) == len(r) and lo == r.start, (n, a, b)
    for H, W in S.EDGE_FRAMES:
        for region in S.edge_regions(H, W).values():
            y0, y1, x0, x1 = M.rectangle(region, H, W)
            mask = np.zeros((H, W), bool)
            mask[region[0]:region[1], region[2]:region[3]] = True
            assert M.count((y0, y1, x0, x1)) == int(mask.sum())
            if mask.any():
                assert mask[y0:y1, x0:x1].all()


def test_fixture_holds_every_scene_and_nothing_else():
    assert sorted(FIX["scenes"]) == sorted(S.SCENES)
    assert FIX["keys"] == list(M.KEYS)
    assert 0 < TERM < 1e-4   # NumPy's float32 arccos is good to a few ulp of 180 degrees (1.5e-5)


def _model_against_fixture(name):
    u, v, ut, vt, region = S.checked_scene(name, FIX)
    entry = FIX["scenes"][name]
    pairs = S.fixture_pairs(name, FIX)
    worst = 0.0
    for row, b in zip(entry["metrics"], pairs):
        got = M.pair_metrics(u[b], v[b], ut[b], vt[b], region)
        for k, ref in zip(M.KEYS, row):
            assert M.agrees_with_reference(got[k], ref, entry["n"], k, TERM), (name, b, k, got[k], ref)
            if isinstance(ref, float) and ref != 0.0 and math.isfinite(got[k]):
                worst = max(worst, abs(got[k] - ref) / abs(ref))
    return worst


@pytest.mark.parametrize("family", ("edges", "once", "values", "sizes", "noise"))
def test_model_equals_the_reference_within_numpy_s_own_error(family):
    """NaN where the reference has NaN, the same infinity, aae == 0.0 where it has 0.0, finite values within
    metrics_model.reference_bound -- a derived bound, loose at large n (6.2e-5 at 4K), which is why the scenes carry the
    test and not this tolerance."""
    worst = 0.0
    for name in S.SCENES:
        if S.FAMILY[name] == family:
            worst = max(worst, _model_against_fixture(name))
    print(f"{family}: worst relative gap model - reference {worst:.2e}")


def _moved(a, b) -> bool:
    """some output changes class, or moves at least 10 float32 ulps"""
    for x, y in zip(np.ravel(a), np.ravel(b)):
        if M.kind(x) != M.kind(y):
            return True
        if M.kind(x) in ("finite",) and M.ulps_apart(x, y) >= 10:
            return True
    return False


def _one(name, b=0, **hooks):
    u, v, ut, vt, region = S.scene(name)
    return [M.pair_metrics(u[b], v[b], ut[b], vt[b], region, **hooks)[k] for k in M.KEYS]


def test_edge_scenes_see_a_rectangle_one_short_or_one_long_on_any_side():
    tried = 0
    for H, W in S.EDGE_FRAMES:
        for which in S.EDGE_REGIONS:
            name = f"edges/{H}x{W}/{which}"
            u, v, ut, vt, region = S.scene(name)
            rect = M.rectangle(region, H, W)
            if M.count(rect) == 0:
                continue
            good = M.batch_metrics(u, v, ut, vt, region)
            for side in range(4):
                for step in (-1, 1):
                    bad = list(rect)
                    bad[side] += step
                    if min(bad) < 0 or bad[0] > H or bad[1] > H or bad[2] > W or bad[3] > W:
                        continue    # would leave the frame: not a mistake a GPU test may run
                    if bad == list(rect):
                        continue
                    assert _moved(good, M.batch_metrics(u, v, ut, vt, region, rect=tuple(bad))), (name, rect, bad)
                    tried += 1
    assert tried > 200, tried
    # a reversed or empty slice taken for its absolute size, or for the whole frame
    for H, W in ((67, 91), (240, 320)):
        for which in ("reversed", "reversed_neg", "zero_width", "zeros"):
            u, v, ut, vt, region = S.scene(f"edges/{H}x{W}/{which}")
            good = M.batch_metrics(u, v, ut, vt, region)
            assert all(math.isnan(x) for x in good.ravel())
            assert _moved(good, M.batch_metrics(u, v, ut, vt, region, rect=(0, H, 0, W)))


STRIDE = 64 * 256


def _stride_plus_one(n):
    """a grid stride of 64 * 256 + 1: elements 16 384, 32 769, ... are never visited"""
    e = np.arange(n)
    return e[e % (STRIDE + 1) != STRIDE]


def test_once_scenes_see_a_dropped_a_doubled_and_a_skipped_element():
    for n in S.ONCE_COUNTS:
        name = f"once/count_{n}"
        good = _one(name)
        assert _moved(good, _one(name, keep=lambda k: np.arange(k - 1))), name                       # last one dropped
        assert _moved(good, _one(name, keep=lambda k: np.arange(1, k))), name                        # first one dropped
        assert _moved(good, _one(name, keep=lambda k: np.concatenate([np.arange(k), [k - 1]]))), name   # last one twice
        if n > STRIDE:
            assert _moved(good, _one(name, keep=_stride_plus_one)), name
    u, v, ut, vt, region = S.scene("once/spikes")
    pos = S.once_positions()
    good = M.batch_metrics(u, v, ut, vt, region)
    assert (good[:, 0] > 0).all()
    for b, e in enumerate(pos):
        lost = M.pair_metrics(u[b], v[b], ut[b], vt[b], region, keep=lambda k, e=e: np.delete(np.arange(k), e))
        assert lost["mae_u"] == 0.0 and lost["epe"] == 0.0, (b, e)
    b = pos.index(STRIDE)
    assert M.pair_metrics(u[b], v[b], ut[b], vt[b], region, keep=_stride_plus_one)["mae_u"] == 0.0


@pytest.mark.parametrize("name", ("once/spikes", "sizes/B300_33x40"))
def test_batched_scenes_see_pair_zero_s_truth_used_for_every_pair(name):
    u, v, ut, vt, region = S.scene(name)
    good = M.batch_metrics(u, v, ut, vt, region)
    bad = M.batch_metrics(u, v, np.full_like(ut, ut[0]), np.full_like(vt, vt[0]), region)
    differs = [b for b in range(len(ut)) if (ut[b], vt[b]) != (ut[0], vt[0])]
    assert len(differs) >= len(ut) * 0.9
    for b in differs:
        assert _moved(good[b], bad[b]), (name, b)


def _clip_fmax_fmin(c):
    """fminf(fmaxf(c, -1), 1): both drop a NaN operand"""
    return np.fmin(np.fmax(c, np.float32(-1.0)), np.float32(1.0)).astype(np.float32)


def _all_small_by_fmax(mag):
    """max |pred| taken with fmax, which drops NaN, then compared"""
    return bool(np.fmax.reduce(mag, initial=np.float32(0.0)) < M.SMALL)


def test_value_scenes_see_the_nan_dropping_clip_and_branch():
    u, v, ut, vt, region = S.scene("values/special_inside")
    for b, (plane, val) in enumerate(S.SPECIALS):
        good = M.pair_metrics(u[b], v[b], ut[b], vt[b], region)
        bad = M.pair_metrics(u[b], v[b], ut[b], vt[b], region, clip=_clip_fmax_fmin)
        if not math.isfinite(val):
            assert math.isnan(good["aae"]) and math.isfinite(bad["aae"]), (b, plane, val)
            first = "mae_u" if plane == "u" else "mae_v"
            assert M.kind(good[first]) == ("nan" if math.isnan(val) else "+inf")
        elif abs(val) > 1:
            assert good["rmse"] == math.inf and good["epe"] == math.inf and math.isfinite(good["aae"])
            assert math.isfinite(good["mae_u"]) and math.isfinite(good["mae_v"])
        else:
            assert all(math.isfinite(x) for x in good.values())
    # outside the region nothing of it shows
    u, v, ut, vt, region = S.scene("values/special_outside")
    out = M.batch_metrics(u, v, ut, vt, region)
    assert np.isfinite(out).all()
    y0, y1, x0, x1 = region
    assert not np.isfinite(u).all() and np.isfinite(u[:, y0:y1, x0:x1]).all() and np.isfinite(v[:, y0:y1, x0:x1]).all()
    # the "nothing moves" branch
    u, v, ut, vt, region = S.scene("values/zero_truth")
    aae = [M.pair_metrics(u[b], v[b], 0.0, 0.0, region)["aae"] for b in range(6)]
    assert aae[0] == 0.0 and math.isnan(aae[1]) and aae[2] == 0.0 and aae[3] == 0.0
    assert 0 < aae[4] < 1e-3 or aae[4] == 0.0
    assert M.pair_metrics(u[1], v[1], 0.0, 0.0, region, all_small=_all_small_by_fmax, clip=_clip_fmax_fmin)["aae"] == 0.0
    assert M.pair_metrics(u[1], v[1], 0.0, 0.0, region, all_small=_all_small_by_fmax)["aae"] == 0.0
    # the threshold on the truth shows on the empty region only
    u, v, ut, vt, region = S.scene("values/truth_threshold_empty")
    aae = M.batch_metrics(u, v, ut, vt, region)[:, 4]
    assert aae[0] == 0.0 and math.isnan(aae[1]) and aae[2] == 0.0 and math.isnan(aae[3])
    assert float(ut[0]) < 1e-6 < float(ut[1]) and float(-vt[2]) < 1e-6 < float(-vt[3])
    # the clip itself
    u, v, ut, vt, region = S.scene("values/cosine_clip")
    c0 = M.pixel_terms(u[0].ravel(), v[0].ravel(), ut[0], vt[0], clip=lambda c: c)[4]
    c1 = M.pixel_terms(u[1].ravel(), v[1].ravel(), ut[1], vt[1], clip=lambda c: c)[4]
    assert (c0 == np.nextafter(np.float32(1), np.float32(2))).all() and (c1 == np.nextafter(np.float32(1), np.float32(0))).all()
    assert M.pair_metrics(u[0], v[0], ut[0], vt[0], region)["aae"] == 0.0
    assert math.isnan(M.pair_metrics(u[0], v[0], ut[0], vt[0], region, clip=lambda c: c)["aae"])
    assert M.pair_metrics(u[1], v[1], ut[1], vt[1], region)["aae"] == pytest.approx(0.0197823, rel=1e-5)


def test_zero_truth_pairs_at_the_float32_threshold():
    """|pred| one float32 step below 1e-6 everywhere keeps the branch; one pixel a step above, or at float32(1e-6) itself,
    leaves it (NumPy compares the float32 magnitudes with float32(1e-6)); the fixture says what the reference does"""
    rows = FIX["scenes"]["values/zero_truth"]["metrics"]
    u, v, ut, vt, region = S.scene("values/zero_truth")
    assert float(S.F32_BELOW) < float(S.F32_AT) < 1e-6 < float(S.F32_ABOVE)
    for b in range(6):
        got = M.pair_metrics(u[b], v[b], 0.0, 0.0, region)
        for k, ref in zip(M.KEYS, rows[b]):
            assert M.kind(got[k]) == M.kind(float(ref)), (b, k, got[k], ref)


@pytest.mark.parametrize("family", ("edges", "once", "values", "sizes", "noise"))
def test_host_drop_in_equals_the_fixture(family):
    """flow_metrics.compute_all_metrics is the same operations in the same library as the reference: equal where the running
    NumPy is the recorded one, within the bound otherwise"""
    import warnings

    import flow_metrics as F

    same_numpy = np.__version__ == FIX["numpy"]
    for name in S.SCENES:
        if S.FAMILY[name] != family:
            continue
        u, v, ut, vt, region = S.checked_scene(name, FIX)
        entry = FIX["scenes"][name]
        mask = np.zeros(u.shape[1:], bool)
        mask[region[0]:region[1], region[2]:region[3]] = True
        for row, b in zip(entry["metrics"], S.fixture_pairs(name, FIX)):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                got = F.compute_all_metrics(u[b], v[b], float(ut[b]), float(vt[b]), mask)
            for k, ref in zip(M.KEYS, row):
                if same_numpy:
                    assert got[k] == float(ref) or (math.isnan(got[k]) and math.isnan(float(ref))), (name, b, k, got[k], ref)
                else:
                    # both sides carry NumPy's error: each agrees with the model, so they lie within twice the bound
                    model = M.pair_metrics(u[b], v[b], ut[b], vt[b], region)[k]
                    assert M.agrees_with_reference(model, got[k] if math.isfinite(got[k]) else repr(got[k]), entry["n"], k,
                                                   TERM), (name, b, k, got[k], ref)
