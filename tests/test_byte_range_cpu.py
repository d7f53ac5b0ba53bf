"""The uint8 conversions at and beyond the byte range, on the statements alone (no GPU): mosaic_model.resolve's saturating rule
against a scalar form written another way, against the expression it replaces, and without any warning to hide; the scenes of
tests/byte_range_scenes.py where they claim to be; and the calls that keep a bare rint -- the warps, the interpolation and
the plain mosaic -- inside [0, 255] on frames of 0 and 255, which is what licenses that conversion."""
import math
import warnings

import numpy as np
import pytest

import byte_range_scenes as S
import mosaic_exposure_model as MEM
import mosaic_model as MM

BLENDS = list(MM.BLENDS.items())


@pytest.fixture(autouse=True)
def _warnings_are_errors():
    """every statement of this module's scenes is evaluated with no np.errstate around it and every warning an error"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        yield


def _scalar(v):
    """the rule on one float32 value after another: Python's round is half to even, and it refuses an infinity, so the value
    is held to [-1, 256] first -- that moves no result"""
    out = np.empty(v.shape, np.uint8)
    flat = out.reshape(-1)
    for i, x in enumerate(np.asarray(v, np.float32).reshape(-1)):
        x = float(x)
        flat[i] = 0 if math.isnan(x) else min(max(round(min(max(x, -1.0), 256.0)), 0), 255)
    return out


def _states():
    """(what, state) of every new mosaic scene"""
    for case in range(len(S.CASES)):
        (_, _), (Hc, Wc), (x0, y0), _, _ = S.CASES[case]
        for blend in ("last", "first"):
            fr, maps, ex, code, _ = S.ladder(case, blend)
            yield f"ladder {case} {blend}", S.state_of(fr, maps, None, ex, x0, y0, Hc, Wc, code)
        for dtype in (np.uint8, np.float32):
            fr, maps, skip, ex = S.wide(case, dtype)
            for blend, code in BLENDS:
                yield f"wide {case} {blend} {np.dtype(dtype).name}", S.state_of(fr, maps, skip, ex, x0, y0, Hc, Wc, code)
    for name, projective, extra in S.FLOAT_STATES:
        fr, maps, (x0, y0), (Hc, Wc) = S.float_state(name, projective, extra)
        for blend, code in BLENDS:
            yield f"float_state {name} {projective} +{extra} {blend}", S.state_of(fr, maps, None, None, x0, y0, Hc, Wc, code)


def test_resolve_equals_a_scalar_form_and_nothing_warns():
    """the new scenes' statements, with every warning an error and no errstate here: the cast never leaves uint8's domain"""
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for what, st in _states():
            v = S.value(st)
            got, cnt = MM.resolve(st, True)
            assert got.dtype == np.uint8 and np.array_equal(cnt, st["count"])
            assert np.array_equal(got, _scalar(v)), what
            assert not got[st["count"] == 0].any(), what
            n += 1
        pan = S.highlight_pan()
        MEM.composite(pan["frames"], pan["maps"], None, pan["exposure"], *pan["origin"], *pan["shape"], MM.FEATHER)
    assert n == 2 * (2 + 8) + 16


def test_the_ladder_holds_every_target_and_the_rule_s_value():
    for case in range(len(S.CASES)):
        (_, _), (Hc, Wc), (x0, y0), _, _ = S.CASES[case]
        outs = []
        for blend in ("last", "first"):
            fr, maps, ex, code, band = S.ladder(case, blend)
            st = S.state_of(fr, maps, None, ex, x0, y0, Hc, Wc, code)
            v, out = S.value(st), MM.resolve(st, True)[0]
            outs.append(out)
            assert ((band >= 0) == (st["count"] > 0)).all() and (band < 0).any()
            for k, (t, want) in enumerate(zip(S.TARGETS, S.RULE)):
                at = band == k
                assert at.sum() >= 8, f"case {case}: target {t} shows"
                assert (np.isnan(v[at]).all() if math.isnan(t) else (v[at] == np.float32(t)).all()), f"case {case}: {t} is planted exactly"
                assert (out[at] == want).all(), f"case {case} {blend}: {t} -> {want}, got {np.unique(out[at])}"
        assert np.array_equal(outs[0], outs[1]), "first on the reversed order is last"
        # the bands of 255.5 and 300 lie across two lanes' four pixels; a band of the upper strip fills a lane
        rows = np.nonzero((band == S.TARGETS.index(255.5)).any(1))[0]
        for t in (255.5, 300.0):
            cols = np.nonzero(band[rows[0]] == S.TARGETS.index(t))[0]
            assert len(cols) == 4 and cols[0] % 4 == 2
        cols = np.nonzero(band[0] == S.TARGETS.index(-300.0))[0]
        assert len(cols) == 4 and cols[0] % 4 == 0


def test_the_rule_differs_from_the_bare_cast_exactly_outside_the_byte_range():
    """np.rint(v).astype(np.uint8), the expression that resolve held before, wraps: -300 -> 212, -1 -> 255, 255.5 -> 0,
    300 -> 44.  It agrees with the rule on [-0.5, 255.5) and differs at every finite target outside -- but for the two whose
    wrapped value happens to be the saturated one: -256.5 rounds to -256 = 0 mod 256, and 65535 = 255 mod 256.  NaN, the
    infinities and +-1e30 are left out: the cast is not defined for them"""
    (_, _), (Hc, Wc), (x0, y0), _, _ = S.CASES[0]
    fr, maps, ex, code, band = S.ladder(0, "last")
    st = S.state_of(fr, maps, None, ex, x0, y0, Hc, Wc, code)
    v, new = S.value(st), MM.resolve(st, True)[0]
    same, differ = [], []
    for k, t in enumerate(S.TARGETS):
        if not math.isfinite(t) or abs(t) > 1e6:
            continue
        at = band == k
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            old = np.rint(v[at]).astype(np.uint8)
        assert (old == old[0]).all()
        (same if (old == new[at]).all() else differ).append(t)
        assert (old == new[at]).all() or (old != new[at]).all()
    inside = [t for t in S.TARGETS if -0.5 <= t < 255.5]
    assert same == sorted(inside + [-256.5, 65535.0]), same
    assert differ == [-300.0, -1.0, 255.5, 256.0, 300.0, 511.5, 512.0], differ


def test_the_scenes_go_where_they_claim():
    for case in range(len(S.CASES)):
        (_, _), (Hc, Wc), (x0, y0), _, _ = S.CASES[case]
        fr, maps, skip, ex = S.wide(case)
        assert fr.min() <= 1 and fr.max() >= 254 and 0.6 <= ex[:, 0].min() and ex[:, 0].max() <= 1.5 and np.abs(ex[:, 1]).max() <= 40
        for blend in (MM.MEAN, MM.FEATHER):
            st = S.state_of(fr, maps, skip, ex, x0, y0, Hc, Wc, blend)
            v, cov = S.value(st), st["count"] > 0
            assert st["count"].max() >= 3 and not cov.all()
            hi, lo = (v[cov] > 255.5).mean(), (v[cov] < -0.5).mean()
            assert hi >= 0.05 and lo >= 0.05, f"wide {case} blend {blend}: {hi:.3f} above, {lo:.3f} below"
    pan = S.highlight_pan()
    assert (pan["exposure"][:-1, 0] > 1).all() and (pan["exposure"][-1] == [1.0, 0.0]).all()
    assert abs((pan["truth"] > 255.5).mean() - 0.011) < 0.004, "about 1.1 % of the source exceeds 255.5 at the anchor's exposure"
    for blend in (MM.MEAN, MM.FEATHER):
        st = S.state_of(pan["frames"], pan["maps"], None, pan["exposure"], *pan["origin"], *pan["shape"], blend)
        assert (st["count"] > 0).all()
        assert (S.value(st) > 255.5).sum() >= 100
    for name, projective, extra in S.FLOAT_STATES:
        fr, maps, (x0, y0), (Hc, Wc) = S.float_state(name, projective, extra)
        assert fr.dtype == np.float32 and (Wc % 4 == 0) == (extra == 2)
        v = S.value(S.state_of(fr, maps, None, None, x0, y0, Hc, Wc, MM.MEAN))
        assert (v > 255.5).mean() > 0.2 if name == "u16" else (v < -0.5).any() and (v > 0.5).any()


def _in_range(values, what):
    for p, v in enumerate(values):
        assert v.dtype == np.float32, what
        assert np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 255.0, f"{what} plane {p}: [{v.min()}, {v.max()}]"


def _rint(v):
    return np.rint(v).astype(np.uint8)


@pytest.mark.parametrize("name", S.EXTREMES)
def test_the_warps_of_the_extremes_stay_in_range(name):
    """the float32 value that a warp's statement forms before its conversion lies in [0, 255] on frames of 0 and 255, and its
    rint is the statement's byte; NV12 chroma outside the frame is 128"""
    import nv12_model as NM

    outside = 0
    for what, layout, arg, frames, maps in S.warp_cells(name):
        values = S.warp_values(layout, arg, frames, maps)
        _in_range(values, what)
        want = S.warp_statement(layout, arg, frames, maps)
        if layout == "planar":
            assert np.array_equal(_rint(values[0]), want), what
        elif layout == "packed":
            assert np.array_equal(np.stack([_rint(v) for v in values], -1), want), what
        else:
            y, uv = NM.planes(want)
            assert np.array_equal(_rint(values[0]), y) and np.array_equal(np.stack([_rint(v) for v in values[1:]], -1), uv), what
            for c in range(2):
                _, ins = S._planar(maps)(np.ascontiguousarray(NM.planes(frames)[1][..., c]), NM.chroma_maps(maps, arg))
                assert (uv[..., c][ins == 0] == 128).all(), f"{what}: chroma outside is 128"
                outside += int((ins == 0).sum())
    assert outside > 0


@pytest.mark.parametrize("name", S.EXTREMES)
def test_the_interpolation_of_the_extremes_stays_in_range(name):
    import nv12_model as NM

    for what, layout, arg, frames, flows, taus in S.interp_cells(name):
        values = S.interp_values(layout, arg, frames, flows, taus)
        _in_range(values, what)
        want = S.interp_statement(layout, arg, frames, flows, taus)
        if layout == "planar":
            assert np.array_equal(_rint(values[0]), want), what
        elif layout == "packed":
            assert np.array_equal(np.stack([_rint(v) for v in values], -1), want), what
        else:
            H = flows[0].shape[1]
            y, uv = NM.planes(want[0])
            assert want.shape[0] == 1 and np.array_equal(_rint(values[0][0]), y) and np.array_equal(_rint(values[1]), uv), what
            assert y.shape[1] == H


@pytest.mark.parametrize("name", S.EXTREMES)
def test_the_plain_mosaic_of_the_extremes_stays_in_range(name):
    for what, frames, maps, skip, x0, y0, Hc, Wc in S.mosaic_cells(name):
        for blend, code in BLENDS:
            v, cnt = MM.composite(frames.astype(np.float32), maps, skip, x0, y0, Hc, Wc, code)
            _in_range([v], f"{what} {blend}")
            want = MM.composite(frames, maps, skip, x0, y0, Hc, Wc, code)
            assert np.array_equal(_rint(v), want[0]) and np.array_equal(cnt, want[1]) and cnt.max() >= 3, f"{what} {blend}"
            if name == "full":
                assert (want[0][cnt > 0] == 255).all()
            if name == "zeros":
                assert not want[0].any()
