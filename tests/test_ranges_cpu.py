"""The CPU oracle on frames outside the 8-bit value range (tests/range_scenes.py) against the reference's own values
(tests/golden/reference_ranges.npz, make_golden_ranges.py): every stage, the flows, the residual means and the iteration
counts, under range_scenes.same (NaN positions equal, other values equal as values).  Also: every scene reaches the path
it was built for, and the statements of tests/fb_model.py and tests/track_model.py evaluate NaN-bearing flows."""
import json

import numpy as np
import pytest
from scipy.ndimage import map_coordinates

import range_scenes as S

CFGS = [(3, 5, 3), (2, 7, 2), (1, 5, 1), (4, 5, 3), (3, 5, 2), (1, 5, 2)]
ENVELOPE = [(3, 5, 3), (3, 5, 2), (1, 5, 1), (1, 5, 2)]


@pytest.fixture(autouse=True)
def _quiet_fp():
    """these scenes overflow, underflow and make NaN on purpose: NumPy's warnings off for this module's tests only"""
    with np.errstate(all="ignore"):
        yield


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(golden_dir / "reference_ranges.npz")
    return z, json.loads(str(z["meta"][0]))


def _pin(meta, key, a):
    a = np.asarray(a, np.float32)
    m = meta[key]
    assert list(a.shape) == m["shape"], key
    assert S.digest(a) == m["sha256"], f"{key}: nan {int(np.isnan(a).sum())} vs {m['nan']}, nonzero {np.count_nonzero(a)} vs {m['nonzero']}"


def test_fixture_records_its_versions(fx):
    _, meta = fx
    assert meta["numpy"] and meta["scipy"]
    assert meta["single"] == [3, 5, 7, 13] and meta["pyramidal"] == [list(c) for c in CFGS]


def test_the_rule_reads_nan_positions_and_signed_zero():
    a = np.array([np.nan, -0.0, 1.0], np.float32)
    assert S.same(a, np.array([np.nan, 0.0, 1.0], np.float32))
    assert not S.same(a, np.array([0.0, 0.0, 1.0], np.float32))
    assert not S.same(a, np.array([np.nan, 0.0, np.nan], np.float32))
    assert S.digest(a) == S.digest(np.array([-np.float32(np.nan), 0.0, 1.0], np.float32))


@pytest.mark.parametrize("name", S.SCENES)
def test_oracle_stages_equal_the_reference(oracle, fx, name):
    _, meta = fx
    p, c = S.scene(name)
    _pin(meta, f"{name}/tm/prev", p)
    _pin(meta, f"{name}/tm/curr", c)
    for nm, a in zip(("Ix", "Iy", "It"), oracle.compute_gradients(p, c)):
        _pin(meta, f"{name}/tm/grad/{nm}", a)
    for l, a in enumerate(oracle.build_gaussian_pyramid(p, 3)):
        _pin(meta, f"{name}/tm/pyr/{l}", a)
    _pin(meta, f"{name}/tm/warp", oracle.warp_image(c, *S.special_flow(*p.shape)))


def test_oracle_upsamples_non_finite_flows_as_the_reference(oracle, fx):
    _, meta = fx
    for h, w, seed in ((24, 32, 1), (23, 31, 2)):
        fu, fv = S.coarse_flow(h, w, seed), S.coarse_flow(h, w, seed + 10)
        for H, W in ((48, 64), (45, 61), (96, 128)):
            uu, uv = oracle.upsample_flow(fu, fv, (H, W))
            _pin(meta, f"upsample/{h}x{w}/{H}x{W}/u", uu)
            _pin(meta, f"upsample/{h}x{w}/{H}x{W}/v", uv)


@pytest.mark.parametrize("name", S.SCENES)
@pytest.mark.parametrize("base", list(S.BASES))
def test_oracle_flows_equal_the_reference(oracle, fx, name, base):
    z, meta = fx
    p, c = S.scene(name, base)
    full = base == "tm"
    for win in ((3, 5, 7, 13) if full else (5,)):
        u, v = oracle.lucas_kanade_single_scale(p, c, win)
        _pin(meta, f"{name}/{base}/single/{win}/u", u)
        _pin(meta, f"{name}/{base}/single/{win}/v", v)
    for cfg in (CFGS if full else ENVELOPE):
        ck = f"{name}/{base}/pyr_{cfg[0]}_{cfg[1]}_{cfg[2]}"
        u, v, log, runs = oracle.lucas_kanade_pyramidal_ex(p, c, *cfg)
        _pin(meta, f"{ck}/u", u)
        _pin(meta, f"{ck}/v", v)
        assert list(runs) == list(z[f"{ck}/runs"]), ck
        S.assert_same(log, z[f"{ck}/log"], f"{ck} residual means")
        if f"{ck}/u" in z.files:
            S.assert_same(u, z[f"{ck}/u"], ck)
            S.assert_same(v, z[f"{ck}/v"], ck)


def _window_sums(a, hw):
    """float64 sums over every full (2hw+1)^2 window, at the window centres"""
    k = 2 * hw + 1
    c = np.cumsum(np.cumsum(np.pad(a.astype(np.float64), ((1, 0), (1, 0))), 0), 1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def _window_max(a, hw):
    from numpy.lib.stride_tricks import sliding_window_view
    return sliding_window_view(a, (2 * hw + 1, 2 * hw + 1)).max(axis=(2, 3))


def test_every_scene_reaches_its_path(oracle, fx):
    z, meta = fx
    # unit: the |det| > 1e-4 cut-off decides many windows
    p, c = S.scene("unit")
    Ix, Iy, _ = (a.astype(np.float64) for a in oracle.compute_gradients(p, c))
    det = np.abs(_window_sums(Ix * Ix, 2) * _window_sums(Iy * Iy, 2) - _window_sums(Ix * Iy, 2) ** 2)
    assert np.count_nonzero((det > 1e-4) & (det < 1e-3)) >= 200
    assert np.count_nonzero(det <= 1e-4) >= 200
    # signed: negative pixels, through every pyramid level
    p, c = S.scene("signed")
    assert all((lv < 0).any() for lv in oracle.build_gaussian_pyramid(p, 3))
    # u16: whole streaming tiles (64 x 24, with the R rows and columns of windows that reach into them) in which every
    # window keeps Sxx, Syy < 2^16 and some pixel is above 255: the [0, 255] test alone sends them to the exact redo
    for base in S.BASES:
        p, c = S.scene("u16", base)
        assert p.max() <= 65535 and (p == np.round(p)).all() and (c == np.round(c)).all()
        Ix, Iy, _ = oracle.compute_gradients(p, c)
        H, W = p.shape
        for hw in (2, 3):
            R = hw + 1
            bound = np.zeros((H, W), bool)   # the centre of a window that fails the bound
            bound[hw:H - hw, hw:W - hw] = (_window_sums(Ix.astype(np.float64) ** 2, hw) >= 65536) | \
                                          (_window_sums(Iy.astype(np.float64) ** 2, hw) >= 65536)
            over = np.maximum(p, c) > 255
            clean = 0
            for ty in range(0, H, 24):
                for tx in range(0, W, 64):
                    ys, xs = slice(max(ty - R, 0), min(ty + 24 + R, H)), slice(max(tx - R, 0), min(tx + 64 + R, W))
                    if not bound[ys, xs].any() and over[ys, xs].any():
                        clean += 1
            assert clean >= 1, (base, hw)
        u, _ = oracle.lucas_kanade_single_scale(p, c, 5)
        assert np.count_nonzero(u[:24]) > 0.5 * u[:24].size
    # big: finite frames, NaN flows (single-scale); NaN residual means and warps with NaN flows (pyramidal)
    p, c = S.scene("big")
    assert np.isfinite(p).all() and np.isfinite(c).all()
    assert meta["big/tm/single/5/u"]["nan"] > 0
    assert np.isnan(z["big/tm/pyr_3_5_3/log"]).all() and list(z["big/tm/pyr_3_5_3/runs"]) == [3, 3, 3]
    # steep: finite frames, det finite while a numerator overflows: +inf in u with no NaN beside it, so the reference's
    # single-scale mean |du| is +inf (no NaN flows where the inf is)
    assert meta["steep/tm/single/5/u"]["nan"] == 0
    z_log = z["steep/tm/pyr_1_5_1/log"]
    assert np.isposinf(z_log[0, 0, 0]) and np.isfinite(z_log[0, 0, 1])
    # huge: p + q and the products overflow; zero and NaN flows
    p, c = S.scene("huge")
    Ix, _, _ = oracle.compute_gradients(p, c)
    assert np.isinf(p + c).any() and np.isinf(Ix * Ix).any()
    assert meta["huge/tm/single/3/u"]["nan"] > 0 and meta["huge/tm/single/5/u"]["nonzero"] == 0
    # tiny: subnormal pixels and non-zero gradients
    p, c = S.scene("tiny")
    Ix, Iy, It = oracle.compute_gradients(p, c)
    tiny = np.finfo(np.float32).tiny
    assert (p[p != 0] < tiny).all() and (p != 0).mean() > 0.9
    assert np.count_nonzero(Ix) > 1000 and np.count_nonzero(It) > 1000
    # small: normal pixels whose products underflow
    p, c = S.scene("small")
    Ix, Iy, _ = oracle.compute_gradients(p, c)
    assert (p[p != 0] >= tiny).all()
    prod = Ix * Iy
    assert np.count_nonzero((Ix != 0) & (Iy != 0) & (np.abs(prod) < tiny)) > 1000
    # holes: non-finite pixels inside, on row 0, on the last row and in the last two columns; a NaN in column W-2
    # reaches a sample that lands on column W-1, where its tap carries weight 0
    p, c = S.scene("holes")
    H, W = p.shape
    for f in (p, c):
        bad = ~np.isfinite(f)
        assert bad[0].any() and bad[-1].any() and bad[1:-1, 1:-3].any() and bad[:, -2].any() and bad[:, -1].any()
    zero = np.zeros_like(c)
    w = oracle.warp_image(c, zero, zero)
    rows = np.flatnonzero(~np.isfinite(c[:, W - 2]))   # inf * 0 is NaN too
    assert len(rows) and np.isnan(w[rows, W - 1]).all()


def _scipy_warp(img, u, v):
    H, W = img.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return map_coordinates(img, [yy + v, xx + u], order=1, mode="constant", cval=0.0).astype(np.float32)


def test_oracle_warp_reads_non_finite_coordinates_as_outside(oracle):
    """NaN, +-inf and +-1e30 coordinates sample cval, as SciPy's map_coordinates (the oracle's cast was undefined)"""
    p, c = S.scene("holes")
    u, v = S.special_flow(*p.shape)
    S.assert_same(oracle.warp_image(c, u, v), _scipy_warp(c, u, v), "warp")
    bu, bv = oracle.lucas_kanade_single_scale(*S.scene("big"), 5)
    assert np.isnan(bu).any()
    S.assert_same(oracle.warp_image(p, bu, bv), _scipy_warp(p, bu, bv), "warp with NaN flows")


def test_fb_and_track_statements_evaluate_nan_flows(oracle):
    import fb_model
    import track_model

    p, c = S.scene("big")
    uf, vf = oracle.lucas_kanade_single_scale(p, c, 5)
    ub, vb = oracle.lucas_kanade_single_scale(c, p, 5)
    nan_f = np.isnan(uf) | np.isnan(vf)
    assert nan_f.any()
    err_f, err_b, valid_f, valid_b = fb_model.fb_check(uf, vf, ub, vb)
    assert not valid_f[nan_f].any() and np.isnan(err_f[nan_f]).all()
    # the warp inside the statement is SciPy's at every pixel, NaN coordinates included
    S.assert_same(fb_model.O.warp_image(ub, uf, vf), _scipy_warp(ub, uf, vf), "fb warp")
    H, W = p.shape
    ys, xs = np.nonzero(nan_f)
    q = np.array([[xs[0], ys[0]], [W / 2 + 0.25, H / 2 + 0.5], [3.0, 4.0]], np.float32)
    tr, vis = track_model.track(uf[None], vf[None], ub[None], vb[None], None, q)
    assert vis[0].all() and not vis[1, 0]          # a query on a NaN flow stops there
    assert np.isnan(tr[1][~vis[1].astype(bool)]).all() and np.isfinite(tr[1][vis[1].astype(bool)]).all()
