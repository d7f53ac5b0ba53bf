"""The HIP paths on frames outside the 8-bit value range (tests/range_scenes.py): normalised, signed, 16-bit, huge,
subnormal, underflowing and NaN / inf-holed frames.  Every output is held to the reference's values
(tests/golden/reference_ranges.npz) and, where the fixture does not record it, to the CPU oracle, under
range_scenes.same (NaN positions equal, other values equal as values)."""
import json

import numpy as np
import pytest

import range_scenes as S

pytestmark = pytest.mark.gpu
CFGS = [(3, 5, 3), (2, 7, 2), (1, 5, 1), (4, 5, 3), (3, 5, 2), (1, 5, 2)]
ENVELOPE = [(3, 5, 3), (3, 5, 2), (1, 5, 1), (1, 5, 2)]   # the tolerant mode's cells (recorded on every crop)


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
    assert list(a.shape) == m["shape"] and S.digest(a) == m["sha256"], \
        f"{key}: nan {int(np.isnan(a).sum())} vs {m['nan']}, nonzero {np.count_nonzero(a)} vs {m['nonzero']}"


def _log_matches(log, ref, shape, what):
    """the residual log against the reference's means (include/oflk.h oflk_plan_read_log): NaN and +inf exactly where
    the reference's mean is NaN / +inf; a finite mean within the library's own bound of the reference's --
    oflk_device_mean_error of the kernel path (the worse of the tile and streaming sums) plus NumPy's summation error
    (the OFLK_SUM_HOST bound), both relative to the mean -- or, where a block's finite |d| sum passed 2^28 px and was
    clamped, below the reference's and at least 2^28 / (h * w)"""
    import _oflk
    import lucas_kanade_pyramidal as P

    L = _oflk.lib()
    log, ref = np.asarray(log, np.float32), np.asarray(ref, np.float32)
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(kind(log), kind(ref)), f"{what}: {kind.__name__} at {np.argwhere(kind(log) != kind(ref))[:4]}"
    for l, (h, w) in enumerate(P.pyramid_level_shapes(shape, ref.shape[0])):
        for k in range(ref.shape[1]):
            for c in range(2):
                d, r = float(log[l, k, c]), float(ref[l, k, c])
                if not np.isfinite(r) or r == 0.0:
                    assert d == r or (np.isnan(d) and np.isnan(r)), (what, l, k, c, d, r)
                    continue
                e = max(L.oflk_device_mean_error(p, h, w, r) for p in (0, 1)) + L.oflk_device_mean_error(2, h, w, r)
                if abs(d - r) <= e * r:
                    continue
                assert 2.0 ** 28 / (h * w) * (1 - 1e-6) <= d < r, f"{what}: level {l} iteration {k}: {d} vs {r} (bound {e:.2e})"


def _dev(*arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in arrs]


def _plan_run(p, c, levels, win, iters, kernels=None, arith=None, single=False):
    """(u, v[, log, runs]) of one pair through oflk_plan_*"""
    import torch

    import _oflk

    H, W = p.shape
    tp, tc = _dev(p[None], c[None])
    tu, tv = torch.empty_like(tp), torch.empty_like(tp)
    st = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, 1, H, W, levels, win, iters)
    try:
        if kernels is not None:
            plan.set_kernels(kernels)
        if arith is not None:
            plan.set_arithmetic(arith)
        if single:
            plan.single_scale(tp.data_ptr(), tc.data_ptr(), tu.data_ptr(), tv.data_ptr(), st)
            torch.cuda.synchronize()
            return tu.cpu().numpy()[0], tv.cpu().numpy()[0]
        plan.pyramidal(tp.data_ptr(), tc.data_ptr(), tu.data_ptr(), tv.data_ptr(), st)
        torch.cuda.synchronize()
        log, runs = plan.read_log(st)
        return tu.cpu().numpy()[0], tv.cpu().numpy()[0], np.asarray(log)[0], np.asarray(runs)[0]
    finally:
        plan.close()


@pytest.mark.parametrize("name", S.SCENES)
def test_stage_entry_points_equal_the_reference(fx, name):
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    _, meta = fx
    p, c = S.scene(name)
    for nm, a in zip(("Ix", "Iy", "It"), K.compute_gradients(p, c)):   # huge, holes: 0 * inf on the zero taps is NaN
        _pin(meta, f"{name}/tm/grad/{nm}", a)
    for l, a in enumerate(P.build_gaussian_pyramid(p, 3)):
        _pin(meta, f"{name}/tm/pyr/{l}", a)
    _pin(meta, f"{name}/tm/warp", P.warp_image(c, *S.special_flow(*p.shape)))


def test_upsample_of_non_finite_flows_equals_the_reference(fx):
    import lucas_kanade_pyramidal as P

    _, meta = fx
    for h, w, seed in ((24, 32, 1), (23, 31, 2)):
        fu, fv = S.coarse_flow(h, w, seed), S.coarse_flow(h, w, seed + 10)
        for H, W in ((48, 64), (45, 61), (96, 128)):
            uu, uv = P.upsample_flow(fu, fv, (H, W))
            _pin(meta, f"upsample/{h}x{w}/{H}x{W}/u", uu)
            _pin(meta, f"upsample/{h}x{w}/{H}x{W}/v", uv)


@pytest.mark.parametrize("name", S.SCENES)
@pytest.mark.parametrize("base", list(S.BASES))
@pytest.mark.parametrize("win", [5, 7])
@pytest.mark.parametrize("kernels", [0, 1, 2])
def test_single_scale_plan_under_every_kernel_choice(oracle, fx, name, base, win, kernels):
    """oflk_plan_single_scale with set_kernels 0 (auto), 1 (tile), 2 (streaming, forced)"""
    _, meta = fx
    p, c = S.scene(name, base)
    u, v = _plan_run(p, c, 1, win, 1, kernels=kernels, single=True)
    if f"{name}/{base}/single/{win}/u" in meta:
        _pin(meta, f"{name}/{base}/single/{win}/u", u)
        _pin(meta, f"{name}/{base}/single/{win}/v", v)
    ou, ov = oracle.lucas_kanade_single_scale(p, c, win)
    S.assert_same(u, ou, f"{name}/{base} {win}x{win} kernels {kernels} u")
    S.assert_same(v, ov, f"{name}/{base} {win}x{win} kernels {kernels} v")


@pytest.mark.parametrize("name", S.SCENES)
def test_single_scale_host_entry_every_window(fx, name):
    """the float32 host entry point at windows 3, 5, 7 (fused kernels) and 13 (the generic window)"""
    import lucas_kanade_core as K

    _, meta = fx
    p, c = S.scene(name)
    for win in (3, 5, 7, 13):
        u, v = K.lucas_kanade_single_scale(p, c, win)
        _pin(meta, f"{name}/tm/single/{win}/u", u)
        _pin(meta, f"{name}/tm/single/{win}/v", v)


@pytest.mark.parametrize("name", S.SCENES)
@pytest.mark.parametrize("base", list(S.BASES))
def test_pyramidal_host_and_plan_equal_the_reference(fx, name, base):
    """flows, every residual mean (NaN where the reference's is NaN) and the iterations run per level"""
    import lucas_kanade_pyramidal as P

    z, meta = fx
    p, c = S.scene(name, base)
    for cfg in (CFGS if base == "tm" else ENVELOPE):
        ck = f"{name}/{base}/pyr_{cfg[0]}_{cfg[1]}_{cfg[2]}"
        u, v, log, runs = P.lucas_kanade_pyramidal_with_log(p, c, *cfg)
        _pin(meta, f"{ck}/u", u)
        _pin(meta, f"{ck}/v", v)
        assert list(runs) == list(z[f"{ck}/runs"]), (ck, runs)
        _log_matches(log, z[f"{ck}/log"], p.shape, f"{ck} residual log")
        pu, pv, plog, pruns = _plan_run(p, c, *cfg)
        S.assert_same(pu, u, ck)
        S.assert_same(pv, v, ck)
        _log_matches(plog, z[f"{ck}/log"], p.shape, f"{ck} plan log")
        assert list(pruns) == list(runs)


@pytest.mark.parametrize("name", ["unit", "big"])
def test_printed_log_equals_the_reference_stdout(fx, name, capsys, monkeypatch):
    """the check of test_gpu_round2.test_printed_log_equals_the_reference_stdout on the new stdout fixtures (a NaN mean
    prints as the reference's "nan")"""
    import lucas_kanade_pyramidal as P

    _, meta = fx
    p, c = S.scene(name)
    monkeypatch.setenv("OFLK_QUIET", "0")
    capsys.readouterr()
    P.lucas_kanade_pyramidal(p, c, 3, 5, 3)
    assert capsys.readouterr().out == meta["stdout"][name]


def _big_sequence():
    p, c = S.scene("big")
    q = np.ascontiguousarray(np.roll(c, (1, -2), axis=(0, 1)))
    return np.stack([p, c, q])


def test_big_sequence_equals_the_pair_batch_and_its_reverse():
    import torch

    import _oflk
    import lucas_kanade_pyramidal as P

    fr = _big_sequence()
    T, H, W = fr.shape
    u, v, log, runs = P.lucas_kanade_pyramidal_sequence_with_log(fr)
    assert np.isnan(u).any() and np.isnan(log).any()
    tp, tc = _dev(fr[:-1], fr[1:])
    tu, tv = torch.empty_like(tp), torch.empty_like(tp)
    st = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, T - 1, H, W, 3, 5, 3)
    try:
        plan.pyramidal(tp.data_ptr(), tc.data_ptr(), tu.data_ptr(), tv.data_ptr(), st)
        torch.cuda.synchronize()
        blog, bruns = plan.read_log(st)
    finally:
        plan.close()
    S.assert_same(u, tu.cpu().numpy(), "sequence u vs pair batch")
    S.assert_same(v, tv.cpu().numpy(), "sequence v vs pair batch")
    S.assert_same(log, blog, "sequence log vs pair batch")
    assert np.array_equal(runs, bruns)
    fb = P.lucas_kanade_pyramidal_sequence_fb(fr)
    S.assert_same(fb.u_fwd, u, "fb forward")
    ru, rv = P.lucas_kanade_pyramidal_sequence(fr[::-1].copy())
    S.assert_same(fb.u_bwd, ru[::-1], "fb backward u vs reversed sequence")
    S.assert_same(fb.v_bwd, rv[::-1], "fb backward v vs reversed sequence")


def test_fb_and_tracks_on_nan_flows_equal_their_statements():
    import fb_model
    import lucas_kanade_pyramidal as P
    import track_model

    fr = _big_sequence()
    T, H, W = fr.shape
    fb = P.lucas_kanade_pyramidal_sequence_fb(fr)
    assert np.isnan(fb.u_fwd).any()
    ef, eb, vf, vb = fb_model.fb_check(fb.u_fwd, fb.v_fwd, fb.u_bwd, fb.v_bwd)
    S.assert_same(fb.err_fwd, ef, "err_fwd")
    S.assert_same(fb.err_bwd, eb, "err_bwd")
    assert np.array_equal(fb.valid_fwd, vf.astype(bool)) and np.array_equal(fb.valid_bwd, vb.astype(bool))
    rng = np.random.default_rng(5)
    q = np.stack([rng.uniform(0, W - 1, 300), rng.uniform(0, H - 1, 300)], 1).astype(np.float32)
    ys, xs = np.nonzero(np.isnan(fb.u_fwd[0]))
    q[:len(ys[:40])] = np.stack([xs[:40], ys[:40]], 1)    # queries on NaN flow vectors
    tr = P.lucas_kanade_pyramidal_sequence_tracks(fr, q)
    mt, mv = track_model.track(fb.u_fwd, fb.v_fwd, fb.u_bwd, fb.v_bwd, None, q)
    assert np.array_equal(tr.visible, mv.astype(bool))
    S.assert_same(tr.tracks, mt, "tracks")


@pytest.mark.parametrize("name", S.SCENES)
@pytest.mark.parametrize("base", list(S.BASES))
@pytest.mark.parametrize("cfg", [(3, 5, 3), (3, 5, 2), (1, 5, 1), (1, 5, 2), (2, 7, 2)])
def test_tolerant_plan_equals_its_model(name, base, cfg):
    """OFLK_ARITH_TOLERANT equals oracle/oflk_tolerant_model.c bit for bit (inside the envelope and outside it)"""
    import oflk_tolerant_model as M

    p, c = S.scene(name, base)
    L, win, K = cfg
    u, v, log, runs = _plan_run(p, c, L, win, K, arith=2)
    mu, mv, mlog, mruns = M.pyramidal(p, c, M.tolerant_spec(L, K, p.shape, win), win)
    S.assert_same(u, mu, f"{name}/{base} {cfg} u")
    S.assert_same(v, mv, f"{name}/{base} {cfg} v")
    assert list(runs) == list(mruns)


# u16 is outside the tolerant mode's promise (include/oflk.h OFLK_ARITH_TOLERANT: frames with |pixel| <= 255); its
# measured EPE is in DESIGN.md section 2, and test_tolerant_plan_equals_its_model still holds it bit for bit to the model
@pytest.mark.parametrize("name", [s for s in S.SCENES if s not in ("big", "steep", "huge", "u16")])
@pytest.mark.parametrize("base", list(S.BASES))
@pytest.mark.parametrize("cfg", ENVELOPE)
def test_tolerant_mode_keeps_its_bar_on_finite_scenes(oracle, fx, name, base, cfg):
    """inside the envelope: mean EPE against the reference's flow at most TOL / 3 (TOL = 1e-4 px) and the reference's
    iteration counts"""
    z, meta = fx
    p, c = S.scene(name, base)
    u, v, _, runs = _plan_run(p, c, *cfg, arith=2)
    ck = f"{name}/{base}/pyr_{cfg[0]}_{cfg[1]}_{cfg[2]}"
    if f"{ck}/u" in z.files:
        ru, rv = z[f"{ck}/u"], z[f"{ck}/v"]
    else:   # the oracle's flow, pinned here to the reference's digest (every crop records the four cells)
        ru, rv, _, _ = oracle.lucas_kanade_pyramidal_ex(p, c, *cfg)
    _pin(meta, f"{ck}/u", ru)
    _pin(meta, f"{ck}/v", rv)
    assert np.isfinite(ru).all() and np.isfinite(rv).all()
    assert list(runs) == list(z[f"{ck}/runs"])
    epe = float(np.mean(np.hypot(u.astype(np.float64) - ru, v.astype(np.float64) - rv)))
    assert epe <= 1e-4 / 3, f"{ck}: mean EPE {epe:.3e}"
