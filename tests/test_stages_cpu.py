"""CPU tests of the stage cases (tests/stage_scenes.py): no GPU is used.

1. The statement.  upsample_flow and build_gaussian_pyramid are written out below with the library calls of their definition
   (scipy.ndimage.gaussian_filter with sigma = 1 / scale_factor, int(h * scale_factor), np.linspace,
   map_coordinates(order=1, mode="constant"), the float32 multiply by target / coarse), and the oracle
   (oracle/oflk_oracle.c) equals them on EVERY case of both lists: NaN at the same positions, every other element the same
   32 bits.  tests/test_gpu_stages.py holds the kernels to the oracle on the same cases, so this is the link from there to
   SciPy.  If it breaks, SciPy is right and the oracle is mended.
2. The lists do what they were built for, asked of the library's own decisions (oflk_upsample_staged,
   oflk_pyramid_step_fused): both kernels of each stage occur, the tile capacities are met exactly and exceeded by one on
   each axis.  Were the capacity that the predicate uses off by one against the staged tile, these tests fail.
3. The two predicates against the span arithmetic restated in stage_scenes.max_span.
4. Frames of 2^23 rows or columns or more are refused before any device call (the kernels' signed 24-bit row products).
"""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter, map_coordinates

import stage_scenes as S


@pytest.fixture(scope="module")
def L():
    import _oflk

    return _oflk.lib()


# ---- 1. the statement -----------------------------------------------------------------------------------------------------------
def scipy_upsample_flow(u, v, target_shape):
    hc, wc = u.shape
    ht, wt = target_shape
    yy, xx = np.meshgrid(np.linspace(0, hc - 1, ht), np.linspace(0, wc - 1, wt), indexing="ij")
    uu = map_coordinates(u, [yy, xx], order=1, mode="constant")
    vv = map_coordinates(v, [yy, xx], order=1, mode="constant")
    assert uu.dtype == np.float32 and vv.dtype == np.float32
    # a float32 array times a Python float: NumPy multiplies in float32, by the float32 of the ratio
    uu, vv = uu * (wt / wc), vv * (ht / hc)
    assert uu.dtype == np.float32 and vv.dtype == np.float32
    return uu, vv


def scipy_pyramid(image, levels, scale_factor):
    out = [image.copy()]
    for _ in range(levels - 1):
        blurred = gaussian_filter(out[0], sigma=1.0 / scale_factor)
        h, w = blurred.shape
        nh, nw = int(h * scale_factor), int(w * scale_factor)
        yy, xx = np.meshgrid(np.linspace(0, h - 1, nh), np.linspace(0, w - 1, nw), indexing="ij")
        out.insert(0, map_coordinates(blurred, [yy, xx], order=1, mode="constant"))
    return out


def _uid(i):
    c, t = S.UPSAMPLE_CASES[i]
    return f"{c[0]}x{c[1]}-{t[0]}x{t[1]}"


def _pid(i):
    (h, w), lv, sf = S.PYRAMID_CASES[i]
    return f"{h}x{w}-L{lv}-{sf:.6g}"


@pytest.mark.parametrize("i", range(len(S.UPSAMPLE_CASES)), ids=_uid)
def test_oracle_upsample_equals_scipy(oracle, i):
    cshape, tshape = S.UPSAMPLE_CASES[i]
    u, v = S.flow_fields(cshape, i)
    (ou, ov), (su, sv) = oracle.upsample_flow(u, v, tshape), scipy_upsample_flow(u, v, tshape)
    S.same_bits(ou, su, f"upsample {cshape} -> {tshape}, u")
    S.same_bits(ov, sv, f"upsample {cshape} -> {tshape}, v")


@pytest.mark.parametrize("i", S.UPSAMPLE_NONFINITE, ids=_uid)
def test_oracle_upsample_equals_scipy_on_nonfinite_flows(oracle, i):
    cshape, tshape = S.UPSAMPLE_CASES[i]
    u, v = S.plant_nonfinite(*S.flow_fields(cshape, i), seed=i)
    assert np.isnan(u).any() and np.isposinf(u).any() and np.isneginf(u).any()
    with np.errstate(invalid="ignore"):
        su, sv = scipy_upsample_flow(u, v, tshape)
    ou, ov = oracle.upsample_flow(u, v, tshape)
    S.same_bits(ou, su, f"upsample {cshape} -> {tshape} with non-finite flows, u")
    S.same_bits(ov, sv, f"upsample {cshape} -> {tshape} with non-finite flows, v")


@pytest.mark.parametrize("i", range(len(S.PYRAMID_CASES)), ids=_pid)
def test_oracle_pyramid_equals_scipy(oracle, i):
    shape, levels, sf = S.PYRAMID_CASES[i]
    img = S.image_field(shape, i)
    got, exp = oracle.build_gaussian_pyramid(img, levels, sf), scipy_pyramid(img, levels, sf)
    assert [g.shape for g in got] == [e.shape for e in exp] == S.level_shapes(shape, levels, sf)[::-1]
    for l, (g, e) in enumerate(zip(got, exp)):
        S.same_bits(g, e, f"pyramid {shape} x{levels} at {sf!r}, level {l} {e.shape}")


# ---- 2. what the lists cover ------------------------------------------------------------------------------------------------------
def test_cases_are_distinct_and_named_by_the_issue():
    assert len(set(S.UPSAMPLE_CASES)) == len(S.UPSAMPLE_CASES) and len(set(S.PYRAMID_CASES)) == len(S.PYRAMID_CASES)
    assert len(set(S.UPSAMPLE_NONFINITE)) == len(S.UPSAMPLE_NONFINITE)
    for c in [((540, 960), (1080, 1920)), ((101, 158), (203, 317)), ((37, 641), (75, 1283)), ((240, 320), (360, 480)),
              ((300, 700), (301, 701)), ((480, 640), (240, 320)), ((500, 520), (171, 173)), ((137, 300), (16, 512)),
              ((60, 80), (7, 1000)), ((12, 300), (36, 900)), ((1, 1), (40, 50)), ((1, 9), (3, 700)), ((9, 1), (700, 3)),
              ((2, 2), (33, 1025)), ((37, 53), (1, 1)), ((37, 53), (1, 300))]:
        assert c in S.UPSAMPLE_CASES, c
    for sf in S.BAND_FACTORS:
        assert S.gauss_radius(sf) == 8 and ((480, 640), 3, sf) in S.PYRAMID_CASES, sf
    assert S.gauss_radius(8.0 / 17.0) == 9 and S.gauss_radius(8.0 / 15.0 + 1e-9) == 7
    for sf in (0.6, 0.4, 0.75, 0.3, 0.25, 0.9, 1.0):
        assert ((480, 640), 3, sf) in S.PYRAMID_CASES and S.gauss_radius(sf) != 8
    assert S.gauss_radius(1.0 / 16.0) == 64 and S.gauss_radius(0.062) == 65
    for shape, levels, sf in S.PYRAMID_CASES:
        assert all(h >= 1 and w >= 1 for h, w in S.level_shapes(shape, levels, sf)), (shape, levels, sf)


def test_upsample_cases_reach_both_kernels_and_the_edges(L):
    kern = [S.upsample_kernel(L, c, t) for c, t in S.UPSAMPLE_CASES]
    spans = [S.upsample_spans(c, t) for c, t in S.UPSAMPLE_CASES]
    assert kern.count("k_resample<2>") >= 8 and kern.count("k_upsample") >= 8
    # the decision is the span against the staged tile, on every case
    for (c, t), k, sp in zip(S.UPSAMPLE_CASES, kern, spans):
        fits = sp[0] <= S.UPSAMPLE_CAP[0] and sp[1] <= S.UPSAMPLE_CAP[1]
        assert (k == "k_upsample") == fits, (c, t, k, sp)
    # the edges the issue names
    edge = {((20, 136), (40, 257)): 1, ((20, 137), (40, 258)): 1, ((20, 137), (40, 257)): 0, ((20, 138), (40, 258)): 0,
            ((10, 80), (17, 160)): 1, ((11, 80), (18, 160)): 1, ((11, 80), (17, 160)): 0, ((12, 80), (18, 160)): 0,
            ((10, 136), (17, 257)): 1, ((11, 137), (18, 258)): 1, ((11, 137), (17, 257)): 0, ((12, 138), (18, 258)): 0}
    for (c, t), staged in edge.items():
        assert (c, t) in S.UPSAMPLE_CASES and L.oflk_upsample_staged(c[0], c[1], t[0], t[1]) == staged, (c, t)
    for axis in (0, 1):
        other = 1 - axis
        # exactly at the capacity and staged, with more than one tile along the axis; exactly one over (the other axis fitting)
        assert any(k == "k_upsample" and sp[axis] == S.UPSAMPLE_CAP[axis] and t[axis] > S.UPSAMPLE_TILE[axis]
                   for (c, t), k, sp in zip(S.UPSAMPLE_CASES, kern, spans)), axis
        assert any(k == "k_resample<2>" and sp[axis] == S.UPSAMPLE_CAP[axis] + 1 and sp[other] <= S.UPSAMPLE_CAP[other]
                   for k, sp in zip(kern, spans)), axis
    # several tiles along both axes on both kernels, and the ratios other than 2 are fallback cases wider than one block
    for want in ("k_upsample", "k_resample<2>"):
        assert any(k == want and t[0] > 2 * S.UPSAMPLE_TILE[0] and t[1] > S.UPSAMPLE_TILE[1]
                   for (c, t), k in zip(S.UPSAMPLE_CASES, kern)), want
    for c, t in [((240, 320), (360, 480)), ((240, 320), (240, 320)), ((300, 700), (301, 701)), ((480, 640), (240, 320)),
                 ((137, 300), (16, 512)), ((60, 80), (7, 1000))]:
        assert S.upsample_kernel(L, c, t) == "k_resample<2>", (c, t)
    nf = [kern[i] for i in S.UPSAMPLE_NONFINITE]
    assert nf.count("k_upsample") >= 1 and nf.count("k_resample<2>") >= 3
    # both store variants of both kernels (16-byte stores need a target width that is a multiple of 4)
    for want in ("k_upsample", "k_resample<2>"):
        assert {t[1] % 4 == 0 for (c, t), k in zip(S.UPSAMPLE_CASES, kern) if k == want} == {True, False}, want


def test_pyramid_cases_reach_both_paths_and_the_edges(L):
    fused_steps = unfused_steps = 0
    per_factor = {sf: {"rows": set(), "cols": set(), "paths": set()} for sf in S.BAND_FACTORS}
    at_cap, one_over = [0, 0], [0, 0]
    for shape, levels, sf in S.PYRAMID_CASES:
        kerns = S.pyramid_kernels(L, shape, levels, sf)
        for (src, dst), k in zip(S.pyramid_steps(shape, levels, sf), kerns):
            sp = S.pyramid_spans(src, dst)
            fits = sp[0] <= S.PYRAMID_CAP[0] and sp[1] <= S.PYRAMID_CAP[1]
            if S.gauss_radius(sf) != 8:
                assert k != "k_pyr_down", (shape, sf)
                unfused_steps += 1
                continue
            assert (k == "k_pyr_down") == fits, (shape, levels, sf, src, dst, sp, k)
            fused_steps += fits
            unfused_steps += not fits
            if sf in per_factor:
                per_factor[sf]["paths"].add(k)
                per_factor[sf]["rows"].add(sp[0] <= S.PYRAMID_CAP[0])
                per_factor[sf]["cols"].add(sp[1] <= S.PYRAMID_CAP[1])
            for axis in (0, 1):
                other = 1 - axis
                at_cap[axis] += fits and sp[axis] == S.PYRAMID_CAP[axis]
                one_over[axis] += sp[axis] == S.PYRAMID_CAP[axis] + 1 and sp[other] <= S.PYRAMID_CAP[other]
    for sf in S.BAND_FACTORS:
        rows_both, cols_both = S.BAND_BOTH_SIDES[sf]
        got = per_factor[sf]
        assert "k_pyr_down" in got["paths"], sf
        assert got["rows"] == ({True, False} if rows_both else {True}), (sf, got)
        assert got["cols"] == ({True, False} if cols_both else {True}), (sf, got)
        assert ("k_blur+k_resample<1>" in got["paths"]) == (rows_both or cols_both), (sf, got)
    assert min(at_cap) >= 1 and min(one_over) >= 1, (at_cap, one_over)
    # the capacity is met at every factor of the band below 0.5, on both axes, by a fused step
    for sf in (0.48, 0.485, 0.49, 0.495, 0.499):
        for axis in (0, 1):
            assert any(S.pyramid_kernels(L, sh, lv, f)[0] == "k_pyr_down"
                       and S.pyramid_spans(*S.pyramid_steps(sh, lv, f)[0])[axis] == S.PYRAMID_CAP[axis]
                       for sh, lv, f in S.PYRAMID_BAND if f == sf), (sf, axis)
    assert fused_steps >= 40 and unfused_steps >= 40, (fused_steps, unfused_steps)
    # the unfused chain: outputs over more than one x-block of k_resample (256 outputs), both store variants, the largest
    # radius, levels shorter than the radius
    wo = [S.level_shapes(sh, lv, sf)[1][1] for sh, lv, sf in S.PYRAMID_UNFUSED]
    assert any(w > 256 and w % 4 == 0 for w in wo) and any(w > 256 and w % 4 != 0 for w in wo) and max(wo) > 1024
    assert any(S.gauss_radius(sf) == 64 for _, _, sf in S.PYRAMID_UNFUSED)
    assert any(min(sh) < S.gauss_radius(sf) // 2 for sh, _, sf in S.PYRAMID_UNFUSED)


def test_band_sweep_finds_both_paths_where_the_lists_say(L):
    """BAND_BOTH_SIDES is what a sweep of the library's decision over sizes 40 .. 699 finds (the other axis 20 -> fits), and
    the decision is the span against the tile at every size of the sweep"""
    for sf in S.BAND_FACTORS:
        h0, w0 = 20, 40
        assert L.oflk_pyramid_step_fused(h0, w0, int(h0 * sf), int(w0 * sf), 8) == 1
        rows, cols = set(), set()
        for n in range(40, 700):
            m = int(n * sf)
            r = L.oflk_pyramid_step_fused(n, w0, m, int(w0 * sf), 8)
            c = L.oflk_pyramid_step_fused(h0, n, int(h0 * sf), m, 8)
            assert r == (S.max_span(n, m, S.PYRAMID_TILE[0]) <= S.PYRAMID_CAP[0]), (sf, n)
            assert c == (S.max_span(n, m, S.PYRAMID_TILE[1]) <= S.PYRAMID_CAP[1]), (sf, n)
            rows.add(r)
            cols.add(c)
        assert (rows == {0, 1}, cols == {0, 1}) == S.BAND_BOTH_SIDES[sf], (sf, rows, cols)


# ---- 3. the predicates ------------------------------------------------------------------------------------------------------------
def test_pyramid_step_is_fused_for_radius_8_only(L):
    for radius in list(range(0, 8)) + list(range(9, 66)) + [-1, 1 << 20]:
        for h, w in ((480, 640), (64, 64), (2, 2), (1080, 1920)):
            assert L.oflk_pyramid_step_fused(h, w, h // 2, w // 2, radius) == 0, (radius, h, w)
    assert L.oflk_pyramid_step_fused(480, 640, 240, 320, 8) == 1


def test_predicates_never_fail_on_sizes_below_one(L):
    for bad in (0, -1, -(1 << 30)):
        assert L.oflk_upsample_staged(bad, 8, 16, 16) == 0 and L.oflk_upsample_staged(8, 8, 16, bad) == 0
        assert L.oflk_pyramid_step_fused(bad, 8, 4, 4, 8) == 0 and L.oflk_pyramid_step_fused(8, 8, 4, bad, 8) == 0
    assert L.oflk_upsample_staged(1, 1, 1, 1) == 1 and L.oflk_pyramid_step_fused(2, 2, 1, 1, 8) == 1


def test_ratio_two_is_always_staged_and_fused(L):
    """every size a pyramidal pass can meet, 2 .. 2000 per axis: the finer level n, the coarser int(n * 0.5)"""
    for n in range(2, 2001):
        m = int(n * 0.5)
        assert S.max_span(m, n, S.UPSAMPLE_TILE[0]) <= S.UPSAMPLE_CAP[0] and S.max_span(m, n, S.UPSAMPLE_TILE[1]) <= S.UPSAMPLE_CAP[1]
        assert S.max_span(n, m, S.PYRAMID_TILE[0]) <= S.PYRAMID_CAP[0] and S.max_span(n, m, S.PYRAMID_TILE[1]) <= S.PYRAMID_CAP[1]
        assert L.oflk_upsample_staged(m, 50, n, 100) == 1 and L.oflk_upsample_staged(50, m, 100, n) == 1, n
        assert L.oflk_pyramid_step_fused(n, 100, m, 50, 8) == 1 and L.oflk_pyramid_step_fused(100, n, 50, m, 8) == 1, n
        assert L.oflk_upsample_staged(m, m, n, n) == 1 and L.oflk_pyramid_step_fused(n, n, m, m, 8) == 1, n


def test_upsample_predicate_is_the_span_against_the_tile(L):
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(4000):
        hc, wc = int(rng.integers(1, 400)), int(rng.integers(1, 1500))
        ht, wt = int(rng.integers(1, 700)), int(rng.integers(1, 2600))
        sp = S.upsample_spans((hc, wc), (ht, wt))
        fits = sp[0] <= S.UPSAMPLE_CAP[0] and sp[1] <= S.UPSAMPLE_CAP[1]
        assert L.oflk_upsample_staged(hc, wc, ht, wt) == fits, (hc, wc, ht, wt, sp)
        seen.add(fits)
    assert seen == {True, False}
    # the column edge at every width of a second tile: coarse n -> 2 n - 15 .. 2 n + 2
    for n in range(130, 400):
        for wt in range(2 * n - 15, 2 * n + 3):
            fits = S.max_span(n, wt, S.UPSAMPLE_TILE[1]) <= S.UPSAMPLE_CAP[1]
            assert L.oflk_upsample_staged(20, n, 40, wt) == fits, (n, wt)


# ---- 4. frames the signed 24-bit row product cannot address ---------------------------------------------------------------------
def test_frames_of_2_to_the_23_rows_or_columns_are_refused_before_any_device_call(L):
    import _oflk

    f32p, UNS = ctypes.POINTER(ctypes.c_float), _oflk.OFLK_ERR_UNSUPPORTED
    buf = ctypes.cast(ctypes.c_void_p(1 << 20), f32p)   # never dereferenced: each call below ends in its checks
    vbuf = ctypes.c_void_p(1 << 20)
    BIG = 1 << 23

    def calls(H, W):
        h = ctypes.c_void_p()
        yield "oflk_warp", L.oflk_warp(buf, buf, buf, H, W, buf)
        yield "oflk_upsample_flow (coarse)", L.oflk_upsample_flow(buf, buf, H, W, 4, 4, buf, buf)
        yield "oflk_upsample_flow (target)", L.oflk_upsample_flow(buf, buf, 4, 4, H, W, buf, buf)
        yield "oflk_single_scale", L.oflk_single_scale(buf, buf, H, W, 5, buf, buf)
        yield "oflk_fb_consistency_host", L.oflk_fb_consistency_host(buf, buf, buf, buf, 1, H, W, 0.01, 0.5, buf, buf, vbuf, vbuf)
        yield "oflk_track_points_host", L.oflk_track_points_host(buf, buf, buf, buf, 1, H, W, 0.01, 0.5, None, buf, 1, buf, vbuf)
        yield "oflk_plan_create", L.oflk_plan_create(ctypes.byref(h), 0, 1, H, W, 1, 5, 0)
        assert not h.value

    for H, W in ((3, BIG), (BIG, 3), (1, BIG), (BIG, 1), (3, (1 << 24) - 1)):
        for name, rc in calls(H, W):
            assert rc == UNS, (name, H, W, rc, L.oflk_last_error())
            assert b"2^23" in L.oflk_last_error(), (name, L.oflk_last_error())
    # one less passes the size check.  Only where no device is usable is that safe to ask: the call then ends in
    # OFLK_ERR_NO_DEVICE before it reads a pointer; with a device it would go on to copy from them.
    if _oflk.device_count() == 0:
        for H, W in ((3, BIG - 1), (BIG - 1, 3)):
            for name, rc in calls(H, W):
                assert rc == _oflk.OFLK_ERR_NO_DEVICE, (name, H, W, rc, L.oflk_last_error())
