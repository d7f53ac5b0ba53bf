"""The stage entry points with a free resampling ratio against the oracle, bit for bit, on every case of
tests/stage_scenes.py: upsample_flow (k_upsample and its fallback k_resample<2>) and build_gaussian_pyramid (k_pyr_down
and the unfused chain k_blur<0>, k_blur<1>, k_resample<1>), away from the half-scale ratio of a pyramidal pass.

There is no tolerance here: NaN at the same positions, every other element the same 32 bits, every element compared.
tests/test_stages_cpu.py holds the oracle to SciPy on the same cases and asserts which kernel each case reaches.

A staged kernel that read one cell past its LDS tile would get whatever a block staged there last, so a case runs twice
inside one test, the second time after a call of another shape with values far from the case's, and both results must equal
the oracle.  A failure names the case, the kernel that liboflk's own predicate chose, the number of differing elements and
the first differing index with both values.

Run on an MI355X:  python -m pytest tests/test_gpu_stages.py -m gpu -q
"""
import ctypes

import numpy as np
import pytest

import stage_scenes as S

pytestmark = pytest.mark.gpu

_f32p = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def P():
    import lucas_kanade_pyramidal

    return lucas_kanade_pyramidal


@pytest.fixture(scope="module")
def L():
    import _oflk

    return _oflk.lib()


def _uid(i):
    c, t = S.UPSAMPLE_CASES[i]
    return f"{c[0]}x{c[1]}-{t[0]}x{t[1]}"


def _pid(i):
    (h, w), lv, sf = S.PYRAMID_CASES[i]
    return f"{h}x{w}-L{lv}-{sf:.6g}"


def _disturb_upsample(P):
    """a call of another shape on both kernels' paths, with values far from any case's"""
    rng = np.random.default_rng(77)
    for cshape, tshape in (((23, 300), (47, 601)), ((50, 300), (40, 333))):
        a = rng.normal(1e6, 1e5, cshape).astype(np.float32)
        P.upsample_flow(a, -a, tshape)


def _disturb_pyramid(P):
    rng = np.random.default_rng(78)
    P.build_gaussian_pyramid(rng.normal(-1e6, 1e5, (150, 210)).astype(np.float32), 2, 0.5)
    P.build_gaussian_pyramid(rng.normal(-1e6, 1e5, (90, 300)).astype(np.float32), 2, 0.7)


def _check_upsample(P, L, oracle, i, u, v, tag):
    cshape, tshape = S.UPSAMPLE_CASES[i]
    kern, spans = S.upsample_kernel(L, cshape, tshape), S.upsample_spans(cshape, tshape)
    ou, ov = oracle.upsample_flow(u, v, tshape)
    for run in ("first call", "after a call of another shape"):
        gu, gv = P.upsample_flow(u, v, tshape)
        what = f"upsample_flow {cshape} -> {tshape}{tag}, {kern} (span {spans[0]} rows x {spans[1]} columns), {run}"
        S.same_bits(gu, ou, what + ", u")
        S.same_bits(gv, ov, what + ", v")
        _disturb_upsample(P)


@pytest.mark.parametrize("i", range(len(S.UPSAMPLE_CASES)), ids=_uid)
def test_upsample_flow_equals_the_oracle(P, L, oracle, i):
    u, v = S.flow_fields(S.UPSAMPLE_CASES[i][0], i)
    _check_upsample(P, L, oracle, i, u, v, "")


@pytest.mark.parametrize("i", S.UPSAMPLE_NONFINITE, ids=_uid)
def test_upsample_flow_equals_the_oracle_on_nonfinite_flows(P, L, oracle, i):
    u, v = S.plant_nonfinite(*S.flow_fields(S.UPSAMPLE_CASES[i][0], i), seed=i)
    _check_upsample(P, L, oracle, i, u, v, " with NaN and +-inf flows")


def _check_levels(got, exp, shapes, what):
    assert [g.shape for g in got] == [e.shape for e in exp] == shapes, what
    for l, (g, e) in enumerate(zip(got, exp)):
        S.same_bits(g, e, f"{what}, level {l} {e.shape}")


@pytest.mark.parametrize("i", range(len(S.PYRAMID_CASES)), ids=_pid)
def test_build_gaussian_pyramid_equals_the_oracle(P, L, oracle, i):
    shape, levels, sf = S.PYRAMID_CASES[i]
    img = S.image_field(shape, i)
    kerns = S.pyramid_kernels(L, shape, levels, sf)
    spans = [S.pyramid_spans(s, d) for s, d in S.pyramid_steps(shape, levels, sf)]
    exp = oracle.build_gaussian_pyramid(img, levels, sf)
    shapes = S.level_shapes(shape, levels, sf)[::-1]
    assert P.pyramid_level_shapes(shape, levels, sf) == shapes
    for run in ("first call", "after a call of another shape"):
        got = P.build_gaussian_pyramid(img, levels, sf)
        _check_levels(got, exp, shapes, f"build_gaussian_pyramid {shape} x{levels} at {sf!r}, steps finest first {kerns} "
                                        f"(spans rows x columns {spans}, radius {S.gauss_radius(sf)}), {run}")
        _disturb_pyramid(P)


def _build_pyramid_c(L, img, levels, sf):
    """oflk_build_pyramid itself: the library's own Gaussian weights (SciPy's table at sigma 2, libm's exp elsewhere)"""
    import _oflk

    H, W = img.shape
    dims = (ctypes.c_int * (2 * levels))()
    _oflk.check(L.oflk_pyramid_level_dims(H, W, levels, float(sf), dims))
    outs = [np.full((dims[2 * l], dims[2 * l + 1]), np.nan, np.float32) for l in range(levels)]
    arr = (_f32p * levels)(*[_oflk.ptr(o) for o in outs])
    _oflk.check(L.oflk_build_pyramid(_oflk.ptr(img), H, W, levels, float(sf), arr))
    return outs


def _libm_cases():
    """one case per scale factor of the lists: the 480 x 640 one where there is one, else the first"""
    by_sf = {}
    for shape, levels, sf in S.PYRAMID_CASES:
        if sf not in by_sf or (shape == (480, 640) and by_sf[sf][0] != (480, 640)):
            by_sf[sf] = (shape, levels, sf)
    return list(by_sf.values())


@pytest.mark.parametrize("case", _libm_cases(), ids=lambda c: f"{c[0][0]}x{c[0][1]}-L{c[1]}-{c[2]:.6g}")
def test_oflk_build_pyramid_equals_the_all_c_oracle(L, oracle, case):
    """no caller weights: liboflk forms the Gaussian itself, with the same libm on the same host as the oracle's all-C form"""
    shape, levels, sf = case
    img = S.image_field(shape, 500)
    got = _build_pyramid_c(L, img, levels, sf)
    exp = oracle.build_gaussian_pyramid_libm(img, levels, sf)
    _check_levels(got, exp, S.level_shapes(shape, levels, sf)[::-1],
                  f"oflk_build_pyramid {shape} x{levels} at {sf!r}, steps finest first {S.pyramid_kernels(L, shape, levels, sf)}")


@pytest.mark.parametrize("shape,levels", [((480, 640), 3), ((203, 317), 3), ((1080, 1920), 2), ((2, 2), 2), ((66, 130), 4)])
def test_oflk_build_pyramid_at_the_default_factor_equals_the_scipy_weights_form(L, oracle, shape, levels):
    """at 0.5 the library's embedded table is SciPy's own kernel: the result is the reference's pyramid"""
    img = S.image_field(shape, 501)
    got = _build_pyramid_c(L, img, levels, 0.5)
    _check_levels(got, oracle.build_gaussian_pyramid(img, levels, 0.5), S.level_shapes(shape, levels, 0.5)[::-1],
                  f"oflk_build_pyramid {shape} x{levels} at 0.5")
    _check_levels(got, oracle.build_gaussian_pyramid_libm(img, levels, 0.5), S.level_shapes(shape, levels, 0.5)[::-1],
                  f"oflk_build_pyramid {shape} x{levels} at 0.5 (all-C oracle)")


@pytest.mark.parametrize("shape,levels,sf,kind", S.PYRAMID_REFUSALS)
def test_pyramid_refusals_stay(P, L, shape, levels, sf, kind):
    import _oflk

    img = S.image_field(shape, 502)
    if kind == "invalid":
        with pytest.raises(ValueError):
            P.build_gaussian_pyramid(img, levels, sf)
    else:
        with pytest.raises(_oflk.OflkError) as e:
            P.build_gaussian_pyramid(img, levels, sf)
        assert e.value.code == _oflk.OFLK_ERR_UNSUPPORTED
        with pytest.raises(_oflk.OflkError) as e:
            _build_pyramid_c(L, img, levels, sf)
        assert e.value.code == _oflk.OFLK_ERR_UNSUPPORTED
