"""oflk_pyramid_step_half on the CPU: does a pyramid step run k_pyr_down's half-scale instantiation?
It does when the step is tight (oflk_pyramid_step_form == 2), has at least two outputs per axis, and
floor(np.linspace(0, S - 1, T)[i]) == 2 i for every i < T - 1 on both axes: every level of an even-sized frame at scale
factor 0.5.  A tight step at another ratio of the radius-8 band keeps the tight tile's run-time indices."""
import numpy as np

import pyr_half_scenes as S

EVEN_FRAMES = [(64, 96), (96, 200), (1080, 1920), (2160, 3840)]


def lib():
    import _oflk

    return _oflk.lib()


def test_every_step_of_an_even_sized_frame_is_half_scale():
    L = lib()
    for shape in EVEN_FRAMES:
        st = S.steps(L, shape, 3)
        assert len(st) == 2
        for h, w, ho, wo in st:
            assert (ho, wo) == (h // 2, w // 2)
            assert L.oflk_pyramid_step_form(h, w, ho, wo, 8) == S.TIGHT and L.oflk_pyramid_step_half(h, w, ho, wo, 8) == 1, (h, w)
    for n in range(34, 4401, 2):   # every even size up to 4400 per axis
        (h, w, ho, wo), = S.steps(L, (n, n), 2)
        assert (ho, wo) == (n // 2, n // 2) and L.oflk_pyramid_step_half(h, w, ho, wo, 8) == 1, n
        assert L.oflk_pyramid_step_half(n, 1920, n // 2, 960, 8) == 1 and L.oflk_pyramid_step_half(1080, n, 540, n // 2, 8) == 1, n


def test_a_step_that_is_not_tight_is_not_half_scale():
    L = lib()
    for args in ((33, 33, 16, 16), (33, 64, 16, 32), (64, 67, 32, 33), (67, 67, 33, 33), (101, 201, 50, 100)):
        assert L.oflk_pyramid_step_form(*args, 8) != S.TIGHT, args
        assert L.oflk_pyramid_step_half(*args, 8) == 0, args
    assert L.oflk_pyramid_step_form(64, 96, 25, 38, 8) == S.UNFUSED and L.oflk_pyramid_step_half(64, 96, 25, 38, 8) == 0
    assert L.oflk_pyramid_step_half(64, 96, 32, 48, 7) == 0   # another radius: the unfused chain
    for args in ((0, 0, 0, 0), (-5, 3, 7, 9)):
        assert L.oflk_pyramid_step_half(*args, 8) == 0


def test_a_tight_step_away_from_the_half_scale_ratio_exists_and_is_not_half_scale():
    L = lib()
    found = S.tight_but_not_half(L)
    assert found is not None, "no tight step off the half-scale ratio near 100 x 150 at 0.52"
    (h, w), sf = found
    ho, wo = int(h * sf), int(w * sf)
    assert int(4.0 / sf + 0.5) == 8
    assert L.oflk_pyramid_step_form(h, w, ho, wo, 8) == S.TIGHT and L.oflk_pyramid_step_half(h, w, ho, wo, 8) == 0
    assert not (S.half_axis(h, ho) and S.half_axis(w, wo))
    # one output per axis: tight, never half scale
    assert L.oflk_pyramid_step_form(2, 2, 1, 1, 8) == S.TIGHT and L.oflk_pyramid_step_half(2, 2, 1, 1, 8) == 0


def test_predicate_agrees_with_numpy_linspace():
    """a few hundred random (S, T) per axis around the ratio 2, the other axis a known half-scale one and both random"""
    L = lib()
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(400):
        s = int(rng.integers(2, 900))
        t = max(1, int(s / rng.choice([1.9, 1.96, 2.0, 2.0, 2.04, 2.1])) + int(rng.integers(-1, 2)))
        s2 = int(rng.integers(2, 900))
        t2 = (s2 + int(rng.integers(0, 2))) // 2
        for h, w, ho, wo in ((s, 96, t, 48), (64, s, 32, t), (s, s2, t, max(t2, 1))):
            tight = L.oflk_pyramid_step_form(h, w, ho, wo, 8) == S.TIGHT
            exp = tight and S.half_axis(h, ho) and S.half_axis(w, wo)
            assert L.oflk_pyramid_step_half(h, w, ho, wo, 8) == int(exp), (h, w, ho, wo)
            seen.add((tight, exp))
    assert seen == {(False, False), (True, False), (True, True)}
    # odd sizes whose linspace step is exactly 2 (S = 2 T - 1): every point but the last at 2 i, the last at 2 (T - 1)
    for s, t in ((33, 17), (65, 33), (5, 3)):
        assert S.half_axis(s, t) and L.oflk_pyramid_step_half(s, s, t, t, 8) == 1, (s, t)
