"""Shapes for the tests of k_pyr_down's half-scale instantiation: the steps a pyramid takes, the
predicate oflk_pyramid_step_half restated with NumPy, and the search for a step that is tight (form 2) without being at
the exact half-scale ratio.  Shared by tests/test_pyr_half_cpu.py and tests/test_gpu_pyr_half.py."""
import numpy as np

UNFUSED, GENERAL, TIGHT = 0, 1, 2


def steps(L, shape, levels, sf=0.5):
    """(h, w, ho, wo) of every step of a pyramid, finest first, from the library's own level shapes"""
    import ctypes

    dims = (ctypes.c_int * (2 * levels))()
    assert L.oflk_pyramid_level_dims(shape[0], shape[1], levels, sf, dims) == 0
    d = [(dims[2 * l], dims[2 * l + 1]) for l in range(levels)]   # l = 0 is the coarsest
    return [(d[l + 1][0], d[l + 1][1], d[l][0], d[l][1]) for l in range(levels - 2, -1, -1)]


def half_axis(S, T):
    """every point of np.linspace(0, S - 1, T) but the last lies in [2 i, 2 i + 1)"""
    if T < 2:
        return False
    return bool(np.array_equal(np.floor(np.linspace(0, S - 1, T))[:-1], 2.0 * np.arange(T - 1)))


def tight_but_not_half(L, sf=0.52):
    """the first 2-level frame near 100 x 150 whose one step at `sf` (radius 8) is tight and not at the half-scale ratio"""
    for h in range(96, 112):
        for w in range(144, 160):
            ho, wo = int(h * sf), int(w * sf)
            if L.oflk_pyramid_step_form(h, w, ho, wo, 8) == TIGHT and not L.oflk_pyramid_step_half(h, w, ho, wo, 8):
                return (h, w), sf
    return None
