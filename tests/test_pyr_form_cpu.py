"""oflk_pyramid_step_form on the CPU: which of its three paths a pyramid step takes (2: k_pyr_down's tight tile, 32 x 64
blurred values per 32 x 16 output tile; 1: its general tile, 34 x 66; 0: the unfused chain).  The decision is the span
arithmetic of the kernel's own indices, restated here in Python."""
import math

import numpy as np

UNFUSED, GENERAL, TIGHT = 0, 1, 2


def largest_span(S, T, tile):
    """source elements the widest run of `tile` outputs of np.linspace(0, S - 1, T) touches, both bilinear taps counted"""
    step = (S - 1) / (T - 1) if T > 1 else 0.0
    at = lambda i: 0.0 if T <= 1 else (float(S - 1) if i == T - 1 else i * step)
    worst = 0
    for t0 in range(0, T, tile):
        lo = math.floor(at(t0))
        if t0 + tile >= T:
            lo = min(lo, max(S - 2, 0))
        hi = min(math.floor(at(min(t0 + tile, T) - 1)) + 1, S - 1)
        worst = max(worst, hi - lo + 1)
    return worst


def form(h, w, ho, wo):
    rows, cols = largest_span(h, ho, 16), largest_span(w, wo, 32)
    return TIGHT if rows <= 32 and cols <= 64 else GENERAL if rows <= 34 and cols <= 66 else UNFUSED


def lib():
    import _oflk

    return _oflk.lib()


def test_half_scale_steps_of_even_sizes_are_tight():
    L = lib()
    for S in range(34, 4401, 2):
        assert L.oflk_pyramid_step_form(S, S, S // 2, S // 2, 8) == TIGHT, S
        assert L.oflk_pyramid_step_form(S, 1920, S // 2, 960, 8) == TIGHT and L.oflk_pyramid_step_form(1080, S, 540, S // 2, 8) == TIGHT, S


def test_a_tile_that_needs_33_values_keeps_the_general_form():
    L = lib()
    assert largest_span(33, 16, 16) == 33
    assert L.oflk_pyramid_step_form(33, 33, 16, 16, 8) == GENERAL
    assert L.oflk_pyramid_step_form(33, 64, 16, 32, 8) == GENERAL
    # 33 columns are one tile of 16 outputs, well inside 64; 67 -> 33 columns put 65 under a full tile of 32
    assert L.oflk_pyramid_step_form(64, 33, 32, 16, 8) == TIGHT
    assert largest_span(67, 33, 32) == 65 and L.oflk_pyramid_step_form(64, 67, 32, 33, 8) == GENERAL


def test_form_agrees_with_the_span_arithmetic_and_with_the_fused_predicate():
    L = lib()
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(400):
        h, w = (int(x) for x in rng.integers(2, 700, 2))
        # ratios around 2 (where the three forms meet) and anywhere
        ho, wo = (max(1, int(s / r)) for s, r in zip((h, w), rng.choice([1.7, 1.9, 2.0, 2.05, 2.1, 2.2, 2.5], 2)))
        if rng.random() < 0.25:
            ho, wo = (int(x) for x in rng.integers(1, 400, 2))
        got = L.oflk_pyramid_step_form(h, w, ho, wo, 8)
        assert got == form(h, w, ho, wo), (h, w, ho, wo)
        assert (got != UNFUSED) == bool(L.oflk_pyramid_step_fused(h, w, ho, wo, 8))
        assert L.oflk_pyramid_step_form(h, w, ho, wo, 7) == UNFUSED
        seen.add(got)
    assert seen == {UNFUSED, GENERAL, TIGHT}
    for args in ((0, 0, 0, 0), (-5, 3, 7, 9)):
        assert L.oflk_pyramid_step_form(*args, 8) == UNFUSED
