"""The CPU statement of the fp16 single-scale mode (oracle/oflk_fp16_model.py) on its own, without a GPU: its rounding
primitive against exact rational rounding, its window sums against box sums (every tap, once), its sensitivity to the
order and coverage errors the GPU tolerance must see, its accuracy against the exact flow (the bars of
tests/test_gpu_fp16.py), and the range scaling on adversarial frames.  tests/test_gpu_fp16.py holds the kernel to it."""
from fractions import Fraction

import numpy as np
import pytest

import oflk_fp16_model as M
from test_gpu_fp16 import PATTERNS, TOL_MEAN_ALL, TOL_MEDIAN, TOL_WELL_CONDITIONED_MEAN, epe_of

WINDOWS = (3, 5, 7, 9, 11)
PIXEL_MAX = (1.0, 255.0, 1023.0, 4095.0, 65535.0)
GPU_ULP = 2   # the kernel's tolerance against the model, tests/test_gpu_fp16.py


def _rne_fp16(x: Fraction) -> float:
    """x rounded to the nearest fp16 value, ties to even, subnormals kept, overflow to inf -- in exact arithmetic"""
    if x == 0:
        return 0.0
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2^e <= a < 2^(e+2)
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    q = Fraction(2) ** (max(e, -14) - 10)   # the fp16 quantum at a's binade (subnormal below 2^-14)
    n = a / q
    m = n.numerator // n.denominator
    rem = n - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m % 2 == 1):
        m += 1
    r = m * q
    return s * float("inf") if r > 65504 else s * float(r)


def _fp16_operands(rng):
    """random fp16 values of every binade, subnormals, ties and operands whose sum or product overflows"""
    bits = rng.integers(0, 0x7C00, 400).astype(np.uint16)           # finite non-negative fp16 bit patterns
    vals = bits.view(np.float16).astype(np.float64) * rng.choice([-1.0, 1.0], 400)
    sub = np.arange(1, 1024, 37) * 2.0 ** -24                         # subnormals
    pairs = [(float(a), float(b)) for a, b in zip(vals[:200], vals[200:])]
    pairs += [(float(a), float(b)) for a, b in zip(sub, sub[::-1])] + [(float(a), -float(b)) for a, b in zip(sub, sub[3:])]
    pairs += [(1.0, 2.0 ** -11), (1.0, 3 * 2.0 ** -11), (1.0 + 2.0 ** -10, 2.0 ** -11), (-1.0, -(2.0 ** -11)),   # add ties
              (2048.0, 1.0), (2048.0, 3.0), (2.0 ** -14, -(2.0 ** -24)), (6.1e-5, 2.0 ** -24),
              (65504.0, 8.0), (65504.0, 16.0), (65504.0, 15.0), (65504.0, 65504.0), (-65504.0, -16.0),        # overflow
              (255.0, 255.0), (256.0, 256.0), (1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10), (2.0 ** -12, 2.0 ** -12),   # products
              (2.0 ** -7, 2.0 ** -8), (3 * 2.0 ** -9, 2.0 ** -15), (1 + 2.0 ** -9, 1 + 2.0 ** -2)]
    return [(float(np.float16(a)), float(np.float16(b))) for a, b in pairs]


def test_rounding_primitive_is_exact_rne():
    rng = np.random.default_rng(0)
    r16 = M._Fp16()
    n = 0
    for a, b in _fp16_operands(rng):
        for exact, got in ((Fraction(a) + Fraction(b), a + b), (Fraction(a) * Fraction(b), a * b)):
            assert Fraction(got) == exact, (a, b)   # one fp16 add or multiply is exact in float64
            want = _rne_fp16(exact)
            have = float(r16(np.array([got]))[0])
            assert have == want, (a, b, float(exact), have, want)
            n += 1
    assert n > 500


def _box(c, hw):
    """exact box sums over (2HW+1)^2 taps where the window lies in the frame, NaN elsewhere"""
    n, H, W = c.shape
    out = np.full(c.shape, np.nan)
    for y in range(hw, H - hw):
        for x in range(hw, W - hw):
            out[:, y, x] = c[:, y - hw:y + hw + 1, x - hw:x + hw + 1].sum(axis=(1, 2))
    return out


@pytest.mark.parametrize("win", WINDOWS)
def test_window_sums_take_every_tap_once(win):
    """integer products small enough that every fp16 add is exact: the model's vertical and horizontal folds must give
    the box sums -- every row position mod S, both column parities, frames from 1 pixel to a few blocks"""
    hw = win // 2
    S = 2 * hw + 1
    rng = np.random.default_rng(win)
    sizes = (1, 2, 3, S - 1, S, S + 1)
    shapes = [(h, w) for h in sizes for w in sizes] + [(3 * S + 2, 2 * S + 3), (4 * S, 3 * S + 1), (2 * S + 5, 40)]
    for H, W in shapes:
        c = rng.integers(-8, 9, (2, H, W)).astype(np.float64)   # |sum| <= 121 * 8 < 2048: exact in fp16
        got = M.window_sums(c, win)
        want = _box(c, hw)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (win, H, W)
        assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (win, H, W)
        assert np.array_equal(M.window_sums(c, win, rounding=False), got, equal_nan=True)


@pytest.mark.parametrize("win", WINDOWS)
def test_row_bands_equal_the_whole_frame(win):
    """fp16_flow(rows=...) -- how the 8K frame is checked -- gives the whole frame's rows, at every band alignment"""
    rng = np.random.default_rng(100 + win)
    p = rng.integers(0, 256, (61, 45)).astype(np.float32)
    c = np.roll(p, (1, 2), (0, 1))
    u, v = M.fp16_flow(p, c, win)
    for y0, y1 in ((0, 61), (0, 1), (3, 17), (12, 13), (29, 61), (60, 61), (5, 5 + 2 * win + 1)):
        bu, bv = M.fp16_flow(p, c, win, rows=(y0, y1))
        assert np.array_equal(bu, u[y0:y1]) and np.array_equal(bv, v[y0:y1]), (win, y0, y1)


@pytest.fixture(scope="module")
def suite(golden_dir):
    d = np.load(golden_dir / "patterns_320x240.npz")
    p = d["frame_0"].astype(np.float32)
    return {n: (p, d[f"frame_1__{n}"].astype(np.float32)) for n in PATTERNS}


def _misses_gpu_bar(u, v, mu, mv):
    zeros, d = M.compare(u, v, mu, mv)
    return (not zeros) or d > GPU_ULP


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("win", [5, 7])
def test_gpu_tolerance_sees_order_and_coverage_errors(suite, variant, win):
    """a right fold taken as a left fold, blocks aligned to a segment start instead of absolute rows, one tap dropped at
    a strip seam: each moves the flow by more than the kernel's tolerance on every pattern that has motion"""
    for name in PATTERNS:
        p, c = suite[name]
        mu, mv = M.fp16_flow(p, c, win)
        u, v = M.fp16_flow(p, c, win, variant=variant)
        if name == "no_motion":   # It = 0: every numerator is 0 whatever the sums
            assert not mu.any() and not mv.any()
            continue
        assert _misses_gpu_bar(u, v, mu, mv), (variant, win, name)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("win", [7, 5])
def test_model_meets_the_epe_bars(suite, oracle, name, win):
    """the fp16 arithmetic as stated, against the exact flow: the bars tests/test_gpu_fp16.py holds the kernel to"""
    p, c = suite[name]
    u, v = oracle.lucas_kanade_single_scale(p, c, win)
    mu, mv = M.fp16_flow(p, c, win)
    st = epe_of(p, c, win, u, v, mu, mv)
    assert st["median_epe_all"] <= TOL_MEDIAN, st
    assert st["mean_epe_well_conditioned"] <= TOL_WELL_CONDITIONED_MEAN, st
    assert st["mean_epe_all"] <= TOL_MEAN_ALL, st


def range_frames(P: float, H: int = 36, W: int = 44):
    """frames that drive |Ix|, |Iy|, |It| and their products to the scaling rule's bound pixel_max / 2 (before scaling)"""
    y, x = np.mgrid[0:H, 0:W]
    cols = np.where(x % 4 >= 2, P, 0.0)      # (0, 0, P, P): |Ix| = P/2 at every column
    rows = np.where(y % 4 >= 2, P, 0.0)
    diag = np.where((x + y) % 4 >= 2, P, 0.0)
    zero, full = np.zeros((H, W)), np.full((H, W), P)
    pairs = {"cols": (cols, cols), "rows": (rows, rows), "dt": (zero, full), "dt_neg": (full, zero),
             "cols_vs_zero": (cols, zero), "rows_vs_full": (rows, full), "cols_vs_rows": (cols, rows),
             "diag": (diag, diag), "diag_vs_inverse": (diag, P - diag), "cols_vs_shift": (cols, np.roll(cols, 1, 1))}
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in pairs.items()}


@pytest.mark.parametrize("pixel_max", PIXEL_MAX)
@pytest.mark.parametrize("win", WINDOWS)
def test_range_scaling_keeps_fp16_finite(win, pixel_max):
    """no fp16 operation exceeds 65504 on frames at the range's edges, and the flow is finite; where the scaling is
    active (k > 0) the frames reach at least a quarter of the rule's 60000, so they do test it"""
    k = M.range_scale(win, pixel_max)[0]
    top = 0.0
    for name, (p, c) in range_frames(pixel_max).items():
        u, v, peak = M.fp16_flow(p, c, win, pixel_max, return_peak=True)
        assert peak <= M.FP16_MAX, (win, pixel_max, name, peak)
        assert np.isfinite(u).all() and np.isfinite(v).all(), (win, pixel_max, name)
        top = max(top, peak)
    if k > 0:
        assert top >= 15000.0, (win, pixel_max, top)
