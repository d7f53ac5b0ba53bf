"""The rounding certificate of the exact pyramid (k_pyr_down<PIX, PYR_CERTIFIED>) on the CPU:
wherever the guard calls a fused 17-tap sum t' safe, float32(t') is float32 of SciPy's sum t, bit for bit -- on random
windows, on windows steered onto float32 rounding boundaries, and at the edges of the number format -- and the guard
is needed (unguarded, some of those windows round differently) without firing often on ordinary frames."""
import numpy as np
import pytest

import pyr_cert_model as C

W = C.weights()


def bits32(t):
    return C.f32(t).view(np.uint32)


def check_safe_implies_equal(x):
    """returns (t, t', safe) after asserting the certificate on every window of x, with each value's own M"""
    x = np.asarray(x, np.float32)
    t, tp = C.scipy_sum(x, W), C.fma_sum(x, W)
    safe = C.guard_safe(tp, C.window_max(x))
    bad = safe & (bits32(t) != bits32(tp))
    assert not bad.any(), (x[bad][:3], t[bad][:3], tp[bad][:3])
    return t, tp, safe


@pytest.mark.parametrize("kind", C.KINDS)
def test_random_windows(kind):
    x = C.random_windows(kind, 4000, np.random.default_rng(7))
    t, tp, safe = check_safe_implies_equal(x)
    # the derivation bounds |t - t'| by 18 u M (1 + tiny); c = 32 is what the guard assumes
    M = C.window_max(x).astype(np.float64)
    worst = float(np.max(np.abs(t - tp) / (2.0 ** -53 * M)))
    print(f"{kind}: worst |t - t'| = {worst:.2f} u M, flagged {1 - safe.mean():.2e}")
    assert worst <= 18.0 * (1 + 2.0 ** -40)
    assert safe.mean() > 0.9 if kind != "normal" else safe.mean() > 0.5   # the guard is not vacuous


@pytest.mark.parametrize("kind", C.KINDS)
def test_windows_on_a_rounding_boundary(kind):
    """SciPy's t within 1, 16 and 256 fp64 ulps of a float32 midpoint, on both sides and exactly on it"""
    found = C.adversarial_windows(kind, 2024 + C.KINDS.index(kind))
    for band in C.BANDS:
        for side in ((0,) if band[0] == 0 else (-1, 1)):
            assert (band, side) in found, (kind, band, side)
    flagged_any = differs_any = False
    for (band, side), ws in found.items():
        x = np.asarray(ws, np.float32)
        d = C.midpoint_distance(C.scipy_sum(x, W))
        assert np.all((np.abs(d) >= band[0]) & (np.abs(d) <= band[1]) & (np.sign(d) == side))
        t, tp, safe = check_safe_implies_equal(x)
        # 18 u M is at most 18 * 64 ulps of a t' that passes the magnitude rule: every window this close must be flagged
        assert not safe.any(), (kind, band, side)
        flagged_any |= bool((~safe).any())
        differs_any |= bool((bits32(t) != bits32(tp)).any())
    assert flagged_any
    assert differs_any, "no steered window rounds differently when unguarded: the guard's necessity is untested"


def test_cancellation_and_magnitudes():
    rng = np.random.default_rng(11)
    n = 400
    sign = np.where(np.arange(17) % 2 == 0, 1.0, -1.0).astype(np.float32)
    cancel = (rng.integers(200, 256, (n, 17)).astype(np.float32) * sign)                      # t << M
    w17 = np.concatenate([W[:0:-1], W])
    ortho = rng.standard_normal((n, 17))
    ortho -= np.outer(ortho @ w17 / (w17 @ w17), w17)                                         # sum w x ~ 0
    ortho = (ortho * 1000).astype(np.float32)
    spike = (rng.random((n, 17), dtype=np.float32) * np.float32(1e-20)).astype(np.float32)    # one huge, many tiny
    spike[np.arange(n), rng.integers(0, 17, n)] = np.float32(3e30)
    far = spike.copy()
    far[:, 8] = np.float32(1e-30)
    zeros = np.zeros((4, 17), np.float32)
    negz = -zeros
    for name, x in (("cancel", cancel), ("ortho", ortho), ("spike", spike), ("far", far), ("zeros", zeros), ("-0", negz)):
        t, tp, safe = check_safe_implies_equal(x)
        print(f"{name}: flagged {1 - safe.mean():.3f}")
    t, tp, safe = check_safe_implies_equal(ortho)
    assert (~safe).any()                       # |t'| < M / 64 somewhere: the magnitude rule fires
    t, tp, safe = check_safe_implies_equal(zeros)
    assert safe.all() and np.all(bits32(tp) == 0)   # M == 0: proven, a black region costs no redo
    t, tp, safe = check_safe_implies_equal(negz)
    assert safe.all() and np.all(bits32(tp) == bits32(t))


def test_float32_range_edges():
    rng = np.random.default_rng(13)
    base = rng.integers(1, 256, (300, 17)).astype(np.float32)
    for scale, must_flag in ((2.0 ** -149, True), (2.0 ** -140, True), (2.0 ** -133, True), (2.0 ** -127, False),
                             (2.0 ** 119, False)):
        x = (base * np.float32(scale)).astype(np.float32)
        t, tp, safe = check_safe_implies_equal(x)
        print(f"scale 2^{int(np.log2(scale))}: flagged {1 - safe.mean():.3f}")
        if must_flag:   # float32 denormal results
            assert not safe.any(), scale
    x = (rng.integers(128, 256, (300, 17)).astype(np.float32) * np.float32(2.0 ** 120)).astype(np.float32)
    t, tp, safe = check_safe_implies_equal(x)     # results within a binade of overflow
    assert not safe.any()
    big = np.full((2, 17), np.finfo(np.float32).max, np.float32)     # float32(t) overflows
    t, tp, safe = check_safe_implies_equal(big)
    assert not safe.any()


def test_nan_and_inf_fall_to_the_doubtful_side():
    rng = np.random.default_rng(17)
    for bad in (np.nan, np.inf, -np.inf):
        x = rng.integers(0, 256, (34, 17)).astype(np.float32)
        x[np.arange(34), np.arange(34) % 17] = bad
        t, tp, safe = check_safe_implies_equal(x)
        assert not safe.any(), bad
    x = np.zeros((17, 17), np.float32)            # fmaxf drops the NaN: M reads 0, the zero rule must not pass it
    x[np.arange(17), np.arange(17)] = np.nan
    t, tp, safe = check_safe_implies_equal(x)
    assert np.all(C.window_max(x) == 0) and not safe.any()
    x = np.zeros((2, 17), np.float32)
    x[0, 3], x[0, 13] = np.inf, -np.inf           # the pair sum is NaN
    x[1, 3], x[1, 12] = np.inf, -np.inf
    t, tp, safe = check_safe_implies_equal(x)
    assert not safe.any()
    # the guard itself, on values no window produced
    for tp in (np.nan, np.inf, -np.inf):
        for M in (0.0, 1.0, np.inf, np.nan):
            assert not C.guard_safe(np.float64(tp), np.float32(M))
    assert not C.guard_safe(np.float64(1.0), np.float32(np.inf))


def test_a_smooth_frame_rarely_leaves_the_fast_path():
    """a smooth 8-bit-valued 64 x 96 texture: the share of 12-row x 64-column groups (what a wave of the vertical pass
    computes) that hold a flagged value stays below 5 % -- otherwise the GPU tests would never run the fast path"""
    img = C.smooth_u8(64, 96)
    assert np.array_equal(img, np.round(img)) and img.min() >= 0 and img.max() <= 255
    flagged, _ = C.flag_vertical(img)
    groups = [flagged[r: r + 12, c: c + 64].any() for r in range(0, 64, 12) for c in range(0, 96, 64)]
    share = float(np.mean(groups))
    print(f"flagged values {flagged.mean():.2e}, groups {sum(groups)} of {len(groups)}")
    assert share < 0.05
