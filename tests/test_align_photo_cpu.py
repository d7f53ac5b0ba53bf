"""CPU tests of the photometric alignment's statement (tests/align_photo_model.py): planted pairs under a planted exposure
change, against the planted map and against the plain statement (tests/align_model.py) on the same frames.  No GPU is used.

The bounds were set before the code was written, from a prototype of the statement; the figures measured with the
statement are in DESIGN.md section 2.
"""
import functools

import numpy as np
import pytest

import align_model as AM
import align_photo_model as APM

SIZES = [(70, 257), (96, 130)]
KINDS = [("homography", AM.HOMOGRAPHY), ("affine", AM.AFFINE)]
EXPOSURES = [(0.7, 20.0), (1.3, -15.0), (1.0, 0.0)]
CORNER_BOUND = 0.05    # px: six times the 0.008 px worst of the statement on these pairs
LEVEL_BOUND = 0.5      # grey levels at v = 128


@functools.lru_cache(maxsize=None)
def planted(H, W, code):
    A, B, m = AM.planted_pair(H, W, 5, code)
    return A, B, m, AM.pushed(m, H, W, code)


@functools.lru_cache(maxsize=None)
def refined(H, W, code, gain, bias):
    A, B, m, m0 = planted(H, W, code)
    return APM.refine(A[None], APM.exposed(B, gain, bias)[None], m0[None], None, code, 3, 4)


@pytest.mark.parametrize("gain,bias", EXPOSURES)
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_a_planted_map_is_recovered_under_a_planted_exposure(oracle, H, W, kind, code, gain, bias):
    A, B, m, m0 = planted(H, W, code)
    model, status, stats, photo = refined(H, W, code, gain, bias)
    start = AM.corner_error(m0, m, H, W)
    err = AM.corner_error(model[0], m, H, W)
    g, b = float(photo[0, 0]), float(photo[0, 1])
    level = abs((g * 128.0 + b) - (gain * 128.0 + bias))
    print(f"{W}x{H} {kind} gain {gain} bias {bias}: corner error {start:.3f} -> {err:.4f} px, g {g:.5f} b {b:.4f}, "
          f"|g 128 + b - planted| {level:.4f}, residual {stats[0, 0]:.4g} -> {stats[0, 1]:.4g}")
    assert status[0] == 1 and stats[0, 3] == 12
    assert err < CORNER_BOUND
    assert level < LEVEL_BOUND
    if (gain, bias) != (1.0, 0.0):
        plain = AM.refine(A[None], APM.exposed(B, gain, bias)[None], m0[None], None, code, 3, 4)
        perr = AM.corner_error(plain[0][0], m, H, W)
        print(f"    the plain statement: status {plain[1][0]}, corner error {perr:.4f} px, residual {plain[2][0, 0]:.4g} -> {plain[2][0, 1]:.4g}")
        assert err < perr / 10.0


def test_the_sums_at_gain_one_and_bias_zero_hold_the_plain_normal_equations(oracle):
    """with g = 1, b = 0 the first NP columns are sd itself, so the geometric block of the photometric sums is the plain
    statement's sums of products byte for byte; the count appears three times"""
    A, B, m, m0 = planted(70, 257, AM.HOMOGRAPHY)
    lv = AM.Level(A, B)
    mm = [np.float64(c) for c in m0]
    plain = AM.sums(lv, mm, AM.HOMOGRAPHY)
    photo = APM.sums_photo(lv, mm, AM.HOMOGRAPHY, 1.0, 0.0)
    assert photo.shape == (67,) and APM.n_sums(AM.HOMOGRAPHY) == 67 and APM.n_sums(AM.AFFINE) == 46
    G = AM.normal_equations(photo, 10)
    assert G[:8, :8].tobytes() == AM.normal_equations(plain, 8)[:, :8].tobytes()
    assert G[9, 9] == photo[-1] == plain[-1]


def test_refused_and_frozen_steps_keep_the_model_and_report_no_exposure(oracle):
    A, B, m, m0 = planted(70, 257, AM.AFFINE)
    one = np.array([1.0, 0.0], np.float32).tobytes()
    bad = m0.copy()
    bad[1] = np.nan
    flat = np.full_like(A, 9.0)
    a, b = np.stack([A, A, flat]), np.stack([B, B, B])
    model, status, stats, photo = APM.refine(a, b, np.stack([m0, bad, m0]), [0, 1, 1], AM.AFFINE, 1, 1)
    assert status.tolist() == [0, 0, 0] and not stats[:2].any() and stats[2, 3] == 0
    assert model[0].tobytes() == m0.tobytes() and model[1].tobytes() == bad.tobytes() and model[2].tobytes() == m0.tobytes()
    assert all(photo[s].tobytes() == one for s in range(3))


def test_a_gain_that_would_not_be_positive_freezes_the_step(oracle):
    """B = 255 - A on a textured pair: the one Gauss-Newton step from g = 1 lands on g' near -1, which the statement refuses;
    the step keeps its model and reports (1, 0)"""
    A, _, m, m0 = planted(70, 257, AM.HOMOGRAPHY)
    ident = AM.IDENTITY[AM.HOMOGRAPHY]
    B = (np.float32(255.0) - A).astype(np.float32)
    lv = AM.Level(A, B)
    S = APM.sums_photo(lv, [np.float64(c) for c in ident], AM.HOMOGRAPHY, 1.0, 0.0)
    q, ok = AM.solve(AM.normal_equations(S, 10), 10)
    print(f"g' = {1.0 + q[8]:.4f}, b' = {q[9]:.3f}")
    assert ok and 1.0 + q[8] <= 0
    model, status, stats, photo = APM.refine(A[None], B[None], ident[None], None, AM.HOMOGRAPHY, 1, 1)
    assert status[0] == 0 and stats[0, 3] == 0 and model[0].tobytes() == ident.tobytes()
    assert photo[0].tobytes() == np.array([1.0, 0.0], np.float32).tobytes()
    assert stats[0, 0] == stats[0, 1]   # nothing moved: before and after are one sum


def test_the_sequence_form_is_the_pair_form(oracle):
    frames, _, _, _ = APM.pan_scene(4, 40, 70)
    model = np.stack([AM.IDENTITY[AM.AFFINE]] * 3)
    model[:, 2] = -4.7
    seq = APM.sequence(frames, model, [1, 0, 1], AM.AFFINE, 2, 2)
    pair = APM.refine(frames[:-1], frames[1:], model, [1, 0, 1], AM.AFFINE, 2, 2)
    APM.same(seq, pair, "sequence against pair")
    assert seq[1].tolist() == [1, 0, 1] and seq[3][1].tolist() == [1.0, 0.0]
