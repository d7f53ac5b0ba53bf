"""CPU tests of the forward-backward consistency statement (tests/fb_model.py), of its input checks and of the new C ABI
surface.  Nothing here touches a device."""
import re
from pathlib import Path

import numpy as np
import pytest

import fb_model as M

ROOT = Path(__file__).resolve().parents[1]
FB_SYMBOLS = ["oflk_plan_pyramidal_sequence_fb", "oflk_plan_pyramidal_sequence_fb_u8", "oflk_plan_read_log_backward",
              "oflk_plan_read_uncertain_backward", "oflk_plan_resolve_uncertain_sequence_fb",
              "oflk_plan_resolve_uncertain_sequence_fb_u8", "oflk_fb_consistency", "oflk_fb_consistency_host",
              "oflk_pyramidal_sequence_fb", "oflk_pyramidal_sequence_fb_u8"]


@pytest.mark.parametrize("shift", [(2, 0), (-3, 1), (0, -2), (5, 4)])
def test_opposite_integer_shifts_are_consistent(shift):
    """F = -G = a constant whole-pixel shift: the sampled backward vector is exactly -F, so err = 0 wherever the target is
    inside, and err = |F| (target outside: warp_image samples 0) elsewhere"""
    H, W = 17, 23
    dx, dy = shift
    uf, vf = np.full((H, W), dx, np.float32), np.full((H, W), dy, np.float32)
    ef, eb, qf, qb = M.fb_check(uf, vf, -uf, -vf)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for e, q, sx, sy in ((ef, qf, dx, dy), (eb, qb, -dx, -dy)):
        inside = (xx + sx >= 0) & (xx + sx <= W - 1) & (yy + sy >= 0) & (yy + sy <= H - 1)
        assert (e[inside] == 0).all()
        assert np.array_equal(e[~inside], np.full((~inside).sum(), np.float32(np.hypot(dx, dy))))
        assert np.array_equal(q.astype(bool), inside)


@pytest.mark.parametrize("W", [1, 2, 7])
def test_inside_follows_the_stated_closed_interval(W):
    """targets x + u in {-0.5, 0, W-1, W-0.75}: inside exactly for 0 and W-1 (closed interval), in both directions"""
    H = 3
    for target, want in ((-0.5, False), (0.0, True), (W - 1.0, True), (W - 0.75, False)):
        xx = np.arange(W, dtype=np.float64)[None, :].repeat(H, 0)
        u = (target - xx).astype(np.float32)
        assert np.array_equal(xx + u.astype(np.float64), np.full((H, W), target))   # the offsets are exact
        z = np.zeros((H, W), np.float32)
        _, _, qf, qb = M.fb_check(u, z, u, z, alpha=1e6, beta=1e6)   # the magnitude test always passes
        assert (qf.astype(bool) == want).all(), (W, target)
        assert (qb.astype(bool) == want).all(), (W, target)


def test_zero_flows_are_valid_when_beta_is_positive():
    z = np.zeros((2, 9, 11), np.float32)
    for alpha, beta in ((0.01, 0.5), (0.0, 1e-30), (0.05, 1e6)):
        ef, eb, qf, qb = M.fb_check(z, z, z, z, alpha, beta)
        assert (qf == 1).all() and (qb == 1).all() and (ef == 0).all() and (eb == 0).all()
    _, _, qf, qb = M.fb_check(z, z, z, z, 0.01, 0.0)   # 0 <= 0: still valid at beta = 0
    assert (qf == 1).all() and (qb == 1).all()


def test_alpha_beta_and_inputs_are_checked_before_any_device():
    """ValueError from the Python layer itself: these calls never reach the library's compute path"""
    import _oflk
    import flow_metrics
    import lucas_kanade_pyramidal as P

    f = np.zeros((3, 16, 16), np.float32)
    for alpha, beta in ((-0.01, 0.5), (0.01, -1.0), (float("nan"), 0.5), (0.01, float("inf")), (1e300, 0.5)):
        with pytest.raises(ValueError):
            _oflk.check_fb_params(alpha, beta)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_fb(f, alpha=alpha, beta=beta)
        with pytest.raises(ValueError):
            flow_metrics.forward_backward_consistency(f[0], f[0], f[0], f[0], alpha, beta)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_fb(f[:1])
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_fb([f[0], f[0, :8]])
    with pytest.raises(ValueError):
        flow_metrics.forward_backward_consistency(f[0], f[0], f[0], f[0, :8])
    with pytest.raises(ValueError):
        flow_metrics.forward_backward_consistency(f[0, 0], f[0, 0], f[0, 0], f[0, 0])
    with pytest.raises(ValueError):   # a B mismatch
        flow_metrics.forward_backward_consistency(f[:2], f[:2], f, f)


def test_new_symbols_are_declared_and_exported():
    import _oflk

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oflk.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oflk_[a-z0-9_]+)\s*\(", text))
    L = _oflk.lib()
    for name in FB_SYMBOLS:
        assert name in declared, f"{name} not declared in include/oflk.h"
        assert hasattr(L, name), f"{name} not exported by liboflk.so"
        assert name in _oflk.SIGNATURES


def test_model_scene_calibration():
    """the occluder scene of the GPU meaning test, on the oracle's flows: most of the covered background strip fails the
    forward test and most pixels far from the square's boundaries pass (thresholds of tests/test_gpu_fb.py)"""
    import oflk_oracle as O

    H, W, S, step = 96, 128, 36, (3, 1)
    frames, corners = M.occluder_scene(3, H, W, S, step)
    for t in range(2):
        uf, vf = O.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3)
        ub, vb = O.lucas_kanade_pyramidal(frames[t + 1], frames[t], 3, 5, 3)
        _, _, qf, _ = M.fb_check(uf, vf, ub, vb)
        covered, far = M.scene_regions(corners, t, H, W, S, step, 6)
        assert covered.sum() > 100 and far.sum() > 5000
        assert qf[covered].mean() <= 0.35, qf[covered].mean()
        assert qf[far].mean() >= 0.85, qf[far].mean()
