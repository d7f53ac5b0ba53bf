"""BASELINE.json config 5 (7680x4320 pair, 7x7 window, fp16 gradients / accumulators): the opt-in
reduced-precision single-scale mode against the exact result -- on the 13 patterns the exact flow is the CPU ORACLE's
(pinned to the reference by tests/test_oracle_golden.py), so a regression shared by both HIP paths cannot hide.

The reference has no such mode (its arithmetic is fp32, lucas_kanade_core.py:110-133), so the bar is
not equality: SURVEY.md section 7 -- "parity target there is EPE vs fp32 reference REPORTED, not 1e-4".
The endpoint error (EPE) of the fp16 flow against the exact flow is measured per pattern and held to
the tolerances below, which are properties of half precision (11-bit significands in the gradients and
in 49-tap sums), not tuning knobs:

  * well-conditioned pixels (|det| of the exact normal matrix among the upper half of the frame's
    values): mean EPE <= 0.01 px   (measured: <= 0.0042 px over the 13 patterns, 5x5 and 7x7)
  * all pixels: MEDIAN EPE <= 0.01 px (measured: <= 0.0023 px) and MEAN EPE <= 0.02 px (measured: <= 0.0072 px; where
    det ~ 0 the exact flow itself reaches thousands of pixels -- 7078 px on translate_extreme -- and any rounding moves
    it by pixels, so the bound on the mean is a regression gate at ~3x the measured value, not a property of fp16)
  * the mode keeps the reference's border and det-threshold semantics: borders exactly 0.

Those bars are the ACCURACY claim.  The CORRECTNESS claim is the kernel's equality with a stated CPU model of its
arithmetic, oracle/oflk_fp16_model.py (tested on its own in tests/test_fp16_model.py): the kernel's flow has exactly the
model's zero set (the same solve decision per pixel) and is within MODEL_ULP = 2 float32 ulp of it everywhere else --
det and the numerators are identical, and the kernel's v_rcp_f32 is within 1 ulp of the model's IEEE reciprocal.  That
is checked on the 13 patterns at every window and at pixel_max 255 and 1 (fp16 subnormals), at and around the strip
seams, on tiny frames, batches, 8-byte and 4-byte loads, the range scaling's adversarial frames, and the 8K config in
row bands that straddle the launch's segment boundaries.  The EPE bars alone cannot see a seam or lane error: dropping
one column of taps in one column out of every 120 leaves the median at 0 and the well-conditioned mean under its bar.

Numbers of one run are written to gpurun_out/fp16_epe.json (copied to profiles/ by the refresh script).
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest

import oflk_fp16_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PATTERNS = ["translate_small", "translate_medium", "translate_large", "translate_vertical", "translate_diagonal",
            "rotate_small", "rotate_medium", "rotate_large", "zoom_in", "zoom_out", "translate_rotate", "no_motion",
            "translate_extreme"]
TOL_WELL_CONDITIONED_MEAN = 0.01   # px
TOL_MEDIAN = 0.01                  # px
TOL_MEAN_ALL = 0.02                # px: regression gate, ~3x what is measured
MODEL_ULP = 2                      # float32 ulp from oracle/oflk_fp16_model.py outside the (equal) zero set

_report = {}


def _dets(p, c, win):
    """det of the exact (float64) normal matrix per pixel, to tell well- from ill-conditioned windows"""
    from scipy.ndimage import uniform_filter
    from scipy.signal import convolve2d

    avg = (p.astype(np.float64) + c) / 2
    sx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]) / 8.0
    ix = convolve2d(avg, sx, mode="same", boundary="symm")
    iy = convolve2d(avg, sx.T, mode="same", boundary="symm")
    n = win * win
    sxx, syy, sxy = (uniform_filter(q, win, mode="constant") * n for q in (ix * ix, iy * iy, ix * iy))
    return sxx * syy - sxy * sxy


def _epe_stats(p, c, win, exact=None):
    import lucas_kanade_core as K

    u, v = exact if exact is not None else K.lucas_kanade_single_scale(p, c, win)
    hu, hv = K.lucas_kanade_single_scale_fp16(p, c, win, 255.0)
    return epe_of(p, c, win, u, v, hu, hv)


def epe_of(p, c, win, u, v, hu, hv):
    """EPE statistics of an fp16 flow (hu, hv) against the exact flow (u, v) of the pair (p, c); shared with the CPU
    model's accuracy test, tests/test_fp16_model.py"""
    assert np.isfinite(hu).all() and np.isfinite(hv).all()
    hw = win // 2
    # borders: exactly zero, like the reference (lucas_kanade_core.py:101-108)
    for a in (hu, hv):
        assert not a[:hw].any() and not a[-hw:].any() and not a[:, :hw].any() and not a[:, -hw:].any()
    inner = (slice(hw, -hw), slice(hw, -hw))
    epe = np.sqrt((hu.astype(np.float64) - u) ** 2 + (hv.astype(np.float64) - v) ** 2)[inner]
    det = _dets(p, c, win)[inner]
    good = det >= np.median(det)
    return {"mean_epe_all": float(epe.mean()), "median_epe_all": float(np.median(epe)),
            "mean_epe_well_conditioned": float(epe[good].mean()), "p99_epe_well_conditioned": float(np.percentile(epe[good], 99)),
            "max_abs_exact_flow": float(max(np.abs(u).max(), np.abs(v).max()))}


def _assert_model(u, v, mu, mv, ctx):
    """the kernel's flow against the model's: the same zero set, within MODEL_ULP elsewhere (worst case recorded)"""
    assert np.isfinite(mu).all() and np.isfinite(mv).all(), ctx
    zeros, d = M.compare(u, v, mu, mv)
    _report["model_max_ulp"] = max(_report.get("model_max_ulp", 0), d)
    _report["model_cases"] = _report.get("model_cases", 0) + 1
    assert zeros, ("zero set differs from the model", ctx)
    assert d <= MODEL_ULP, ("ulp distance from the model", d, ctx)


def _plan_fp16(p, c, win, pixel_max=255.0, offset=False):
    """[B,H,W] frames through a plan; offset=True hands it pointers one float past 8-byte alignment (4-byte loads)"""
    import torch

    import _oflk

    B, H, W = p.shape
    n = B * H * W
    dev = torch.device("cuda", 0)
    bufs = [torch.full((n + 2,), 7.0, dtype=torch.float32, device=dev) for _ in range(4)]
    o = 1 if offset else 0
    tp, tc, tu, tv = (b[o:o + n].view(B, H, W) for b in bufs)
    tp.copy_(torch.from_numpy(np.ascontiguousarray(p, np.float32)))
    tc.copy_(torch.from_numpy(np.ascontiguousarray(c, np.float32)))
    assert all((t.data_ptr() % 8 == 4) == offset for t in (tp, tc, tu, tv))
    plan = _oflk.Plan(0, B, H, W, 1, win, 0)
    plan.single_scale_fp16(tp.data_ptr(), tc.data_ptr(), tu.data_ptr(), tv.data_ptr(), pixel_max,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    for b in bufs:   # nothing written outside the planes
        assert float(b[:o].sum()) == 7.0 * o and float(b[o + n:].sum()) == 7.0 * (2 - o)
    return tu.cpu().numpy(), tv.cpu().numpy()


def _random_pairs(rng, B, H, W):
    a = rng.integers(0, 256, (B, H, W)).astype(np.float32)
    return a, np.roll(a, (1, -1), (1, 2)) + rng.integers(-3, 4, (B, H, W)).astype(np.float32)


@pytest.fixture(scope="module")
def suite(golden_dir):
    return np.load(golden_dir / "patterns_320x240.npz")


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("win", [7, 5])
def test_fp16_epe_on_the_13_patterns(suite, oracle, name, win):
    p, c = suite["frame_0"].astype(np.float32), suite[f"frame_1__{name}"].astype(np.float32)
    st = _epe_stats(p, c, win, exact=oracle.lucas_kanade_single_scale(p, c, win))   # the oracle's exact flow
    _report[f"{name} {win}x{win}"] = st
    assert st["median_epe_all"] <= TOL_MEDIAN, st
    assert st["mean_epe_well_conditioned"] <= TOL_WELL_CONDITIONED_MEAN, st
    assert st["mean_epe_all"] <= TOL_MEAN_ALL, st


def test_fp16_at_8k_config5():
    """the config as stated: 7680x4320 pair, 7x7 window; crops against the exact path (a full 8K float64
    conditioning map is not needed: the synthetic frames are textured everywhere)"""
    import torch

    import _oflk
    from oflk_synth import synth_pair

    H, W, win = 4320, 7680, 7
    p, c = synth_pair(H, W, 0)
    dev = torch.device("cuda", 0)
    tp, tc = torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev)
    u, v, hu, hv = (torch.empty_like(tp) for _ in range(4))
    plan = _oflk.Plan(0, 1, H, W, 1, win, 0)
    st = torch.cuda.current_stream().cuda_stream
    plan.single_scale(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    plan.single_scale_fp16(tp.data_ptr(), tc.data_ptr(), hu.data_ptr(), hv.data_ptr(), 255.0, st)
    torch.cuda.synchronize()
    assert torch.isfinite(hu).all() and torch.isfinite(hv).all()
    epe = torch.sqrt((hu.double() - u.double()) ** 2 + (hv.double() - v.double()) ** 2)[3:-3, 3:-3]
    stats = {"mean_epe_all": float(epe.mean()), "median_epe_all": float(epe.median()),
             "p99_epe_all": float(torch.quantile(epe.flatten()[::97].float(), 0.99))}
    # timing, inputs resident: the figure profiles/<tag>_configs.json carries
    for fn, key in ((plan.single_scale, "exact_fp32_us"), (plan.single_scale_fp16, "fp16_us")):
        args = (tp.data_ptr(), tc.data_ptr(), hu.data_ptr(), hv.data_ptr()) + ((255.0, st) if key == "fp16_us" else (st,))
        for _ in range(3):
            fn(*args)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn(*args)
        e1.record()
        torch.cuda.synchronize()
        stats[key] = round(e0.elapsed_time(e1) / 20 * 1e3, 1)
    stats["fp16_GBs_algorithmic"] = round(16.0 * H * W / stats["fp16_us"] / 1e3, 1)
    _report["8K 7x7 synthetic"] = stats
    plan.close()
    assert stats["median_epe_all"] <= TOL_MEDIAN, stats


def test_fp16_other_windows_and_ragged_shapes():
    import lucas_kanade_core as K

    rng = np.random.default_rng(4)
    for (H, W) in ((37, 53), (64, 64), (5, 300), (131, 70)):
        a = rng.integers(0, 256, (H, W)).astype(np.float32)
        b = np.roll(a, (1, 1), (0, 1))
        for win in (3, 5, 7, 9, 11):
            u, v = K.lucas_kanade_single_scale(a, b, win)
            hu, hv = K.lucas_kanade_single_scale_fp16(a, b, win)
            assert hu.shape == (H, W) and np.isfinite(hu).all() and np.isfinite(hv).all()
            if min(H, W) > win:
                epe = np.sqrt((hu - u) ** 2 + (hv - v) ** 2)
                assert np.median(epe) <= 0.1, (H, W, win, float(np.median(epe)))
            _assert_model(hu, hv, *M.fp16_flow(a, b, win), ("ragged", H, W, win))


def test_fp16_strip_and_segment_seams():
    """the streaming kernel cuts the frame into strips of 128 - 4 ceil(R/2) columns and segments of Hs rows (Hs follows
    from the frame height and the batch size): widths around the strip seams, several pairs per call, and the same
    frames with 17 / 40 more rows appended (the segments are then cut at other rows) give the same flow wherever the
    window does not see the difference -- the arithmetic per pixel does not depend on the cut"""
    import torch

    import _oflk

    rng = np.random.default_rng(11)
    dev = torch.device("cuda", 0)
    # two columns per lane: strips of 124 (3x3), 120 (5x5, 7x7), 116 (9x9, 11x11) columns
    for (B, H, W, win) in ((2, 90, 56, 7), (1, 77, 113, 7), (3, 41, 58 * 3 + 1, 5), (1, 200, 129, 3), (2, 60, 241, 7), (1, 50, 121, 7),
                           (1, 64, 250, 11), (2, 33, 117, 9), (1, 45, 375, 3), (1, 700, 130, 7)):
        hw = win // 2
        a = rng.integers(0, 256, (B, H + 40, W)).astype(np.float32)
        b = np.roll(a, (1, -1), (1, 2))
        outs = []
        for extra in (0, 17, 40):
            Hx = H + extra
            ta = torch.from_numpy(np.ascontiguousarray(a[:, :Hx])).to(dev)
            tb = torch.from_numpy(np.ascontiguousarray(b[:, :Hx])).to(dev)
            u, v = torch.full_like(ta, 7.0), torch.full_like(ta, 7.0)
            plan = _oflk.Plan(0, B, Hx, W, 1, win, 0)
            plan.single_scale_fp16(ta.data_ptr(), tb.data_ptr(), u.data_ptr(), v.data_ptr(), 255.0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            plan.close()
            outs.append((u.cpu().numpy(), v.cpu().numpy()))
        keep = H - hw - 1   # rows whose window and Sobel ring lie inside the shortest frame
        for u, v in outs[1:]:
            assert np.array_equal(u[:, :keep], outs[0][0][:, :keep]) and np.array_equal(v[:, :keep], outs[0][1][:, :keep]), (B, H, W, win)
        u0 = outs[0][0]
        assert not u0[:, :hw].any() and not u0[:, -hw:].any() and not u0[:, :, :hw].any() and not u0[:, :, -hw:].any()


@pytest.mark.parametrize("pixel_max", [255.0, 1.0])
@pytest.mark.parametrize("win", [3, 5, 7, 9, 11])
def test_fp16_equals_model_on_the_13_patterns(suite, win, pixel_max):
    """pixel_max 1: the patterns divided by 255, k = 0 -- the products and sums are fp16 subnormals"""
    scale = np.float32(255.0 / pixel_max)
    for name in PATTERNS:
        p = suite["frame_0"].astype(np.float32) / scale
        c = suite[f"frame_1__{name}"].astype(np.float32) / scale
        u, v = _plan_fp16(p[None], c[None], win, pixel_max)
        _assert_model(u[0], v[0], *M.fp16_flow(p, c, win, pixel_max), (name, win, pixel_max))


@pytest.mark.parametrize("win", [3, 5, 7, 9, 11])
def test_fp16_equals_model_at_strip_seams_and_tiny_frames(win):
    """widths n OUTW + {-1, 0, 1, 2} (a strip seam at, just before and just after the edge), widths below one strip, and
    frames of 1, 2, 3 and 2HW pixels a side (all zero unless a full window fits)"""
    hw = win // 2
    outw = M.strip_width(win)
    assert outw == 2 * (64 - 2 * -(-(hw + 1) // 2))
    rng = np.random.default_rng(20 + win)
    H = 4 * win + 3
    widths = sorted({n * outw + d for n in (1, 2, 3) for d in (-1, 0, 1, 2)} | {1, 2, 3, 2 * hw, win + 1, outw // 2 + 1, outw - 2})
    for W in widths:
        p, c = _random_pairs(rng, 1, H, W)
        u, v = _plan_fp16(p, c, win)
        _assert_model(u, v, *M.fp16_flow(p, c, win), ("seams", win, H, W))
    for H in (1, 2, 3, 2 * hw):
        for W in (1, 2, 3, 2 * hw):
            p, c = _random_pairs(rng, 1, H, W)
            u, v = _plan_fp16(p, c, win)
            if min(H, W) <= 2 * hw:   # no full window (3x3 at H = W = 3 has one)
                assert not u.any() and not v.any(), (win, H, W)
            _assert_model(u, v, *M.fp16_flow(p, c, win), ("tiny", win, H, W))


@pytest.mark.parametrize("win", [5, 7, 11])
def test_fp16_batches_equal_model_per_pair(win):
    """B = 1 .. 5 distinct pairs in one launch (the segment height follows from B): every pair equals the model"""
    rng = np.random.default_rng(30 + win)
    H, W = 157, 251
    for B in range(1, 6):
        p, c = _random_pairs(rng, B, H, W)
        u, v = _plan_fp16(p, c, win)
        hs = M.segment_rows(B, H, W, win)
        for b in range(B):
            _assert_model(u[b], v[b], *M.fp16_flow(p[b], c[b], win), ("batch", win, B, b, hs))


@pytest.mark.parametrize("win", [3, 5, 7, 9, 11])
def test_fp16_vector_and_scalar_loads_equal_model(suite, win):
    """even widths take 8-byte column-pair loads from 8-byte-aligned planes and 4-byte loads otherwise: the same frames
    through both must equal the model"""
    rng = np.random.default_rng(40 + win)
    outw = M.strip_width(win)
    cases = [_random_pairs(rng, 2, 45, outw + 2), _random_pairs(rng, 1, 37, 2 * outw),
             (suite["frame_0"].astype(np.float32)[None], suite["frame_1__zoom_in"].astype(np.float32)[None])]
    for p, c in cases:
        m = M.fp16_flow(p, c, win)
        for offset in (False, True):
            u, v = _plan_fp16(p, c, win, offset=offset)
            _assert_model(u, v, *m, ("loads", win, p.shape, offset))


@pytest.mark.parametrize("pixel_max", [1.0, 255.0, 1023.0, 4095.0, 65535.0])
@pytest.mark.parametrize("win", [3, 5, 7, 9, 11])
def test_fp16_range_frames_equal_model(win, pixel_max):
    """the adversarial frames of tests/test_fp16_model.py (|Ix|, |Iy|, |It| at the scaling rule's bound), one launch"""
    from test_fp16_model import range_frames

    frames = range_frames(pixel_max)
    p = np.stack([a for a, _ in frames.values()])
    c = np.stack([b for _, b in frames.values()])
    u, v = _plan_fp16(p, c, win, pixel_max)
    assert np.isfinite(u).all() and np.isfinite(v).all()
    mu, mv = M.fp16_flow(p, c, win, pixel_max)
    for b, name in enumerate(frames):
        _assert_model(u[b], v[b], mu[b], mv[b], ("range", win, pixel_max, name))


def test_fp16_at_8k_config5_equals_model_in_bands():
    """BASELINE config 5 (7680x4320, 7x7): finite everywhere, and equal to the model in row bands -- the top and bottom
    edges and bands across the launch's segment boundaries (multiples of Hs)"""
    import torch

    import _oflk
    from oflk_synth import synth_pair

    H, W, win = 4320, 7680, 7
    p, c = synth_pair(H, W, 0)
    dev = torch.device("cuda", 0)
    tp, tc = torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev)
    hu, hv = torch.empty_like(tp), torch.empty_like(tp)
    plan = _oflk.Plan(0, 1, H, W, 1, win, 0)
    plan.single_scale_fp16(tp.data_ptr(), tc.data_ptr(), hu.data_ptr(), hv.data_ptr(), 255.0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    assert torch.isfinite(hu).all() and torch.isfinite(hv).all()
    hs = M.segment_rows(1, H, W, win)
    assert 8 <= hs < H // 4, hs
    bands = [(0, 40), (H - 40, H)] + [(m * hs - 20, m * hs + 20) for m in (1, (H // hs) // 2, H // hs - 1)]
    for y0, y1 in bands:
        mu, mv = M.fp16_flow(p, c, win, rows=(y0, y1))
        _assert_model(hu[y0:y1].cpu().numpy(), hv[y0:y1].cpu().numpy(), mu, mv, ("8K", y0, y1, hs))


def test_fp16_host_entry_batched_equals_plan():
    """oflk_single_scale_fp16 with B > 1 (host frames) returns what the plan path returns, and the model's flow"""
    import _oflk

    rng = np.random.default_rng(50)
    B, H, W, win = 3, 70, 131, 5
    p, c = _random_pairs(rng, B, H, W)
    u, v = np.empty_like(p), np.empty_like(p)
    _oflk.check(_oflk.lib().oflk_single_scale_fp16(_oflk.ptr(p), _oflk.ptr(c), B, H, W, win, 255.0, _oflk.ptr(u), _oflk.ptr(v)))
    pu, pv = _plan_fp16(p, c, win)
    assert np.array_equal(u, pu) and np.array_equal(v, pv)
    _assert_model(u, v, *M.fp16_flow(p, c, win), ("host", B, H, W))


def test_zz_write_report():
    out = ROOT / "gpurun_out"
    out.mkdir(exist_ok=True)
    (out / "fp16_epe.json").write_text(json.dumps({"tolerances_px": {"median_all": TOL_MEDIAN,
                                                                      "mean_well_conditioned": TOL_WELL_CONDITIONED_MEAN},
                                                   "reference_for_epe": "exact fp32 path (equal to the Python reference value for value)",
                                                   "rows": _report}, indent=1))
    assert _report
