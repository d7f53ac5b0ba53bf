"""GPU tests of the early-exit band (run on an MI355X: python -m pytest tests -m gpu -x -q).

The library flags an exit decision when the level's device mean |d| lies within decision_guard of 0.01, and promises that 0
flags mean "provably the reference's iteration counts" (include/oflk.h, oflk_plan_read_uncertain).  That rests on two
bounds against the EXACT mean of the same d (oracle exact_mean_abs: an exact sum, one fp64 division):
  * NumPy's fp32 pairwise np.mean:  |NumPy - exact| <= numpy_mean_error(n) x exact;
  * the device's total of partial sums rounded to a 2^-20 grid:  |device - exact| <= E_dev(path, level, exact) x exact;
and on the band covering both.  Here every logged mean of every mode (exact, contracted, tolerant), frame type, window path
(tiled 3 / 5 / 7, one generic window) and size (ragged and tiny levels up to one 7680x4320 level) is held to both bounds;
means placed by bisection just inside and just outside the band are flagged or not as they must be; and the bench workload's
1080p pairs are flagged nowhere, so the widened band costs the workload no exact redo.
"""
import os

import numpy as np
import pytest

from test_tolerant_model import SUM_HOST, decision_guard, device_mean_error, level_sum_path, numpy_mean_error

pytestmark = pytest.mark.gpu

THR = float(np.float32(0.01))
ARITH = {"exact": 0, "contracted": 1, "tolerant": 2}


@pytest.fixture(scope="module")
def threaded_oracle(oracle):
    oracle.set_threads(min(oracle.max_threads(), len(os.sched_getaffinity(0)), 16))
    yield oracle
    oracle.set_threads(1)


def _frames(kind, H, W, seed):
    from oflk_synth import synth_pair, synth_pair_smooth

    rng = np.random.default_rng(seed)
    if kind == "synth":
        return synth_pair(H, W, seed)
    if kind == "noise":
        a = rng.integers(0, 256, (H, W)).astype(np.float32)
        b = np.roll(a, (1, 2), axis=(0, 1)) + rng.integers(-6, 7, (H, W)).astype(np.float32)
        return a, np.clip(b, 0, 255).astype(np.float32)
    if kind == "smooth":   # a sub-pixel shift of a smooth image: most |d| far below 2^-21 after the first iteration
        return synth_pair_smooth(H, W, seed, 2e-5, -1e-5)
    if kind == "outlier":  # near-zero |d| everywhere but around one bright pixel
        p, c = synth_pair_smooth(H, W, seed, 1e-6, 0.0)
        c = c.copy()
        c[H // 2, W // 3] += 120.0
        return p, c
    raise ValueError(kind)


def _run(plan, p, c, u8=False):
    """device-resident run of a batch; (u, v, log, runs, flags) on the host"""
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    if u8:
        p, c = np.rint(p).clip(0, 255).astype(np.uint8), np.rint(c).clip(0, 255).astype(np.uint8)
    tp, tc = torch.from_numpy(np.ascontiguousarray(p)).to(dev), torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    u = torch.empty(p.shape, dtype=torch.float32, device=dev)
    v = torch.empty_like(u)
    (plan.pyramidal_u8 if u8 else plan.pyramidal)(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    log, runs = plan.read_log(st)
    flags = plan.read_uncertain(st)
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy(), log, runs, flags


def _reference(oracle, mode, p, c, L, K, window):
    """(u, v, NumPy-order log, runs, exact log) of what the device computes in `mode`: the oracle (exact), the CPU model of
    the contracted / tolerant arithmetic otherwise"""
    import oflk_tolerant_model as M

    if mode == "exact":
        return oracle.lucas_kanade_pyramidal_ex(p, c, L, window, K, exact_means=True)
    spec = M.contracted_spec(L, K) if mode == "contracted" else M.tolerant_spec(L, K, p.shape, window)
    return M.pyramidal(p, c, spec, window, exact_means=True)


def assert_means_within_bounds(log, nplog, xlog, runs, dims, paths, what):
    """every executed (level, iteration, axis): |device - exact| <= E_dev x exact, |NumPy - exact| <= NumPy's bound x exact,
    and the library's band at that level >= NumPy's bound + E_dev at 0.01.  Returns how many means were checked."""
    import _oflk

    L = _oflk.lib()
    checked = 0
    for l, (h, w) in enumerate(dims):
        path = paths[l]
        g = L.oflk_decision_guard(path, h, w)
        assert g == pytest.approx(decision_guard(path, h, w), rel=1e-12, abs=0), (what, l)
        if path != SUM_HOST:
            assert g >= numpy_mean_error(h * w) + device_mean_error(path, h, w, THR), (what, l, g)
        for k in range(int(runs[l])):
            for ax in range(2):
                x, d, n = float(xlog[l, k, ax]), float(log[l, k, ax]), float(nplog[l, k, ax])
                e_dev = L.oflk_device_mean_error(path, h, w, x) if x > 0 else 0.0
                assert abs(d - x) <= e_dev * x, f"{what}: level {l} ({h}x{w}) iter {k} axis {ax}: device {d!r}, exact {x!r}, " \
                                                f"{abs(d - x) / max(x, 1e-300):.3e} > E_dev {e_dev:.3e}"
                assert abs(n - x) <= numpy_mean_error(h * w) * x, f"{what}: level {l} iter {k} axis {ax}: NumPy {n!r}, exact {x!r}"
                checked += 1
    return checked


def _case(oracle, H, W, L, K, window, mode, kind, u8=False, batch=None, seed=0):
    import _oflk

    if batch is None:
        p, c = _frames(kind, H, W, seed)
        if u8:
            p, c = np.rint(p).clip(0, 255).astype(np.float32), np.rint(c).clip(0, 255).astype(np.float32)
        batch = [(p, c)]
    P = np.stack([b[0] for b in batch])
    C = np.stack([b[1] for b in batch])
    plan = _oflk.Plan(0, len(batch), H, W, L, window, K)
    try:
        plan.set_arithmetic(ARITH[mode])
        u, v, log, runs, flags = _run(plan, P, C, u8)
    finally:
        plan.close()
    dims = oracle.pyramid_dims(H, W, L)
    paths = [level_sum_path(ARITH[mode], L, K, window, dims, l) for l in range(L)]
    checked = 0
    for b in range(len(batch)):
        what = f"{mode} {H}x{W} L={L} K={K} win={window} {kind}{' u8' if u8 else ''} pair {b}"
        ru, rv, nplog, rruns, xlog = _reference(oracle, mode, P[b], C[b], L, K, window)
        assert not flags[b].any(), (what, flags[b])
        assert list(runs[b]) == list(rruns), (what, runs[b], rruns)
        assert np.array_equal(u[b], ru) and np.array_equal(v[b], rv), f"{what}: flow differs from its reference (not the same d)"
        if paths[0] == SUM_HOST:   # NumPy's own order on the host: the logged means ARE NumPy's
            assert np.array_equal(log[b][:, :K], nplog), what
        checked += assert_means_within_bounds(log[b], nplog, xlog, rruns, dims, paths, what)
    return checked


# ---------------------------------------------------------------------------------------------------------------
# every logged mean within both bounds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "contracted", "tolerant"])
def test_pattern_means_within_both_bounds(threaded_oracle, golden_dir, mode):
    """the 13 verification patterns (320x240, one batch), float32 and uint8 frames"""
    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    batch = [(z["frame_0"].astype(np.float32), z[f"frame_1__{n}"].astype(np.float32)) for n in names]
    n = 0
    for u8 in (False, True):
        n += _case(threaded_oracle, 240, 320, 3, 3, 5, mode, "patterns", u8=u8, batch=batch)
    assert n >= 2 * 13 * 3 * 2


@pytest.mark.parametrize("window", [3, 7, 13])
def test_other_windows_means_within_both_bounds(threaded_oracle, golden_dir, window):
    """the tiled 3x3 and 7x7 windows (k_lkw) and one generic window (13x13: NumPy's own mean on the host)"""
    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")][:4 if window == 13 else 13]
    batch = [(z["frame_0"].astype(np.float32), z[f"frame_1__{n}"].astype(np.float32)) for n in names]
    if window == 13:
        batch = [(p[::2, ::2].copy(), c[::2, ::2].copy()) for p, c in batch]
    H, W = batch[0][0].shape
    for mode in ("exact", "tolerant"):
        assert _case(threaded_oracle, H, W, 3, 3, window, mode, "patterns", batch=batch) > 0


@pytest.mark.parametrize("shape,L", [((241, 323), 4), ((97, 131), 4), ((23, 21), 3), ((33, 250), 4), ((64, 48), 3)])
@pytest.mark.parametrize("kind", ["synth", "noise", "smooth", "outlier"])
def test_ragged_and_tiny_means_within_both_bounds(threaded_oracle, shape, L, kind):
    """ragged shapes whose coarsest level is a few pixels, every content kind, every mode (tolerant in two envelope cells)"""
    H, W = shape
    for mode, (LL, K) in (("exact", (L, 3)), ("contracted", (L, 3)), ("tolerant", (3, 3)), ("tolerant", (1, 2))):
        _case(threaded_oracle, H, W, LL, K, 5, mode, kind, seed=H + W)
    _case(threaded_oracle, H, W, L, 3, 5, "exact", kind, u8=True, seed=H + W)


@pytest.mark.parametrize("kind", ["synth", "smooth", "outlier"])
def test_1080p_means_within_both_bounds(threaded_oracle, kind):
    for mode in ("exact", "tolerant"):
        _case(threaded_oracle, 1080, 1920, 3, 3, 5, mode, kind)
    _case(threaded_oracle, 1080, 1920, 3, 3, 5, "tolerant", kind, u8=True)


def test_4k_means_within_both_bounds(threaded_oracle):
    for mode in ("exact", "tolerant"):
        _case(threaded_oracle, 2160, 3840, 3, 3, 5, mode, "synth")


def test_8k_single_level_means_within_both_bounds(threaded_oracle):
    """7680x4320 at levels = 1: NumPy's bound alone is 2.43e-4 there, the band is that plus E_dev"""
    for mode in ("exact", "tolerant"):
        _case(threaded_oracle, 4320, 7680, 1, 2, 5, mode, "synth")


# ---------------------------------------------------------------------------------------------------------------
# constructed near-threshold decisions, where the band is tightest
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,L,mode", [(48, 64, 2, "exact"), (240, 320, 1, "exact"), (240, 320, 1, "tolerant"),
                                        (4320, 7680, 1, "exact")])
def test_near_threshold_decisions_flagged_as_the_bounds_say(threaded_oracle, H, W, L, mode):
    """curr = prev + t (shifted - prev), t bisected so that the EXACT mean of the first decision of level 0 (768 px, a
    320x240 level, the single 8K level) sits at a chosen offset from 0.01.  Just inside NumPy's bound + E_dev (at +-S/2):
    flagged, and after oflk_plan_resolve_uncertain the flow and the iteration counts are the oracle's bit for bit.  Outside
    the band (at +-2 x band): not flagged, with the reference's counts.  Small levels are bisected on the exact mean itself;
    the 8K level on the device's mean (the CPU oracle is slow there), then checked on the exact mean."""
    import torch

    import _oflk
    from oflk_synth import synth_pair

    oracle = threaded_oracle
    K = 2
    h, w = oracle.pyramid_dims(H, W, L)[0]
    path = level_sum_path(ARITH[mode], L, K, 5, oracle.pyramid_dims(H, W, L), 0)
    S = numpy_mean_error(h * w) + device_mean_error(path, h, w, THR)
    g = float(_oflk.lib().oflk_decision_guard(path, h, w))
    assert g >= S
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, 1, H, W, L, 5, K)
    plan.set_arithmetic(ARITH[mode])
    small = h * w <= 1_000_000

    def place(seed, off):
        """(prev, curr, exact mean, reference) with the first decision's exact mean bisected onto THR (1 + off)"""
        prev, shifted = synth_pair(H, W, seed, dx=0.75, dy=-0.5)
        delta = (shifted - prev).astype(np.float64)
        frames = lambda t: (prev + t * delta).astype(np.float32)  # noqa: E731
        d_prev = torch.from_numpy(prev[None]).to(dev)

        def exact(t):
            r = _reference(oracle, mode, prev, frames(t), L, K, 5)
            return float(max(r[4][0, 0])), r

        def device_mean(t):
            d_curr = torch.from_numpy(frames(t)[None]).to(dev)
            plan.pyramidal(d_prev.data_ptr(), d_curr.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
            log, _ = plan.read_log(st)
            return float(max(log[0, 0, 0]))

        mean = (lambda t: exact(t)[0]) if small else device_mean
        target = THR * (1.0 + off)
        lo, hi = 0.0, 1.0
        assert mean(lo) < target < mean(hi)
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if mean(mid) < target:
                lo = mid
            else:
                hi = mid
        t = min((lo, hi), key=lambda e: abs(mean(e) - target))   # the end nearer the target
        x, ref = exact(t)
        return prev, frames(t), x, ref

    d_u = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    d_v = torch.empty_like(d_u)
    try:
        # inside: the exact offset within (0, S) / (-S, 0); outside: within 1.5 ... 2.5 x the band, either side.  A level of a
        # few hundred pixels moves its mean in steps comparable to S (one float32 pixel value flipping), so several pairs are
        # tried until one lands.
        for off, inside in ((0.5 * S, True), (-0.5 * S, True), (2.0 * g, False), (-2.0 * g, False)):
            ok = (lambda r: 0.0 < r * np.sign(off) < S) if inside else (lambda r: 1.5 * g <= abs(r) <= 2.5 * g)
            tried = []
            for seed in range(16 if small else 2):
                prev, curr, x, ref = place(seed, off)
                tried.append(x / THR - 1.0)
                if ok(tried[-1]):
                    break
            rel = tried[-1]
            tag = f"{mode} {h}x{w}: target offset {off:+.3e}, exact mean offset {rel:+.3e} (S {S:.3e}, band {g:.3e})"
            assert ok(rel), f"{tag}: no pair landed in the window; offsets reached {['%.2e' % r for r in tried]}"
            d_prev = torch.from_numpy(prev[None]).to(dev)
            d_curr = torch.from_numpy(curr[None]).to(dev)
            plan.pyramidal(d_prev.data_ptr(), d_curr.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
            log, runs = plan.read_log(st)
            flags = plan.read_uncertain(st)[0]
            m = float(max(log[0, 0, 0]))
            assert abs(m - x) <= device_mean_error(path, h, w, x) * x, tag
            if inside:
                assert flags[0] & 1, tag + ": not flagged"
                n = plan.resolve_uncertain(d_prev.data_ptr(), d_curr.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
                torch.cuda.synchronize()
                assert n == 1, tag
                ou, ov, _, oruns = ref[:4] if mode == "exact" else oracle.lucas_kanade_pyramidal_ex(prev, curr, L, 5, K)
                log, runs = plan.read_log(st)
                assert list(runs[0]) == list(oruns), (tag, runs, oruns)
                assert np.array_equal(d_u[0].cpu().numpy(), ou) and np.array_equal(d_v[0].cpu().numpy(), ov), tag
                assert not plan.read_uncertain(st).any(), tag
            else:
                assert not flags[0] & 1, tag + ": flagged outside the band"
                assert list(runs[0]) == list(ref[3]), (tag, runs, ref[3])
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# the cost of the band on the bench workload
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "tolerant"])
def test_bench_pairs_are_never_flagged(mode):
    """bench.py's default workload -- 1080p, 3 levels, 3 iterations, 5x5, its distinct synthetic pairs tiled over a batch --
    flags no pair in the exact or the tolerant mode: the band (5e-5 at 1080p) costs it no exact redo"""
    import _oflk
    from oflk_synth import synth_pair

    H, W, B = 1080, 1920, 8
    host = [synth_pair(H, W, pair_index=i) for i in range(4)]
    P = np.stack([host[b % 4][0] for b in range(B)])
    C = np.stack([host[b % 4][1] for b in range(B)])
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    try:
        plan.set_arithmetic(ARITH[mode])
        _, _, log, runs, flags = _run(plan, P, C)
    finally:
        plan.close()
    assert int(flags.astype(bool).sum()) == 0, flags
    assert (runs >= 1).all()
