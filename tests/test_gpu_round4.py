"""GPU tests added in round 4 (run on an MI355X: python -m pytest tests -m gpu -x -q).

  * the opt-in within-tolerance arithmetic (OFLK_ARITH_TOLERANT, include/oflk.h), below
  * single-scale 5x5 through the streaming kernel: exact on 8-bit frames, doubtful tiles redone in NumPy's order
  * oflk_*_multi: chunks of pairs pulled from a shared counter
  * bench.py --gather: the flow shards to rank 0 through RCCL, reported next to the throughput

The within-tolerance arithmetic:

Two links, each sharp on its own:
  * HIP == CPU model, bit for bit: oracle/oflk_tolerant_model.c states the tolerant mode's arithmetic operation for operation
    (fused multiply-adds in the pyramid and in the warp's three lerps, window sums vertical-then-horizontal on the two
    finest levels); the kernels reproduce it on every shape tried here -- so the mode has no arithmetic of its own to trust.
  * model (hence HIP) vs THE REFERENCE: mean endpoint error <= 1e-4 (BASELINE.json north_star) against dense flows the
    reference itself produced (tests/golden/dense_reference_flows.npz, made by make_golden_dense.py importing it): all 13
    verification patterns and pair 0 of the bench workload at 1920x1080.
The default (exact) mode is untouched: switching back gives the exact digests again.
"""
import json
from pathlib import Path

import numpy as np
import oflk_oracle as O
import pytest
from test_tolerant_model import assert_log_within_bounds, level_sum_path

pytestmark = pytest.mark.gpu

TOL = 1e-4   # mean endpoint error against the reference's flow, px (north_star)


def _epe(u, v, ru, rv):
    return float(np.mean(np.sqrt((u.astype(np.float64) - ru) ** 2 + (v.astype(np.float64) - rv) ** 2)))


def _run(plan, p, c, u8=False):
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    tp, tc = torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev)
    u = torch.empty(p.shape, dtype=torch.float32, device=dev)
    v = torch.empty_like(u)
    (plan.pyramidal_u8 if u8 else plan.pyramidal)(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    log, runs = plan.read_log(st)
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy(), log, runs


def _model(p, c, L, K, exact_means=False):
    import oflk_tolerant_model as M

    return M.pyramidal(p.astype(np.float32), c.astype(np.float32), M.tolerant_spec(L, K, p.shape), 5, exact_means=exact_means)


def _pair(rng, H, W, kind):
    from oflk_synth import synth_pair, synth_pair_smooth

    if kind == "synth":
        return synth_pair(H, W, int(rng.integers(0, 1000)))
    if kind == "smooth":
        return synth_pair_smooth(H, W, int(rng.integers(0, 1000)))
    a = rng.integers(0, 256, (H, W)).astype(np.float32)
    b = np.roll(a, (1, 2), axis=(0, 1)) + rng.integers(-6, 7, (H, W)).astype(np.float32)
    return a, np.clip(b, 0, 255).astype(np.float32)


@pytest.mark.parametrize("shape", [(240, 320), (241, 323), (97, 131), (64, 48), (33, 250), (480, 644), (270, 480), (23, 21)])
@pytest.mark.parametrize("kind", ["synth", "noise", "smooth"])
def test_tolerant_kernels_equal_their_cpu_model(shape, kind):
    """flows, residual log and iteration counts of a tolerant plan == the CPU model's, value for value: even and odd widths
    (the 8-byte and the element-wise instantiations), strips with a ragged last one, segments, levels smaller than a strip"""
    import _oflk

    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    p, c = _pair(rng, H, W, kind)
    for (L, K) in ((3, 3), (2, 2), (1, 2), (4, 1)):
        plan = _oflk.Plan(0, 1, H, W, L, 5, K)
        plan.set_arithmetic(2)
        u, v, log, runs = _run(plan, p[None], c[None])
        mu, mv, mlog, mruns, xlog = _model(p, c, L, K, exact_means=True)
        assert list(runs[0]) == list(mruns), (shape, kind, L, K, runs, mruns)
        bad = np.argwhere(~((u[0] == mu) & (v[0] == mv)))
        assert bad.size == 0, (shape, kind, L, K, len(bad), bad[:5])
        # the device's log within E_dev, the model's NumPy-order log within NumPy's bound, of the exact means of the same d
        # (each level's pair of bounds at most 2e-5 at the threshold)
        dims = O.pyramid_dims(H, W, L)
        paths = [level_sum_path(2, L, K, 5, dims, l) for l in range(L)]
        assert_log_within_bounds(log[0], mlog, xlog, mruns, dims, paths, (shape, kind, L, K), at_threshold_at_most=2e-5)
        plan.close()


def test_tolerant_batch_u8_and_switching_back(golden_dir):
    """a batch of the 13 patterns: float32 and uint8 frames give the model's flows; back in exact mode the plan gives the
    reference's digests again (the switch leaves nothing behind)"""
    import hashlib

    import _oflk

    z = np.load(golden_dir / "patterns_320x240.npz")
    ref = json.loads((golden_dir / "reference_13patterns.json").read_text())["patterns"]
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    p8 = np.stack([z["frame_0"]] * len(names))
    c8 = np.stack([z[f"frame_1__{n}"] for n in names])
    B, H, W = p8.shape
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    plan.set_arithmetic(2)
    uf, vf, _, rf = _run(plan, p8.astype(np.float32), c8.astype(np.float32))
    ub, vb, _, rb = _run(plan, p8, c8, u8=True)
    assert np.array_equal(uf, ub) and np.array_equal(vf, vb) and np.array_equal(rf, rb)
    for i, n in enumerate(names):
        mu, mv, _, mruns = _model(p8[i], c8[i], 3, 3)
        assert np.array_equal(uf[i], mu) and np.array_equal(vf[i], mv) and list(rf[i]) == list(mruns), n
    plan.set_arithmetic(0)
    ue, ve, _, _ = _run(plan, p8.astype(np.float32), c8.astype(np.float32))
    dig = lambda a: hashlib.sha256((np.ascontiguousarray(a, np.float32) + np.float32(0.0)).tobytes()).hexdigest()  # noqa: E731
    for i, n in enumerate(names):
        assert dig(ue[i]) == ref[n]["pyramidal"]["u_sha256"] and dig(ve[i]) == ref[n]["pyramidal"]["v_sha256"], n
    plan.close()


def test_tolerant_mode_within_tolerance_of_the_reference(golden_dir):
    """mean EPE <= 1e-4 per field against the REFERENCE's own dense flows: the 13 patterns and the 1080p bench pair"""
    import _oflk
    from oflk_synth import synth_pair

    dense = np.load(golden_dir / "dense_reference_flows.npz")
    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    p = np.stack([z["frame_0"].astype(np.float32)] * len(names))
    c = np.stack([z[f"frame_1__{n}"].astype(np.float32) for n in names])
    plan = _oflk.Plan(0, len(names), 240, 320, 3, 5, 3)
    plan.set_arithmetic(2)
    u, v, _, runs = _run(plan, p, c)
    plan.close()
    report = {}
    for i, n in enumerate(names):
        ru, rv = dense[f"{n}__u"], dense[f"{n}__v"]
        report[n] = _epe(u[i], v[i], ru, rv)
        assert list(runs[i]) == list(dense[f"{n}__iters"]), n
        assert report[n] <= TOL, (n, report[n])
    pp, cc = synth_pair(1080, 1920, 0)
    plan = _oflk.Plan(0, 1, 1080, 1920, 3, 5, 3)
    plan.set_arithmetic(2)
    u, v, _, runs = _run(plan, pp[None], cc[None])
    plan.close()
    report["bench_1080p_pair0"] = _epe(u[0], v[0], dense["bench_1080p_pair0__u"].astype(np.float32),
                                       dense["bench_1080p_pair0__v"].astype(np.float32))
    assert list(runs[0]) == list(dense["bench_1080p_pair0__iters"])
    assert report["bench_1080p_pair0"] <= TOL, report


# ---------------------------------------------------------------------------------------------------------------
# single-scale 5x5: the streaming kernel is EXACT on integer-valued frames (its window sums are exact in any order
# while Sxx, Syy < 2^16) and hands every doubtful tile to the NumPy-order tile kernel within the same call
# ---------------------------------------------------------------------------------------------------------------
def _single(plan, p, c, u8=False):
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    tp, tc = torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev)
    u = torch.empty(p.shape, dtype=torch.float32, device=dev)
    v = torch.empty_like(u)
    (plan.single_scale_u8 if u8 else plan.single_scale)(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy()


def _frames(kind, rng, H, W):
    from oflk_synth import synth_pair

    if kind == "synth":           # textured 8-bit frames: every window inside the bound
        return synth_pair(H, W, int(rng.integers(0, 1000)))
    if kind == "noise":           # white 8-bit noise
        a = rng.integers(0, 256, (H, W)).astype(np.float32)
        return a, np.roll(a, (1, 2), axis=(0, 1))
    if kind == "edges":           # 0 / 255 blocks: Sxx reaches 4e5, far over 2^16 -- those tiles must come from the tile kernel
        a = (255.0 * ((np.add.outer(np.arange(H) // 7, np.arange(W) // 5) % 2))).astype(np.float32)
        a[H // 3:, :] = rng.integers(0, 256, (H - H // 3, W)).astype(np.float32)
        return a, np.roll(a, (2, 1), axis=(0, 1))
    if kind == "fractional":      # not integers at all: no window may keep the streaming kernel's sums
        a = (rng.random((H, W)) * 255.0).astype(np.float32)
        return a, (np.roll(a, (1, 1), axis=(0, 1)) * np.float32(0.97)).astype(np.float32)
    # one non-integral pixel and one out-of-range pixel in otherwise 8-bit frames: only the windows they touch are in doubt
    a, b = synth_pair(H, W, int(rng.integers(0, 1000)))
    a = a.copy(); b = b.copy()
    a[H // 2, W // 3] += np.float32(0.5)
    b[min(H - 1, 5), W - 1] = np.float32(300.0)
    a[0, 0] = np.float32(-1.0)
    return a, b


@pytest.mark.parametrize("win", [5, 7])
@pytest.mark.parametrize("shape", [(480, 640), (241, 323), (97, 130), (24, 64), (25, 121), (1080, 1920)])
@pytest.mark.parametrize("kind", ["synth", "noise", "edges", "fractional", "speckled"])
def test_single_scale_streaming_path_is_exact(oracle, shape, kind, win):
    """oflk_plan_single_scale, 5x5 and 7x7, through the streaming kernel == the oracle value for value, for every kind of
    frame: the doubtful tiles (bound exceeded, non-integral or out-of-range pixels) are redone in NumPy's order inside the
    call; the tile kernel and the automatic choice give the same"""
    import _oflk

    H, W = shape
    rng = np.random.default_rng(7 * H + W)
    p, c = _frames(kind, rng, H, W)
    ou, ov = oracle.lucas_kanade_single_scale(p, c, win)
    plan = _oflk.Plan(0, 2, H, W, 1, win, 0)
    pp, cc = np.stack([p, c]), np.stack([c, p])        # two pairs per call (the second one reversed)
    for choice in (2, 1, 0, 2):   # streaming kernel forced, tile kernel, automatic (by launch size), streaming again
        plan.set_kernels(choice)
        u, v = _single(plan, pp, cc)
        assert np.array_equal(u[0], ou) and np.array_equal(v[0], ov), (shape, kind, choice, win)
    ru, rv = oracle.lucas_kanade_single_scale(c, p, win)
    assert np.array_equal(u[1], ru) and np.array_equal(v[1], rv)
    if kind in ("synth", "noise", "edges"):
        u8, v8 = _single(plan, pp.astype(np.uint8), cc.astype(np.uint8), u8=True)
        assert np.array_equal(u8[0], ou) and np.array_equal(v8[0], ov) and np.array_equal(u8[1], ru)
    plan.close()


def test_single_scale_bound_of_the_exactness_argument(oracle):
    """the worst frames the argument admits: two-level images whose windows sit just under / just over Sxx = 2^16 (a step
    edge of height h gives Sxx = 2.5 h^2 per window row crossing it): flow equals the oracle's on both sides of the bound"""
    import _oflk

    H, W = 96, 192
    for win in (5, 7):
        for h in (130, 136, 137, 138, 150, 160, 161, 162, 163, 170, 255):   # 7x7: Sxx = 3.5 h^2 crosses 2^16 at h = 136.8
            a = np.zeros((H, W), np.float32)
            a[:, W // 2:] = h
            a[H // 2:, : W // 4] = h
            b = np.roll(a, (1, 1), axis=(0, 1))
            ou, ov = oracle.lucas_kanade_single_scale(a, b, win)
            plan = _oflk.Plan(0, 1, H, W, 1, win, 0)
            plan.set_kernels(2)
            u, v = _single(plan, a[None], b[None])
            assert np.array_equal(u[0], ou) and np.array_equal(v[0], ov), (win, h)
            plan.close()


# ---------------------------------------------------------------------------------------------------------------
# one process, several GPUs: chunks of pairs pulled from a shared counter (per-pair time is data-dependent)
# ---------------------------------------------------------------------------------------------------------------
def test_multi_chunk_queue_is_independent_of_who_takes_what(oracle):
    """a batch mixing pairs that leave every level after one iteration (identical frames), pairs that leave early and
    pairs that run every iteration, through oflk_pyramidal_batch_multi with 1 ... 5 queue workers (rehearsed on the
    devices this box has): flow, residual log and iteration counts of every pair are those of a call of its own, whoever
    took its chunk; the float32, the uint8 and the single-scale entry points"""
    import ctypes

    import _oflk
    from oflk_synth import synth_pair, synth_pair_smooth

    f32p = ctypes.POINTER(ctypes.c_float)
    i32p = ctypes.POINTER(ctypes.c_int)
    L_ = _oflk.lib()
    H, W, L, K = 240, 320, 3, 4
    pairs = []
    for i in range(11):
        if i % 3 == 0:
            p, _ = synth_pair(H, W, i)
            pairs.append((p, p.copy()))                       # exits after one iteration per level
        elif i % 3 == 1:
            pairs.append(synth_pair_smooth(H, W, i, 0.1, 0.05))     # leaves its levels after 2, 2 and 3 of 4 iterations
        else:
            pairs.append(synth_pair(H, W, i))                 # runs everything
    prev = np.ascontiguousarray(np.stack([p for p, _ in pairs]))
    curr = np.ascontiguousarray(np.stack([c for _, c in pairs]))
    B = len(pairs)
    want = [oracle.lucas_kanade_pyramidal_ex(p, c, L, 5, K) for p, c in pairs]
    assert len({tuple(w[3]) for w in want}) >= 3, "the batch should mix iteration counts"
    try:
        for workers in (0, 2, 3, 5):
            _oflk.check(L_.oflk_multi_rehearsal(workers))
            u, v = np.empty_like(prev), np.empty_like(prev)
            log, runs = np.zeros((B, L, K, 2), np.float32), np.zeros((B, L), np.int32)
            _oflk.check(L_.oflk_pyramidal_batch_multi(prev.ctypes.data_as(f32p), curr.ctypes.data_as(f32p), B, H, W, L, 5, K, 0,
                                                      u.ctypes.data_as(f32p), v.ctypes.data_as(f32p), log.ctypes.data_as(f32p),
                                                      runs.ctypes.data_as(i32p)))
            for b, (wu, wv, wlog, wruns) in enumerate(want):
                assert np.array_equal(u[b], wu) and np.array_equal(v[b], wv) and list(runs[b]) == list(wruns), (workers, b)
        _oflk.check(L_.oflk_multi_rehearsal(4))
        us, vs = np.empty_like(prev), np.empty_like(prev)
        _oflk.check(L_.oflk_single_scale_batch_multi(prev.ctypes.data_as(f32p), curr.ctypes.data_as(f32p), B, H, W, 5, 0,
                                                     us.ctypes.data_as(f32p), vs.ctypes.data_as(f32p)))
        for b, (p, c) in enumerate(pairs):
            ou, ov = oracle.lucas_kanade_single_scale(p, c, 5)
            assert np.array_equal(us[b], ou) and np.array_equal(vs[b], ov), b
        # a failing chunk stops the queue and reports its device
        rc = L_.oflk_pyramidal_batch_multi(prev.ctypes.data_as(f32p), curr.ctypes.data_as(f32p), B, H, W, L, 101, K, 0,
                                           us.ctypes.data_as(f32p), vs.ctypes.data_as(f32p), None, None)
        assert rc != 0 and b"device" in L_.oflk_last_error()
    finally:
        _oflk.check(L_.oflk_multi_rehearsal(0))
    assert L_.oflk_multi_rehearsal(-1) != 0


def test_bench_gather_runs_over_rccl_with_the_rank_this_box_has():
    """bench.py --gather: RCCL is initialised (one rank), the shard is gathered on device tensors after the timed region, the
    gathered flow's checksum equals the all-reduced total, and `value` is computed without it"""
    import os
    import subprocess
    import sys

    root = Path(__file__).resolve().parents[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29581", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, str(root / "bench.py"), "--pairs", "4", "--steps", "2", "--warmup", "1", "--gather",
                          "--no-cpu-baseline", "--no-one-pair", "--no-live-traffic", "--no-parity"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    g = line["gather"]
    assert g["backend"] == "nccl" and g["pairs"] == 4 and g["equals_allreduce_total"] is True and g["gather_ms"] > 0
    assert line["value"] > 0 and line["n_gpus"] == 1


MORE_SCALES = (0.35, 0.45, 0.55, 0.65, 0.8, 0.9, 0.25, 0.7, 1.0 / 3.0)


@pytest.mark.parametrize("sf", MORE_SCALES)
def test_pyramid_any_scale_factor_equals_the_reference(golden_dir, sf):
    """build_gaussian_pyramid of the drop-in module at nine scale factors nobody tuned for: the shim hands SciPy's own
    Gaussian weights (formed with NumPy) to oflk_build_pyramid_w, and the pyramid equals the reference's
    (tests/golden/pyramid_scales_more.npz, made by importing it) value for value"""
    import lucas_kanade_pyramidal as P

    z = np.load(golden_dir / "pyramid_scales_more.npz")
    levels = 3 if sf >= 0.3 else 2
    pyr = P.build_gaussian_pyramid(z["image"], levels, scale_factor=sf)
    assert len(pyr) == levels
    for l, a in enumerate(pyr):
        np.testing.assert_array_equal(np.asarray(a, np.float32), z[f"sf{sf!r}_level{l}"])


def test_contracted_mode_against_the_reference_dense_flows(golden_dir):
    """OFLK_ARITH_CONTRACTED (round 3) graded the way the tolerant mode is: mean EPE per field against dense flows the
    reference itself produced, not against this library's exact path (the round-3 test compares the two HIP modes)"""
    import _oflk

    dense = np.load(golden_dir / "dense_reference_flows.npz")
    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    p = np.stack([z["frame_0"].astype(np.float32)] * len(names))
    c = np.stack([z[f"frame_1__{n}"].astype(np.float32) for n in names])
    plan = _oflk.Plan(0, len(names), 240, 320, 3, 5, 3)
    plan.set_arithmetic(1)
    u, v, _, runs = _run(plan, p, c)
    plan.close()
    for i, n in enumerate(names):
        assert list(runs[i]) == list(dense[f"{n}__iters"]), n
        assert _epe(u[i], v[i], dense[f"{n}__u"], dense[f"{n}__v"]) <= TOL, n


def test_tolerant_mode_keeps_the_exit_decision_band_and_its_exact_redo(oracle):
    """The flag and its exact redo work in the tolerant mode: frames curr_t = prev + t * (shifted - prev), t bisected on the
    DEVICE's own first mean of the (single, streaming) level until it sits 2e-5 (relative) above the threshold -- inside the
    band -- are flagged, and oflk_plan_resolve_uncertain redoes the pair EXACTLY (its own exact pyramid): the redone pair
    equals the oracle, while a pair far from the threshold stays the tolerant model's.  This cannot see a decision that the
    mode's arithmetic flips OUTSIDE the band (it bisects on the device's mean, not the reference's): that the band is wide
    enough for the mode is measured on the CPU, tests/test_tolerant_model.py
    (test_tolerant_mode_moves_near_threshold_means_by_far_less_than_the_band).  L = 1, K = 2 is inside the envelope."""
    import torch

    import _oflk
    import oflk_tolerant_model as M
    from oflk_synth import synth_pair

    H, W, L, K = 96, 128, 1, 2
    prev, shifted = synth_pair(H, W, 0, dx=0.75, dy=-0.5)
    delta = (shifted - prev).astype(np.float64)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    d_prev = torch.from_numpy(prev[None]).to(dev)
    u, v = torch.empty_like(d_prev), torch.empty_like(d_prev)
    plan = _oflk.Plan(0, 1, H, W, L, 5, K)
    plan.set_arithmetic(2)

    def run(t):
        c = (prev + t * delta).astype(np.float32)
        d_curr = torch.from_numpy(c[None]).to(dev)
        plan.pyramidal(d_prev.data_ptr(), d_curr.data_ptr(), u.data_ptr(), v.data_ptr(), st)
        log, runs = plan.read_log(st)
        torch.cuda.synchronize()
        return c, d_curr, float(max(log[0, 0, 0])), list(runs[0])

    thr = float(np.float32(0.01))
    target = thr * (1.0 + 2e-5)
    lo, hi = 0.0, 1.0
    assert run(lo)[2] < target < run(hi)[2]
    got = None
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        c, d_curr, m, runs = run(mid)
        if 0.5e-5 < m / thr - 1.0 < 4e-5:
            got = (c, d_curr, m, runs)
            break
        if m < target:
            lo = mid
        else:
            hi = mid
    assert got is not None, "the bisection never landed inside the band: the construction is broken"
    c, d_curr, m, runs = got
    flags = plan.read_uncertain(st)
    assert flags.astype(bool).any(), f"a first mean {m / thr - 1.0:.2e} above the threshold was not flagged"
    n = plan.resolve_uncertain(d_prev.data_ptr(), d_curr.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    assert n == 1
    ou, ov, _, oruns = oracle.lucas_kanade_pyramidal_ex(prev, c, L, 5, K)
    _, runs2 = plan.read_log(st)
    assert list(runs2[0]) == list(oruns)
    assert np.array_equal(u.cpu().numpy()[0], ou) and np.array_equal(v.cpu().numpy()[0], ov)   # exact, not merely close
    # far from the threshold: no flag, the tolerant model's flow
    c, d_curr, m, runs = run(1.0)
    assert not plan.read_uncertain(st).astype(bool).any()
    mu, mv, _, mruns = M.pyramidal(prev, c, M.tolerant_spec(L, K, (H, W)), 5)
    assert list(runs) == list(mruns) and np.array_equal(u.cpu().numpy()[0], mu) and np.array_equal(v.cpu().numpy()[0], mv)
    plan.close()


def test_round4_passes_captured_into_a_hip_graph(oracle):
    """the new passes only enqueue kernels too: a tolerant pyramidal pass and a single-scale pass with the streaming kernel
    forced (streaming launch + redo pass over a device-side list), captured on a side stream and replayed on new frames
    written into the same buffers, give the model's / the oracle's flow on every replay"""
    import torch

    import _oflk
    import oflk_tolerant_model as M
    from oflk_synth import synth_pair

    dev = torch.device("cuda", 0)
    H, W, L, K = 240, 320, 3, 3
    prev = torch.empty((2, H, W), dtype=torch.float32, device=dev)
    curr = torch.empty_like(prev)
    u, v = torch.empty_like(prev), torch.empty_like(prev)
    us, vs = torch.empty_like(prev), torch.empty_like(prev)
    plan = _oflk.Plan(0, 2, H, W, L, 5, K)
    plan.set_arithmetic(2)
    plan_s = _oflk.Plan(0, 2, H, W, 1, 5, 0)
    plan_s.set_kernels(2)
    st = torch.cuda.current_stream().cuda_stream
    plan.pyramidal(prev.data_ptr(), curr.data_ptr(), u.data_ptr(), v.data_ptr(), st)   # warm-up outside the capture
    plan_s.single_scale(prev.data_ptr(), curr.data_ptr(), us.data_ptr(), vs.data_ptr(), st)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s_ = torch.cuda.current_stream().cuda_stream
        plan.pyramidal(prev.data_ptr(), curr.data_ptr(), u.data_ptr(), v.data_ptr(), s_)
        plan_s.single_scale(prev.data_ptr(), curr.data_ptr(), us.data_ptr(), vs.data_ptr(), s_)
    for rep in range(3):
        pairs = [synth_pair(H, W, pair_index=50 + 2 * rep + b) for b in range(2)]
        if rep == 1:   # a frame with 0 / 255 blocks: the redo list is not empty on this replay
            a = pairs[0][0].copy()
            a[40:80, 60:140] = 255.0 * ((np.add.outer(np.arange(40), np.arange(80)) // 3) % 2)
            pairs[0] = (a.astype(np.float32), pairs[0][1])
        prev.copy_(torch.from_numpy(np.stack([p for p, _ in pairs])))
        curr.copy_(torch.from_numpy(np.stack([c for _, c in pairs])))
        for t in (u, v, us, vs):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for b, (p, c) in enumerate(pairs):
            mu, mv, _, _ = M.pyramidal(p, c, M.tolerant_spec(L, K, (H, W)), 5)
            assert np.array_equal(u[b].cpu().numpy(), mu) and np.array_equal(v[b].cpu().numpy(), mv), f"replay {rep} pair {b} (tolerant)"
            ou, ov = oracle.lucas_kanade_single_scale(p, c, 5)
            assert np.array_equal(us[b].cpu().numpy(), ou) and np.array_equal(vs[b].cpu().numpy(), ov), f"replay {rep} pair {b} (single)"
    plan.close()
    plan_s.close()


def test_host_entry_points_in_the_tolerant_mode(golden_dir):
    """oflk_set_host_arithmetic(OFLK_ARITH_TOLERANT) (what OFLK_ARITH=tolerant makes the shims call): the drop-in function
    then returns the tolerant model's flow -- within 1e-4 px of the reference's dense flow; switching back restores the
    reference's digests"""
    import hashlib

    import _oflk
    import lucas_kanade_pyramidal as P
    import oflk_tolerant_model as M

    L_ = _oflk.lib()
    dense = np.load(golden_dir / "dense_reference_flows.npz")
    z = np.load(golden_dir / "patterns_320x240.npz")
    ref = json.loads((golden_dir / "reference_13patterns.json").read_text())["patterns"]
    f0 = z["frame_0"].astype(np.float32)
    try:
        _oflk.check(L_.oflk_set_host_arithmetic(2))
        for n in ("translate_medium", "rotate_small", "translate_extreme", "no_motion"):
            f1 = z[f"frame_1__{n}"].astype(np.float32)
            u, v = P.lucas_kanade_pyramidal(f0, f1, 3, 5, 3)
            mu, mv, _, _ = M.pyramidal(f0, f1, M.tolerant_spec(3, 3, f0.shape), 5)
            assert np.array_equal(u, mu) and np.array_equal(v, mv), n
            assert _epe(u, v, dense[f"{n}__u"], dense[f"{n}__v"]) <= TOL, n
    finally:
        _oflk.check(L_.oflk_set_host_arithmetic(0))
    f1 = z["frame_1__translate_medium"].astype(np.float32)
    u, v = P.lucas_kanade_pyramidal(f0, f1, 3, 5, 3)
    dig = lambda a: hashlib.sha256((np.ascontiguousarray(a, np.float32) + np.float32(0.0)).tobytes()).hexdigest()  # noqa: E731
    assert dig(u) == ref["translate_medium"]["pyramidal"]["u_sha256"] and dig(v) == ref["translate_medium"]["pyramidal"]["v_sha256"]
    assert L_.oflk_set_host_arithmetic(7) != 0
