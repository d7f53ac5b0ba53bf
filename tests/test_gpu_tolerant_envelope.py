"""GPU tests of the envelope of the opt-in OFLK_ARITH_TOLERANT arithmetic (include/oflk.h; run on an MI355X:
python -m pytest tests/test_gpu_tolerant_envelope.py -m gpu -q).

  * a tolerant plan equals the CPU model (oracle/oflk_tolerant_model.c with tolerant_spec) bit for bit in every
    (levels, iterations) cell of L 1..4 x K 1..5, inside the envelope and outside it, on even, odd and tiny shapes
  * outside the envelope a tolerant plan and the tolerant host entry points return the reference's values
  * inside it, at the bench configuration (3, 3), sizes the round-4 tests did not grade: a 3840x2160 pair (float32 and
    uint8 frames) and a second 1080p pair, within a third of the 1e-4 px bar of the oracle's flow
The CPU side of the same envelope (every cell against the oracle on the 13 patterns) is tests/test_tolerant_model.py.
"""
import hashlib
import json

import numpy as np
import pytest
from test_tolerant_model import assert_log_within_bounds, level_sum_path

pytestmark = pytest.mark.gpu

TOL = 1e-4   # mean endpoint error against the reference's flow, px (north_star)
CELLS = [(L, K) for L in range(1, 5) for K in range(1, 6)]


def _epe(u, v, ru, rv):
    return float(np.mean(np.sqrt((u.astype(np.float64) - ru) ** 2 + (v.astype(np.float64) - rv) ** 2)))


def _digest(a):
    return hashlib.sha256((np.ascontiguousarray(a, np.float32) + np.float32(0.0)).tobytes()).hexdigest()


def _run(plan, p, c, u8=False):
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    tp, tc = torch.from_numpy(np.ascontiguousarray(p)).to(dev), torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    u = torch.empty(p.shape, dtype=torch.float32, device=dev)
    v = torch.empty_like(u)
    (plan.pyramidal_u8 if u8 else plan.pyramidal)(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    log, runs = plan.read_log(st)
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy(), log, runs


def _tolerant_plan(B, H, W, L, K):
    import _oflk

    plan = _oflk.Plan(0, B, H, W, L, 5, K)
    plan.set_arithmetic(2)
    return plan


@pytest.fixture(scope="module")
def patterns(golden_dir):
    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    f0 = z["frame_0"].astype(np.float32)
    return names, f0, {n: z[f"frame_1__{n}"].astype(np.float32) for n in names}


@pytest.mark.parametrize("shape", [(240, 320), (241, 323), (23, 21)])
def test_tolerant_plan_equals_its_cpu_model_in_every_cell(shape):
    """flows, iteration counts and residual logs of a tolerant plan == the CPU model's in all 20 cells (the model is the
    streaming arithmetic inside the envelope and the exact one outside it)"""
    import oflk_tolerant_model as M
    from oflk_synth import synth_pair

    H, W = shape
    p, c = synth_pair(H, W, pair_index=3)
    for L, K in CELLS:
        plan = _tolerant_plan(1, H, W, L, K)
        try:
            u, v, log, runs = _run(plan, p[None], c[None])
        finally:
            plan.close()
        mu, mv, mlog, mruns, xlog = M.pyramidal(p, c, M.tolerant_spec(L, K, shape), 5, exact_means=True)
        assert list(runs[0]) == list(mruns), (shape, L, K, runs, mruns)
        bad = np.argwhere(~((u[0] == mu) & (v[0] == mv)))
        assert bad.size == 0, (shape, L, K, len(bad), bad[:5])
        # the device's log within E_dev, the model's NumPy-order log within NumPy's bound, of the exact means of the same d
        dims = M.O.pyramid_dims(H, W, L)
        paths = [level_sum_path(2, L, K, 5, dims, l) for l in range(L)]
        assert_log_within_bounds(log[0], mlog, xlog, mruns, dims, paths, (shape, L, K), at_threshold_at_most=2e-5)


@pytest.mark.parametrize("cell", [(4, 3), (4, 2), (2, 3), (2, 1), (1, 5)], ids=["L4K3-deep", "L4K2", "L2K3-shallow", "L2K1", "L1K5"])
def test_tolerant_plan_outside_the_envelope_is_the_oracle(oracle, patterns, cell):
    """the 13-pattern batch through a tolerant plan at cells outside the envelope: the oracle's flows and iteration counts
    bit for bit, float32 and uint8 frames (the contracted pyramid is off there too)"""
    import oflk_tolerant_model as M

    L, K = cell
    assert not M.tolerant_relaxes(L, K)
    names, f0, f1 = patterns
    p = np.stack([f0] * len(names))
    c = np.stack([f1[n] for n in names])
    plan = _tolerant_plan(len(names), 240, 320, L, K)
    try:
        u, v, _, runs = _run(plan, p, c)
        ub, vb, _, rb = _run(plan, p.astype(np.uint8), c.astype(np.uint8), u8=True)
    finally:
        plan.close()
    assert np.array_equal(u, ub) and np.array_equal(v, vb) and np.array_equal(runs, rb)
    for i, n in enumerate(names):
        ou, ov, _, oruns = oracle.lucas_kanade_pyramidal_ex(f0, f1[n], L, 5, K)
        assert list(runs[i]) == list(oruns), (cell, n)
        assert np.array_equal(u[i], ou) and np.array_equal(v[i], ov), (cell, n)


@pytest.mark.parametrize("preset", ["shallow", "deep"])
def test_tolerant_host_entry_points_on_the_presets(golden_dir, patterns, preset):
    """oflk_set_host_arithmetic(OFLK_ARITH_TOLERANT) -- what OFLK_ARITH=tolerant makes the shims call -- on the reference's own
    2-level and 4-level presets (both outside the envelope): the drop-in function returns the reference's digests"""
    import _oflk
    import lucas_kanade_pyramidal as P

    _, f0, f1 = patterns
    ref = json.loads((golden_dir / "reference_presets.json").read_text())
    lib = _oflk.lib()
    try:
        _oflk.check(lib.oflk_set_host_arithmetic(2))
        for n in ("translate_medium", "rotate_small", "translate_extreme", "no_motion"):
            r = ref[n][preset]
            u, v = P.lucas_kanade_pyramidal(f0, f1[n], r["levels"], r["window_size"], r["iterations"])
            assert _digest(u) == r["u_sha256"] and _digest(v) == r["v_sha256"], (preset, n)
    finally:
        _oflk.check(lib.oflk_set_host_arithmetic(0))


@pytest.mark.parametrize("case", ["4k_pair0", "1080p_pair1"])
def test_tolerant_mode_at_the_bench_cell_on_new_sizes(oracle, case):
    """(3, 3), the bench configuration, inside the envelope: one 3840x2160 pair of the 4k64 workload and a second 1080p pair
    (pair_index = 1) reach mean EPE <= TOL / 3 against the oracle (the reference's flow) with its iteration counts, equal
    the CPU model bit for bit, and uint8 frames give the float32 frames' flow"""
    import oflk_tolerant_model as M
    from oflk_synth import synth_pair

    (H, W), pi = {"4k_pair0": ((2160, 3840), 0), "1080p_pair1": ((1080, 1920), 1)}[case]
    p, c = synth_pair(H, W, pair_index=pi)
    assert np.array_equal(p, p.astype(np.uint8)) and np.array_equal(c, c.astype(np.uint8))   # 8-bit frames
    plan = _tolerant_plan(1, H, W, 3, 3)
    try:
        u, v, _, runs = _run(plan, p[None], c[None])
        ub, vb, _, rb = _run(plan, p.astype(np.uint8)[None], c.astype(np.uint8)[None], u8=True)
    finally:
        plan.close()
    assert np.array_equal(u, ub) and np.array_equal(v, vb) and np.array_equal(runs, rb)
    ou, ov, _, oruns = oracle.lucas_kanade_pyramidal_ex(p, c, 3, 5, 3)
    assert list(runs[0]) == list(oruns)
    e = _epe(u[0], v[0], ou, ov)
    assert e <= TOL / 3, (case, e)
    mu, mv, _, _ = M.pyramidal(p, c, M.tolerant_spec(3, 3, (H, W)), 5)
    assert np.array_equal(u[0], mu) and np.array_equal(v[0], mv)
