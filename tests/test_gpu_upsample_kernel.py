"""k_upsample's thread mapping, where tests/test_gpu_stages.py does not reach: the interleaved {u, v} form inside a
pyramidal plan call, whose source slot is chosen per pair from that pair's iteration count, and two planar targets whose
right edge the lists of tests/stage_scenes.py lack.

A block of k_upsample makes 256 x 16 outputs; a wave covers one 128-column half of the tile over 8 rows and a lane 2
columns of it.  Each finest shape below is there for one hazard of that mapping:

    35 x 262   width no multiple of 4: 8-byte stores; the last block column holds 6 columns, the rows end 3 into a tile
    40 x 516   16-byte stores; the last block column holds 4 columns
    24 x 384   the last block column is exactly the left 128-column half: the waves of the right half leave
    20 x 600   three block columns: first, middle, last
    70 x 300   five block rows; the last holds 6 of a wave's 8 rows

Every pyramidal case is one call of a 3-pair plan against oracle/oflk_oracle.py pair by pair: u, v and iters_run equal
bit for bit (stage_scenes.same_bits).  Pair 0 and pair 2 are synth_pair frames, which run every iteration.  Pair 1 is a
synth_pair_smooth pair.  With its default shift (0.3, 0.1) that pair leaves no level early at any of these sizes, so each
case carries the shift with which it does (found with the oracle on the CPU): it then leaves a level above the finest after
a number of iterations of the other parity than the full count, so the slot that the upsampling reads differs between the
pairs of one call.  The test asserts that on the oracle's iters_run before it looks at the device, and that every logged
mean stays 2 % or more away from the exit threshold, far outside the band in which the device flags a decision as
uncertain: no pair is redone outside the plan call.

Run on an MI355X:  python -m pytest tests/test_gpu_upsample_kernel.py -m gpu -q
"""
import numpy as np
import pytest

import stage_scenes as S

pytestmark = pytest.mark.gpu

WINDOW = 5
# (finest shape, levels, iterations, shift of the smooth pair, the oracle's iters_run of that pair, finest level first)
PLAN_CASES = [
    ((35, 262), 3, 3, (0.05, 0.02), [1, 1, 2]),
    ((40, 516), 3, 3, (0.1, 0.05), [2, 2, 3]),
    ((24, 384), 3, 3, (0.07, 0.03), [1, 2, 3]),
    ((20, 600), 3, 3, (0.07, 0.03), [1, 2, 3]),
    ((70, 300), 3, 3, (0.07, 0.03), [2, 1, 2]),
    ((40, 516), 2, 2, (0.03, 0.015), [2, 1]),
]
# planar form (oflk_upsample_flow): (coarse shape, target shape)
PLANAR_CASES = [((12, 192), (24, 384)), ((10, 300), (20, 600))]


def _cid(c):
    (h, w), levels, iters = c[0], c[1], c[2]
    return f"{h}x{w}-L{levels}-K{iters}"


@pytest.fixture(scope="module")
def references(oracle):
    """per case: the three pairs and the oracle's (u, v, log, iters_run) of each, computed once"""
    from oflk_synth import synth_pair, synth_pair_smooth

    out = {}
    for case in PLAN_CASES:
        (H, W), levels, iters, (dx, dy), _ = case
        pairs = [synth_pair(H, W, 0), synth_pair_smooth(H, W, 1, dx, dy), synth_pair(H, W, 5)]
        out[_cid(case)] = (pairs, [oracle.lucas_kanade_pyramidal_ex(p, c, levels, WINDOW, iters) for p, c in pairs])
    return out


@pytest.mark.parametrize("case", PLAN_CASES, ids=_cid)
def test_plan_call_with_mixed_exits_equals_the_oracle(references, case):
    import torch

    import _oflk

    (H, W), levels, iters, _, smooth_runs = case
    pairs, want = references[_cid(case)]
    runs = [[int(r) for r in w[3]] for w in want]
    assert runs[0] == [iters] * levels and runs[2] == [iters] * levels, runs
    assert runs[1] == smooth_runs, runs
    assert any((r & 1) != (iters & 1) for r in runs[1][1:]), f"the smooth pair should leave a coarse level in the other slot: {runs[1]}"
    for w in want:
        means = np.asarray(w[2]).reshape(-1)
        means = means[means > 0]
        assert np.min(np.abs(means / np.float32(0.01) - 1.0)) > 0.02, "a logged mean sits near the exit threshold"

    dev = torch.device("cuda", 0)
    prev = torch.from_numpy(np.ascontiguousarray(np.stack([p for p, _ in pairs]))).to(dev)
    curr = torch.from_numpy(np.ascontiguousarray(np.stack([c for _, c in pairs]))).to(dev)
    u, v = torch.full_like(prev, float("nan")), torch.full_like(prev, float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, len(pairs), H, W, levels, WINDOW, iters)
    try:
        plan.pyramidal(prev.data_ptr(), curr.data_ptr(), u.data_ptr(), v.data_ptr(), stream)
        _, got_runs = plan.read_log(stream)
        assert not plan.read_uncertain(stream).any(), "no exit decision of these pairs is near the threshold"
    finally:
        torch.cuda.synchronize()
        plan.close()
    gu, gv = u.cpu().numpy(), v.cpu().numpy()
    for b, (wu, wv, _, _) in enumerate(want):
        what = f"pyramidal {H}x{W}, {levels} levels, {iters} iterations, pair {b} of 3 (iters_run {runs[b]})"
        assert [int(r) for r in got_runs[b]] == runs[b], what
        S.same_bits(gu[b], wu, what + ", u")
        S.same_bits(gv[b], wv, what + ", v")


@pytest.mark.parametrize("cshape,tshape", PLANAR_CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planar_upsample_at_the_half_tile_and_three_column_edges(oracle, cshape, tshape):
    import _oflk
    import lucas_kanade_pyramidal as P

    assert S.upsample_kernel(_oflk.lib(), cshape, tshape) == "k_upsample"
    u, v = S.flow_fields(cshape, 500 + tshape[1])
    ou, ov = oracle.upsample_flow(u, v, tshape)
    gu, gv = P.upsample_flow(u, v, tshape)
    S.same_bits(gu, ou, f"upsample_flow {cshape} -> {tshape}, u")
    S.same_bits(gv, ov, f"upsample_flow {cshape} -> {tshape}, v")
