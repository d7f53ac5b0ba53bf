"""What the scenes of tests/step_loop_scenes.py promise, on the statements alone (no GPU).

tests/test_gpu_step_loops.py holds the kernels' step loops to these scenes past the grid limit.  A batch in which every step
took the same path through a loop body would show nothing, so the conditions below are asserted here, not measured: the seeds
in step_loop_scenes.py are chosen so that they hold.
"""
import numpy as np
import pytest

import align_model as AM
import motion_model as MM
import step_loop_scenes as SC

KINDS = [("affine", AM.AFFINE), ("homography", AM.HOMOGRAPHY)]
FORMS = [("pair", 2, 2, np.float32), ("sequence", 1, 1, np.uint8), ("sequence", 2, 2, np.float32)]


def test_the_second_pass_takes_every_transition_twice():
    assert SC.GRID == 65535 and SC.P == 7 and SC.GRID % SC.P == 1 and SC.S - SC.GRID == 2 * SC.P
    second = np.arange(SC.GRID, SC.S)
    first = second - SC.GRID
    pairs = sorted(zip((first % SC.P).tolist(), (second % SC.P).tolist()))
    assert pairs == sorted([(k, (k + 1) % SC.P) for k in range(SC.P)] * 2)
    steps = SC.sample_steps()
    assert len(steps) < 320 and steps[0] == 0 and steps[-1] == SC.S - 1
    for side in (steps[steps < SC.GRID], steps[steps >= SC.GRID]):
        assert set((side % SC.P).tolist()) == set(range(SC.P)), "the sample holds every kind on both sides of the grid limit"
    assert set(range(SC.GRID, SC.S)) <= set(steps.tolist()) and set(range(2 * SC.P)) <= set(steps.tolist())


@pytest.mark.parametrize("family", SC.FAMILIES, ids=["translation", "similarity", "affine", "homography"])
def test_the_fit_kinds_succeed_and_fail_in_both_ways(family):
    m = SC.sample_size(family)
    model, inlier, counts = SC.fit_model(family, np.arange(SC.P))
    assert counts[:, 2].tolist() == [1, 0, 1, 0, 1, 0, 1]
    assert counts[1, 1] == 0 and counts[3, 1] == m - 1 and counts[5, 1] == 9 >= m, "M = 0, M = m - 1 and a failure with M >= m"
    assert counts[0, 1] == SC.N and counts[6, 1] == SC.N - 2 and counts[2, 1] == SC.N - 5
    assert len({int(c) for c in counts[:, 1]}) >= 5 and counts[4, 1] == SC.N
    for k in (1, 3, 5):
        assert np.isnan(model[k]).all() and not inlier[k].any() and counts[k, 0] == 0
    for k in (0, 2, 4, 6):
        assert np.isfinite(model[k]).all() and counts[k, 0] == inlier[k].sum() >= m
    # the offset is the same on both sides, finite coordinates move with the step and the kinds' masks do not
    src, dst, valid = SC.fit_steps(family, np.array([0, 7, 251 * 7, SC.GRID + 6]))
    assert np.array_equal(valid[0], valid[1]) and np.array_equal(valid[0], valid[2])
    assert np.array_equal(src[1] - src[0], np.full((SC.N, 2), 1.75, np.float32)) and np.array_equal(dst[1] - dst[0], src[1] - src[0])
    assert np.array_equal(src[2], src[0]) and src.dtype == dst.dtype == np.float32 and valid.dtype == np.uint8
    # a step's result depends on its index: the same scene at another step of its kind gives other bytes
    a, b = SC.fit_model(family, [0]), SC.fit_model(family, [SC.P])
    assert a[0].tobytes() != b[0].tobytes()


@pytest.mark.parametrize("photometric", [False, True], ids=["plain", "photometric"])
@pytest.mark.parametrize("kind,code", KINDS)
def test_the_alignment_kinds_end_in_every_status(oracle, kind, code, photometric):
    for form, levels, iterations, dtype in FORMS:
        want = SC.align_model(code, photometric, form, levels, iterations, dtype)
        model, status, stats = want[:3]
        what = f"{kind} {form} L={levels} n={iterations}: statuses {status.tolist()}, accepted {stats[:, 3].tolist()}"
        assert set(status.tolist()) == {0, 1, 2}, what
        assert status[0] == 1 and status[2] == 1 and status[5] == 2, what
        assert status[1] == 0 and not stats[1].any(), what                               # held
        assert status[3] == 0 and np.isnan(stats[3, 0]) and stats[3, 2] == 0, what       # thrown off the frame
        assert status[6] == 0 and stats[6, 3] == 0 and np.isfinite(stats[6, 0]), what    # frozen at the first iteration
        assert (stats[:, 3] < levels * iterations).any() and (stats[:, 3] == levels * iterations).any(), what
        assert stats[0, 3] == levels * iterations, what
        if form == "sequence":
            assert 0 < stats[6, 2] < 0.25, what
        if photometric:
            for k in range(SC.P):
                assert status[k] == 1 or want[3][k].tolist() == [1.0, 0.0]
            assert want[3][0].tolist() != [1.0, 0.0] and want[3][2].tolist() != [1.0, 0.0]
        # the input of a step that is not refined comes back: the bytes differ between the kinds
        src = SC.align_pairs(code, photometric)[2] if form == "pair" else SC.align_frames(code, photometric, dtype)[1]
        for k in (1, 3, 5, 6):
            assert model[k].tobytes() == src[k].tobytes()


def test_the_sequence_frames_are_the_pair_forms_where_they_can_be():
    for photometric in (False, True):
        a, b, model, status = SC.align_pairs(AM.HOMOGRAPHY, photometric)
        frames, smodel, sstatus = SC.align_frames(AM.HOMOGRAPHY, photometric, np.float32)
        assert frames.shape == (SC.P + 1, SC.H, SC.W) and np.array_equal(frames[SC.P], frames[0])
        for k in (0, 2, 5):
            assert np.array_equal(frames[k], a[k]) and np.array_equal(frames[k + 1], b[k]) and np.array_equal(smodel[k], model[k])
        assert np.array_equal(frames[4], frames[5]) and np.array_equal(status, sstatus)
        u8 = SC.align_frames(AM.HOMOGRAPHY, photometric, np.uint8)[0]
        assert u8.dtype == np.uint8 and 0 <= frames.min() and frames.max() < 254.5, "nothing clips"
    t = SC.tiled(np.arange(SC.P))
    assert len(t) == SC.S and t[SC.GRID] == 1 and t[-1] == (SC.S - 1) % SC.P


@pytest.mark.parametrize("photometric", [False, True], ids=["plain", "photometric"])
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W,levels", SC.FLOOR)
def test_a_step_at_the_floor_of_the_sizes_is_refined(oracle, H, W, levels, kind, code, photometric):
    import align_photo_model as APM

    mod = APM if photometric else AM
    h, w = H, W
    for _ in range(levels - 1):
        h, w = h // 2, w // 2
    assert h == 8 and w >= 8, "the coarsest level stands on the floor"
    for dtype in (np.float32, np.uint8):
        a, b, model = SC.floor_steps(H, W, code, photometric, dtype)
        want = mod.refine(a, b, model, None, code, levels, SC.FLOOR_ITERATIONS)
        assert (want[1] == 1).any(), f"{W}x{H} {kind} {np.dtype(dtype).name}: statuses {want[1].tolist()}"
