"""GPU tests of the step loops of the fits and of direct alignment past the grid limit (run on an MI355X:
python -m pytest tests/test_gpu_step_loops.py -m gpu -q).

Every batched kernel puts its steps on a grid axis of at most 65 535 blocks and reaches later steps by
`for (s = blockIdx; s < S; s += gridDim)`.  The batches here have S = 65 549 steps of seven kinds (tests/step_loop_scenes.py,
whose promises tests/test_step_loops_cpu.py asserts), so that 14 blocks of k_motion_compact, k_motion_score, k_motion_refit
(the six-coefficient models' and the homography's), k_align_reduce, k_align_update and the photometric pair take their loop a second time, from every
kind of step into the next one.  The pair form with two levels also hands 2 S = 131 098 images, the sequence form S + 1 =
65 550, to the pyramid launch's grid.z.  Everything is compared byte for byte, a NaN equal to a NaN; no tolerance anywhere.
"""
import numpy as np
import pytest

import align_model as AM
import align_photo_model as APM
import homography_model as HM
import motion_model as MM
import step_loop_scenes as SC
from test_gpu_align import _device as _plain
from test_gpu_align_photo import _device as _photo

pytestmark = pytest.mark.gpu

KINDS = [("affine", AM.AFFINE), ("homography", AM.HOMOGRAPHY)]


# ---------------------------------------------------------------------------------------------------------------------
# the fits
# ---------------------------------------------------------------------------------------------------------------------
class _Fit:
    """the device form of a fit on the batch of SC.S steps: calls on any run of its steps, into outputs and a workspace preset
    with bytes that the call must overwrite"""

    def __init__(self, family):
        import torch

        import _oflk

        self.family = family
        self.nc = 9 if family == SC.HOMOGRAPHY else 6
        d = "cuda:0"
        src, dst, valid = SC.fit_batch(family)
        self.src, self.dst, self.valid = torch.from_numpy(src).to(d), torch.from_numpy(dst).to(d), torch.from_numpy(valid).to(d)
        size = _oflk.homography_workspace if family == SC.HOMOGRAPHY else _oflk.motion_workspace
        self.ws_bytes = size(SC.S, SC.N, SC.HYPS)
        assert size(SC.GRID, SC.N, SC.HYPS) <= self.ws_bytes
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=d)

    def outputs(self):
        import torch

        d = "cuda:0"
        return (torch.full((SC.S, self.nc), -7.0, device=d), torch.full((SC.S, SC.N), 9, dtype=torch.uint8, device=d),
                torch.full((SC.S, 3), -3, dtype=torch.int32, device=d))

    def call(self, out, first, n):
        """steps first .. first + n - 1 in one call, hashed with their own indices, into their rows of `out`"""
        import _oflk

        model, inlier, counts = out
        self.ws.fill_(0xA5)
        args = (self.src.data_ptr() + first * SC.N * 8, self.dst.data_ptr() + first * SC.N * 8, self.valid.data_ptr() + first * SC.N,
                n, SC.N, self.ws.data_ptr(), self.ws_bytes, model.data_ptr() + first * self.nc * 4, inlier.data_ptr() + first * SC.N,
                counts.data_ptr() + first * 12)
        if self.family == SC.HOMOGRAPHY:
            _oflk.estimate_homography(*args, SC.HYPS, SC.THRESHOLD, SC.SEED, SC.STEP0 + first)
        else:
            _oflk.estimate_motion(*args, self.family, SC.HYPS, SC.THRESHOLD, SC.SEED, SC.STEP0 + first)

    @staticmethod
    def read(out):
        import torch

        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in out)


def _fit_past_the_grid_limit(family, name):
    fit = _Fit(family)
    looped, parts = fit.outputs(), fit.outputs()
    fit.call(looped, 0, SC.S)
    fit.call(parts, 0, SC.GRID)
    fit.call(parts, SC.GRID, SC.S - SC.GRID)
    got, unlooped = fit.read(looped), fit.read(parts)
    MM.same(got, unlooped, f"{name}: one call of {SC.S} steps against calls of {SC.GRID} and {SC.S - SC.GRID}")
    steps = SC.sample_steps()
    MM.same(tuple(x[steps] for x in got), SC.fit_model(family, steps), f"{name}: steps {steps[:3].tolist()} .. {steps[-3:].tolist()}")
    assert sorted(set(got[2][:, 2].tolist())) == [0, 1]


@pytest.mark.parametrize("family", [MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE], ids=["translation", "similarity", "affine"])
def test_the_motion_fit_past_the_grid_limit(family):
    """k_motion_compact, k_motion_score and k_motion_refit take their step loops twice: every step equals the same step in
    calls that never loop, and a sample on both sides of the limit equals the statement"""
    _fit_past_the_grid_limit(family, f"family {family}")


def test_the_homography_fit_past_the_grid_limit():
    """k_motion_compact and the homography's k_motion_score and k_motion_refit, as above"""
    assert HM.SAMPLE == SC.sample_size(SC.HOMOGRAPHY)
    _fit_past_the_grid_limit(SC.HOMOGRAPHY, "homography")


# ---------------------------------------------------------------------------------------------------------------------
# direct alignment
# ---------------------------------------------------------------------------------------------------------------------
FORMS = [("pair", 2, 2, np.float32), ("sequence", 1, 1, np.uint8), ("sequence", 2, 2, np.float32)]


@pytest.mark.parametrize("form,levels,iterations,dtype", FORMS, ids=["pair f32 L2", "sequence u8 L1", "sequence f32 L2"])
@pytest.mark.parametrize("photometric", [False, True], ids=["plain", "photometric"])
@pytest.mark.parametrize("kind,code", KINDS)
def test_alignment_past_the_grid_limit(oracle, kind, code, photometric, form, levels, iterations, dtype):
    """The steps do not depend on their index, so the whole batch is the statement on the seven kinds, tiled.  With two levels
    the pyramid launch has 2 S (pair form) or S + 1 (sequence form) images on grid.z, above 65 535"""
    device, same = (_photo, APM.same) if photometric else (_plain, AM.same)
    want = tuple(SC.tiled(x) for x in SC.align_model(code, photometric, form, levels, iterations, dtype))
    what = f"{kind} {form} form, {np.dtype(dtype).name}, L={levels} n={iterations}"
    if form == "pair":
        a, b, model, status = (SC.tiled(x) for x in SC.align_pairs(code, photometric))
        seq = False
    else:
        frames, model, status = SC.align_frames(code, photometric, dtype)
        a, b, model, status, seq = SC.tiled(frames[:SC.P], SC.S + 1), None, SC.tiled(model), SC.tiled(status), True
    got = device(a, b, model, status, code, levels, iterations, sequence=seq)
    same(got, want, f"{what}: {SC.S} steps against the statement")
    n = 2 * SC.P
    few = device(a[:n + seq], None if seq else b[:n], model[:n], status[:n], code, levels, iterations, sequence=seq)
    same(tuple(x[:n] for x in got), few, f"{what}: the first {n} of {SC.S} steps against a call of {n}")


@pytest.mark.parametrize("photometric", [False, True], ids=["plain", "photometric"])
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W,levels", SC.FLOOR)
def test_the_floor_of_the_alignments_sizes(oracle, H, W, levels, kind, code, photometric):
    """8 x 8 per level is the least the calls accept: the smallest frame, a coarsest level of exactly 8 x 8, and one tile row
    with a second tile column of one pixel; device and host form equal the statement"""
    import _oflk

    device, mod = (_photo, APM) if photometric else (_plain, AM)
    for dtype in (np.float32, np.uint8):
        a, b, model = SC.floor_steps(H, W, code, photometric, dtype)
        want = mod.refine(a, b, model, None, code, levels, SC.FLOOR_ITERATIONS)
        what = f"{W}x{H} {kind} {np.dtype(dtype).name} L={levels}"
        mod.same(device(a, b, model, None, code, levels, SC.FLOOR_ITERATIONS), want, what + " device")
        host = _oflk.align_host(a, b, model, None, levels, SC.FLOOR_ITERATIONS, code, 0.25, *([True] if photometric else []))
        mod.same(host, want, what + " host")
