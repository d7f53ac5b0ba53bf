"""Scenes for robust direct alignment (tests/test_align_robust_cpu.py, tests/test_gpu_align_robust.py).

Test infrastructure: the product never imports this file.
"""
import math

import numpy as np

import align_model as AM
import align_photo_model as APM

DELTA = 4.0                    # grey levels: the suggested value, the sparse tracker's max_residual default
NO_DELTA = 3.0e38              # above every residual: the weights are all 1.0
SIZES = [(96, 130), (70, 257)]
SEEDS = [1, 2, 3]
EXPOSURES = [(0.7, 20.0), (1.3, -15.0), (1.0, 0.0)]
MOVE = (3, 7)                  # the object's own motion from A to B: rows, columns


def object_box(H, W):
    """the object's rectangle in A: (top, left, height, width), 12 % of the frame"""
    return H // 5, W // 6, int(H * math.sqrt(0.12)), int(W * math.sqrt(0.12))


def moving_object_pair(H, W, seed, kind, exposure=None):
    """AM.planted_pair(H, W, seed, kind) with a textured rectangle pasted into A at (H // 5, W // 6) and into B 3 rows lower and
    7 columns further right; exposure (gain, bias): B re-exposed after the object is pasted.
    -> (A, B (H, W) float32, planted (9,) float64)"""
    A, B, planted = AM.planted_pair(H, W, seed, kind)
    y, x, oh, ow = object_box(H, W)
    obj = AM.texture(oh, ow, 77 + seed, sigma=1.5, margin=0).astype(np.float32)
    A, B = A.copy(), B.copy()
    A[y:y + oh, x:x + ow] = obj
    B[y + MOVE[0]:y + MOVE[0] + oh, x + MOVE[1]:x + MOVE[1] + ow] = obj
    if exposure is not None:
        B = APM.exposed(B, *exposure)
    return A, B, planted


def rejected_pair(H, W, photometric):
    """a step that the refinement makes worse (align_model.checker_pair; the photometric form takes that pair's one grey level
    for a bias, so its B is A + x / 20, as in step_loop_scenes.rejected_pair)"""
    ca, cb = AM.checker_pair(H, W)
    if photometric:
        x = np.arange(W, dtype=np.float32)[None, :]
        cb = (ca + np.float32(0.05) * x).astype(np.float32)
    return ca, cb


def mixed_steps(H, W, kind, seed, dtype, photometric):
    """S = 8 steps of every sort, built as test_gpu_align_photo._mixed_steps builds its five; photometric: b re-exposed (gain
    0.8, bias +12).  uint8: the source is compressed to 40 + 0.5 v first (the checker pair to 10 + 0.5 v), so that nothing clips
    0  equal frames under the identity                 1  a held step (status 0) of a planted pair
    2  a model that throws b off the frame (count 0)   3  a planted pair seen through a shift of a third of the frame
    4  a flat template                                 5  a model with a NaN
    6  a step made worse: rejected                     7  a planted pair with an object that moves on its own
    -> (a, b (8, H, W) of dtype, model (8, nc) float32, status (8,) int32)"""
    A, B, planted = AM.planted_pair(H, W, seed, kind, move=2.0)
    ident = AM.IDENTITY[kind]
    off = ident.copy()
    off[2], off[5] = 3.0 * W, -2.0 * H
    canvas = AM.texture(H, W + W // 3, seed + 1)
    wide = AM.view(canvas, H, W + W // 3, AM.IDENTITY[AM.HOMOGRAPHY])
    shifted = ident.copy()
    shifted[2] = 0.4 - float(W // 3)
    nan = AM.pushed(planted, H, W, kind, 0.5)
    nan[4] = np.nan
    ca, cb = rejected_pair(H, W, photometric)
    OA, OB, oplanted = moving_object_pair(H, W, seed % 3 + 1, kind)
    a = np.stack([A, A, A, wide[:, :W], np.full((H, W), 9.0, np.float32), A, ca, OA])
    b = np.stack([A, B, B, wide[:, W // 3:], B, B, cb, OB])
    if dtype == np.uint8:
        a, b = np.float32(40.0) + np.float32(0.5) * a, np.float32(40.0) + np.float32(0.5) * b
        a[6], b[6] = a[6] - np.float32(30.0), b[6] - np.float32(30.0)
    if photometric:
        b = APM.exposed(b, 0.8, 12.0)
    if dtype == np.uint8:
        assert b.min() >= 0.5 and b.max() <= 254.5 and a.min() >= 0.5 and a.max() <= 254.5
        a, b = np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8)
    model = np.stack([ident, AM.pushed(planted, H, W, kind, 0.5), off, shifted, ident, nan, ident, AM.pushed(oplanted, H, W, kind, 0.5)])
    return np.ascontiguousarray(a), np.ascontiguousarray(b), model, np.array([1, 0, 1, 1, 1, 1, 1, 1], np.int32)
