"""Scenes for the step loops of the fits and of direct alignment past the grid limit (tests/test_gpu_step_loops.py).

Test infrastructure: the product never imports this file.

Every batched kernel puts its steps on a grid axis of at most GRID = 65 535 blocks and reaches later steps by
`for (s = blockIdx; s < S; s += gridDim)`.  S = GRID + 14 steps cycle through P = 7 kinds, kind(s) = s % 7.  GRID % 7 == 1, so
the block that does step s in its first pass does step s + GRID, of kind kind(s) + 1, in its second: the 14 steps of the
second pass take each of the seven transitions k -> k + 1 twice.  The kinds are ordered so that each transition hands the
block's LDS state and its barriers from one path of the loop body to another one.

The fits (`fit_batch`), N = 12 correspondences, Hn = 4 hypotheses, threshold 1, a mask, step0 = 17; m is the family's sample
    0  a planted scene that fits                   1  no valid correspondence (M = 0)
    2  a planted scene with a NaN and an inf coordinate and three masked slots
    3  exactly m - 1 valid correspondences         4  a planted scene with another outlier share
    5  nine valid points, all identical: every hypothesis is degenerate, the failure branch with M >= m.  The translation
       family has no degenerate sample but one whose difference is not finite in float32, so its points are
       (-3e38, -3e38) -> (3e38, 3e38)
    6  a planted scene with two masked slots: another valid count than kind 0's
and every coordinate of step s is moved by (s % 251) / 4 px, source and destination alike, so that a row read at the wrong
step differs even between steps of one kind.

Direct alignment (`align_pairs`, `align_frames`), frames of 16 x 24
    0  a planted pair from a pushed model          1  a held step (status_in 0)
    2  a planted pair of another seed and move     3  a model that throws B off the frame (count 0, a NaN `before`)
    4  equal frames under the identity             5  align_model.checker_pair under the identity (rejected: status 2)
    6  a flat template (frozen at the first iteration)
The photometric form re-exposes B of kinds 0 and 2.  It takes the checker pair's one grey level for a bias and refines the
step, so its kind 5 has B = A + x / 20 instead: a steeper ramp, which asks for a stretch that blurs the checkerboard as the
shift does, and which no gain and bias explain (`rejected_pair`).  The sequence form's frames cycle with period 7, step s
being the pair (frame s % 7, frame (s + 1) % 7), so a frame is the image of one kind and the template of the next: the frames
are A0, B0, A2, B2, checker A, checker A, checker B.  Kinds 0, 2, 4 and 5 are the pair form's; the held step and the thrown
one take the frames they get; kind 6 has the checker's B as its template, which is not flat, and freezes at the first
iteration by a model that leaves a sixth of the frame in sight (a count above 0 and below min_share).
"""
import numpy as np

import align_model as AM
import align_photo_model as APM
import homography_model as HM
import motion_model as MM

GRID = 65535
P = 7
S = GRID + 2 * P

# ---------------------------------------------------------------------------------------------------------------------
# the fits
# ---------------------------------------------------------------------------------------------------------------------
N, HYPS, THRESHOLD, SEED, STEP0 = 12, 4, 1.0, 5, 17
HOMOGRAPHY = "homography"
FAMILIES = [MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE, HOMOGRAPHY]


def sample_size(family):
    return HM.SAMPLE if family == HOMOGRAPHY else MM.SAMPLE[family]


def fit_kinds(family):
    """the seven kinds before the steps' offsets: (src, dst (7, N, 2) float32, valid (7, N) uint8)"""
    planted = HM.planted_scene if family == HOMOGRAPHY else MM.planted_scene
    m = sample_size(family)
    src, dst, valid = np.zeros((P, N, 2), np.float32), np.zeros((P, N, 2), np.float32), np.ones((P, N), np.uint8)
    for k, (share, seed) in {0: (0.25, 31), 2: (0.25, 32), 4: (0.5, 33), 6: (0.25, 34)}.items():
        src[k], dst[k] = planted(N, share, seed)[:2]
    valid[1] = 0
    src[1], dst[1] = src[0], dst[0]
    dst[2, 5, 1], src[2, 9, 0] = np.nan, np.inf
    valid[2, [0, 4, 11]] = 0
    src[3], dst[3] = src[4], dst[4]
    valid[3] = 0
    valid[3, [2, 6, 7, 10][:m - 1]] = 1
    if family == MM.TRANSLATION:
        src[5], dst[5] = -3e38, 3e38
    else:
        src[5], dst[5] = (12.5, 7.25), (14.5, 9.25)
    valid[5, [1, 3, 8]] = 0
    valid[6, [3, 9]] = 0
    return src, dst, valid


def offsets(steps):
    """the offset of every coordinate of the given steps: (n, 1, 1) float32"""
    return ((np.asarray(steps) % 251).astype(np.float32) * np.float32(0.25))[:, None, None]


def fit_steps(family, steps):
    """the given steps of the batch: (src, dst (n, N, 2) float32, valid (n, N) uint8)"""
    steps = np.asarray(steps)
    src, dst, valid = fit_kinds(family)
    k = steps % P
    with np.errstate(over="ignore"):   # 3e38 + 62.5 is 3e38
        return src[k] + offsets(steps), dst[k] + offsets(steps), np.ascontiguousarray(valid[k])


def fit_batch(family):
    return fit_steps(family, np.arange(S))


def fit_model(family, steps):
    """the statement on the given steps of the batch, step s hashed with index STEP0 + s: (model, inlier, counts)"""
    src, dst, valid = fit_steps(family, steps)
    if family == HOMOGRAPHY:
        r = [HM.estimate(src[i], dst[i], valid[i], HYPS, THRESHOLD, SEED, STEP0 + int(s)) for i, s in enumerate(steps)]
    else:
        r = [MM.estimate(src[i], dst[i], valid[i], family, HYPS, THRESHOLD, SEED, STEP0 + int(s)) for i, s in enumerate(steps)]
    return tuple(np.stack([x[j] for x in r]) for j in range(3))


def sample_steps():
    """the steps held to the statement: 0 .. 13, every 257th, and the last 28, which are 14 on either side of GRID"""
    return np.unique(np.concatenate([np.arange(2 * P), np.arange(0, S, 257), np.arange(GRID - 2 * P, S)]))


# ---------------------------------------------------------------------------------------------------------------------
# direct alignment
# ---------------------------------------------------------------------------------------------------------------------
H, W = 16, 24
GAIN, BIAS = 0.8, 12.0
PLANTED = {0: dict(seed=5, move=1.0, by=0.5), 2: dict(seed=8, move=0.5, by=0.25)}


def _planted(k, kind, photometric):
    A, B, planted = AM.planted_pair(H, W, PLANTED[k]["seed"], kind, move=PLANTED[k]["move"])
    if photometric:
        B = APM.exposed(B, GAIN, BIAS)
    return A, B, AM.pushed(planted, H, W, kind, PLANTED[k]["by"])


def _thrown(kind):
    off = AM.IDENTITY[kind].copy()
    off[2], off[5] = 3.0 * W, -2.0 * H
    return off


def rejected_pair(photometric):
    """kind 5: a step that the refinement makes worse"""
    ca, cb = AM.checker_pair(H, W)
    if photometric:
        x = np.arange(W, dtype=np.float32)[None, :]
        cb = (ca + np.float32(0.05) * x).astype(np.float32)
    return ca, cb


def align_pairs(kind, photometric):
    """the pair form's seven kinds: (a, b (7, H, W) float32, model (7, nc) float32, status (7,) int32)"""
    A0, B0, m0 = _planted(0, kind, photometric)
    A2, B2, m2 = _planted(2, kind, photometric)
    ca, cb = rejected_pair(photometric)
    ident = AM.IDENTITY[kind]
    a = np.stack([A0, A0, A2, A0, A2, ca, np.full((H, W), 9.0, np.float32)])
    b = np.stack([B0, B0, B2, B0, A2, cb, B0])
    model = np.stack([m0, m0, m2, _thrown(kind), ident, ident, ident])
    return a, b, model, np.array([1, 0, 1, 1, 1, 1, 1], np.int32)


def align_frames(kind, photometric, dtype):
    """the sequence form's cycle: (frames (8, H, W) of dtype -- the seven frames and the first again --, model (7, nc) float32,
    status (7,) int32); step k is the pair (frames[k], frames[k + 1])"""
    A0, B0, m0 = _planted(0, kind, photometric)
    A2, B2, m2 = _planted(2, kind, photometric)
    ca, cb = rejected_pair(photometric)
    ident = AM.IDENTITY[kind]
    narrow = ident.copy()
    narrow[2] = 20.0   # columns 20 .. 23 of the image under columns 0 .. 3 of the template: a sixth of the frame
    frames = np.stack([A0, B0, A2, B2, ca, ca, cb, A0])
    frames = np.rint(frames).astype(np.uint8) if dtype == np.uint8 else np.ascontiguousarray(frames, np.float32)
    model = np.stack([m0, m0, m2, _thrown(kind), ident, ident, narrow])
    return frames, model, np.array([1, 0, 1, 1, 1, 1, 1], np.int32)


def tiled(x, n=S):
    """the first n rows of a (7, ...) array repeated with period 7"""
    x = np.asarray(x)
    return np.ascontiguousarray(x[np.arange(n) % P])


def align_model(kind, photometric, form, levels, iterations, dtype=np.float32):
    """the statement on the seven kinds, `form` "pair" or "sequence": (model, status, stats[, photo]) of 7 steps"""
    mod = APM if photometric else AM
    if form == "pair":
        a, b, model, status = align_pairs(kind, photometric)
        return mod.refine(a, b, model, status, kind, levels, iterations)
    frames, model, status = align_frames(kind, photometric, dtype)
    return mod.sequence(frames, model, status, kind, levels, iterations)


# the floor of the alignment's sizes: 8 x 8 per level
FLOOR = [(8, 8, 1), (16, 17, 2), (8, 65, 1)]   # (H, W, levels): the smallest frame; a coarsest level of exactly 8 x 8; one
FLOOR_ITERATIONS = 2                           # tile row and a second tile column of one pixel


def floor_steps(h, w, kind, photometric, dtype):
    """S = 3 planted steps of h x w from pushed models: (a, b (3, h, w) of dtype, model (3, nc) float32)"""
    a, b, model = [], [], []
    for seed in (3, 4, 6):
        A, B, planted = AM.planted_pair(h, w, seed, kind, move=0.5)
        if photometric:
            B = APM.exposed(B, GAIN, BIAS)
        a.append(A)
        b.append(B)
        model.append(AM.pushed(planted, h, w, kind, 0.25))
    a, b = np.stack(a), np.stack(b)
    if dtype == np.uint8:
        return np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8), np.stack(model)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), np.stack(model)
