"""The statement of the global motion fit (oflk_estimate_motion, oflk_tracks_motion, the tracker's motion row) in NumPy.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_motion.hpp) are held to it byte for byte.

One step, with hash index `index`: correspondences src[n] -> dst[n] (float32 (x, y)), a validity mask, a model family, Hn
hypotheses, a threshold in pixels and a seed.

1. Compaction.  Correspondence n is valid when its mask byte is non-zero (no mask: always) and its four coordinates are
   finite.  The M valid ones keep their slot order: positions 0 .. M-1.  M < m: the failure result (six NaNs, mask 0, counts
   (0, M, 0)).
2. Sampling.  draw(seed, index, h, j) is four rounds of the murmur3 finaliser on uint32 (`draw` below).  Hypothesis h picks m
   distinct positions: pick j is r = draw % (M - j), mapped to the r-th position not yet picked, ascending.  Integers only.
3. Minimal solve in float64 on the points converted to double, every operation rounded on its own (`minimal`), then the six
   coefficients [a00 a01 tx; a10 a11 ty] rounded to float32.  Coincident points (SIMILARITY), a zero determinant (AFFINE) or
   a coefficient that is not finite after the rounding: degenerate, score -1.
4. Score in float32, one operation at a time (`residual2`): r2 <= threshold * threshold (the product in float32) is an
   inlier; the score is the count over the valid correspondences.  The best hypothesis has the largest score, ties to the
   lowest h.  Every hypothesis degenerate: the failure result.
5. Refit: least squares of the family over the inliers of the best hypothesis, centred on the inliers' centroids, float64
   sums of the float32 inputs.  The order of every sum (`lane_sum`): LANES = 256 partials, partial l adds the terms of the
   inlier positions l, l + 256, l + 512, ... in ascending order starting from +0.0, then a tree: for stride 128, 64, ..., 1,
   partial[l] += partial[l + stride] for l < stride.  First the count and the four coordinate sums, which give the centroids
   (sum / count); then the seven sums of products of the centred coordinates (`refit`).  No inlier, a zero determinant
   (AFFINE), a zero spread (SIMILARITY) or a result that is not finite in float32: the best hypothesis's model is kept.
6. Outputs: the model in float32; inlier[n]: the test of step 4 with the returned model on the valid correspondences, 0
   elsewhere; counts = (sum of the mask, M, 1).
"""
import numpy as np

TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
FAMILIES = {"translation": TRANSLATION, "similarity": SIMILARITY, "affine": AFFINE}
SAMPLE = {TRANSLATION: 1, SIMILARITY: 2, AFFINE: 3}
LANES = 256
MAX_HYPOTHESES = 65536

_M32 = np.uint64(0xFFFFFFFF)


def _fmix(x):
    """murmur3's 32-bit finaliser on uint64 arrays that hold uint32 values"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x ^ (x >> np.uint64(16))


def draw(seed, index, h, j):
    """the 32-bit draw of (seed, index, h, j): all uint32, sums wrap; h may be an array"""
    x = _fmix(np.uint64((int(seed) & 0xFFFFFFFF) ^ 0x9E3779B9))
    x = _fmix((x + np.uint64(int(index) & 0xFFFFFFFF)) & _M32)
    x = _fmix((x + np.asarray(h, np.uint64)) & _M32)
    return _fmix((x + np.uint64(j)) & _M32)


def sample(seed, index, hyps, m, M):
    """(Hn, m) positions in 0 .. M-1, distinct per row, in pick order"""
    h = np.arange(hyps, dtype=np.uint64)
    out = np.empty((hyps, m), np.int64)
    for j in range(m):
        p = (draw(seed, index, h, j) % np.uint64(M - j)).astype(np.int64)
        if j == 1:
            p = p + (p >= out[:, 0])
        elif j == 2:
            lo, hi = np.minimum(out[:, 0], out[:, 1]), np.maximum(out[:, 0], out[:, 1])
            p = p + (p >= lo)
            p = p + (p >= hi)
        out[:, j] = p
    return out


def valid_mask(src, dst, valid):
    ok = np.isfinite(src).all(-1) & np.isfinite(dst).all(-1)
    return ok if valid is None else ok & (np.asarray(valid) != 0)


def minimal(model, p, q):
    """p, q: (Hn, m, 2) float64.  Returns ((Hn, 6) float32 coefficients, (Hn,) degenerate)"""
    Hn = p.shape[0]
    one, zero = np.ones(Hn), np.zeros(Hn)
    with np.errstate(all="ignore"):
        p0x, p0y, q0x, q0y = p[:, 0, 0], p[:, 0, 1], q[:, 0, 0], q[:, 0, 1]
        if model == TRANSLATION:
            c = [one, zero, q0x - p0x, zero, one, q0y - p0y]
            bad = np.zeros(Hn, bool)
        elif model == SIMILARITY:
            dx, dy = p[:, 1, 0] - p0x, p[:, 1, 1] - p0y
            ex, ey = q[:, 1, 0] - q0x, q[:, 1, 1] - q0y
            den = dx * dx + dy * dy
            a = (dx * ex + dy * ey) / den
            b = (dx * ey - dy * ex) / den
            c = [a, -b, q0x - (a * p0x - b * p0y), b, a, q0y - (b * p0x + a * p0y)]
            bad = den == 0.0
        else:
            d1x, d1y, d2x, d2y = p[:, 1, 0] - p0x, p[:, 1, 1] - p0y, p[:, 2, 0] - p0x, p[:, 2, 1] - p0y
            e1x, e1y, e2x, e2y = q[:, 1, 0] - q0x, q[:, 1, 1] - q0y, q[:, 2, 0] - q0x, q[:, 2, 1] - q0y
            det = d1x * d2y - d1y * d2x
            a00 = (e1x * d2y - e2x * d1y) / det
            a01 = (e2x * d1x - e1x * d2x) / det
            a10 = (e1y * d2y - e2y * d1y) / det
            a11 = (e2y * d1x - e1y * d2x) / det
            c = [a00, a01, q0x - (a00 * p0x + a01 * p0y), a10, a11, q0y - (a10 * p0x + a11 * p0y)]
            bad = det == 0.0
        c32 = np.stack(c, -1).astype(np.float32)
    return c32, bad | ~np.isfinite(c32).all(-1)


def residual2(c, px, py, qx, qy):
    """float32, one operation at a time; c[..., k] broadcasts against the points"""
    with np.errstate(all="ignore"):
        ex = ((c[..., 0] * px + c[..., 1] * py) + c[..., 2]) - qx
        ey = ((c[..., 3] * px + c[..., 4] * py) + c[..., 5]) - qy
        return ex * ex + ey * ey


def lane_sum(terms, inl):
    """the stated order of a sum over the inlier positions; terms (M,) float64"""
    t = np.where(inl, terms, 0.0)      # adding +0.0 to a partial that began at +0.0 changes nothing
    pad = (-len(t)) % LANES
    rows = np.concatenate([t, np.zeros(pad)]).reshape(-1, LANES)
    acc = np.zeros(LANES)
    for r in rows:
        acc = acc + r
    st = LANES // 2
    while st >= 1:
        acc[:st] = acc[:st] + acc[st:2 * st]
        st //= 2
    return acc[0]


def refit(model, best, px, py, qx, qy, inl):
    """px .. qy: (M,) float32, inl (M,) bool -> (6,) float32"""
    n = int(inl.sum())
    X, Y, U, V = (a.astype(np.float64) for a in (px, py, qx, qy))
    with np.errstate(all="ignore"):
        nn = np.float64(n)
        cpx, cpy, cqx, cqy = (lane_sum(a, inl) / nn for a in (X, Y, U, V))
        ux, uy, vx, vy = X - cpx, Y - cpy, U - cqx, V - cqy
        suu, suv, svv = lane_sum(ux * ux, inl), lane_sum(ux * uy, inl), lane_sum(uy * uy, inl)
        sux, svx = lane_sum(ux * vx, inl), lane_sum(uy * vx, inl)
        suy, svy = lane_sum(ux * vy, inl), lane_sum(uy * vy, inl)
        if model == TRANSLATION:
            c = [1.0, 0.0, cqx - cpx, 0.0, 1.0, cqy - cpy]
            singular = False
        elif model == SIMILARITY:
            den = suu + svv
            a = (sux + svy) / den
            b = (suy - svx) / den
            c = [a, -b, cqx - (a * cpx - b * cpy), b, a, cqy - (b * cpx + a * cpy)]
            singular = den == 0.0
        else:
            det = suu * svv - suv * suv
            a00 = (sux * svv - svx * suv) / det
            a01 = (svx * suu - sux * suv) / det
            a10 = (suy * svv - svy * suv) / det
            a11 = (svy * suu - suy * suv) / det
            c = [a00, a01, cqx - (a00 * cpx + a01 * cpy), a10, a11, cqy - (a10 * cpx + a11 * cpy)]
            singular = det == 0.0
        c32 = np.array(c, np.float64).astype(np.float32)
    if n == 0 or singular or not np.isfinite(c32).all():
        return best
    return c32


def estimate(src, dst, valid=None, model=SIMILARITY, hypotheses=256, threshold=1.0, seed=0, index=0, detail=None):
    """one step: (model (6,) float32, inlier (N,) uint8, counts (3,) int32 = (n_inliers, n_valid, status)).  detail: a dict
    that receives the best hypothesis, its model and the scores"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 2), np.asarray(dst, np.float32).reshape(-1, 2)
    N, m = len(src), SAMPLE[model]
    assert hypotheses >= 1 and np.float32(threshold) > 0
    ok = valid_mask(src, dst, valid)
    idx = np.flatnonzero(ok)
    M = len(idx)
    fail = (np.full(6, np.nan, np.float32), np.zeros(N, np.uint8), np.array([0, M, 0], np.int32))
    if M < m:
        return fail
    px, py, qx, qy = src[idx, 0], src[idx, 1], dst[idx, 0], dst[idx, 1]
    pos = sample(seed, index, hypotheses, m, M)
    p = np.stack([px[pos], py[pos]], -1).astype(np.float64)
    q = np.stack([qx[pos], qy[pos]], -1).astype(np.float64)
    c, bad = minimal(model, p, q)
    thr2 = np.float32(threshold) * np.float32(threshold)
    score = np.full(hypotheses, -1, np.int64)
    for h0 in range(0, hypotheses, 64):   # in pieces: (64, M) float32 at a time
        r2 = residual2(c[h0:h0 + 64, None, :], px[None], py[None], qx[None], qy[None])
        score[h0:h0 + 64] = (r2 <= thr2).sum(1)
    score[bad] = -1
    best = int(np.argmax(score))   # the first of the largest
    if detail is not None:
        detail.update(best=best, best_model=c[best].copy(), score=score, positions=pos, idx=idx)
    if score[best] < 0:
        return fail
    inl = residual2(c[best], px, py, qx, qy) <= thr2
    out = refit(model, c[best], px, py, qx, qy, inl)
    mask = np.zeros(N, np.uint8)
    mask[idx] = residual2(out, px, py, qx, qy) <= thr2
    return out, mask, np.array([int(mask.sum()), M, 1], np.int32)


def estimate_batch(src, dst, valid=None, model=SIMILARITY, hypotheses=256, threshold=1.0, seed=0, step0=0):
    """(S, N, 2) steps, step s hashed with index step0 + s: (model (S, 6), inlier (S, N), counts (S, 3))"""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    S = src.shape[0]
    r = [estimate(src[s], dst[s], None if valid is None else np.asarray(valid)[s], model, hypotheses, threshold, seed, step0 + s)
         for s in range(S)]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


def tracks_valid(visible, born=None):
    """(T, K) rows -> (T-1, K): visible on both rows of the step and not born on the later one"""
    vis = np.asarray(visible) != 0
    v = vis[:-1] & vis[1:]
    return v if born is None else v & ~(np.asarray(born)[1:] != 0)


def tracks(tracks_, visible, born=None, model=SIMILARITY, hypotheses=256, threshold=1.0, seed=0, t0=0):
    """the T-1 steps of (T, K, 2) rows, step t from row t to row t + 1 with hash index t0 + t"""
    tr = np.asarray(tracks_, np.float32)
    return estimate_batch(tr[:-1], tr[1:], tracks_valid(visible, born), model, hypotheses, threshold, seed, t0)


def same(got, want, what=""):
    """byte for byte; a NaN equals a NaN"""
    for g, w, name in zip(got, want, ("model", "inlier", "counts")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} != {w.shape}"
        if g.dtype.kind == "f":
            eq = (g.view(np.uint32) == w.astype(np.float32).view(np.uint32)) | (np.isnan(g) & np.isnan(w))
        else:
            eq = g.astype(np.int64) == w.astype(np.int64)
        assert eq.all(), f"{what}: {name} differs at {np.argwhere(~eq)[:5].tolist()}: got {g[~eq][:5]}, want {w[~eq][:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = [(200, 0.4, 256), (65, 0.4, 256), (1000, 0.5, 256), (24, 0.25, 64)]   # (N, outlier share, Hn)


def planted_coefficients():
    """rotation 2 degrees, scale 1.01, translation (3.5, -2.25), float64 [a00 a01 tx a10 a11 ty]"""
    th = np.deg2rad(2.0)
    a, b = 1.01 * np.cos(th), 1.01 * np.sin(th)
    return np.array([a, -b, 3.5, b, a, -2.25])


def planted_scene(N, share, seed):
    """points uniform in 1919 x 1079 under the planted transform; a share of them displaced by 5 to 65 px per axis.
    (src, dst (N, 2) float32, inlier (N,) bool)"""
    rng = np.random.default_rng(seed)
    src = (rng.random((N, 2)) * [1919.0, 1079.0]).astype(np.float32)
    c = planted_coefficients()
    s = src.astype(np.float64)
    dst = np.stack([c[0] * s[:, 0] + c[1] * s[:, 1] + c[2], c[3] * s[:, 0] + c[4] * s[:, 1] + c[5]], -1)
    out = np.zeros(N, bool)
    out[rng.permutation(N)[:int(round(share * N))]] = True
    d = rng.uniform(5.0, 65.0, (N, 2)) * rng.choice([-1.0, 1.0], (N, 2))
    dst = np.where(out[:, None], dst + d, dst).astype(np.float32)
    return src, dst, ~out


def lstsq_fit(model, src, dst, inl):
    """float64 np.linalg.lstsq of the family over the correspondences of `inl`: the independent reference of the refit"""
    s, d = src[inl].astype(np.float64), dst[inl].astype(np.float64)
    n = len(s)
    if model == TRANSLATION:
        t = (d - s).mean(0)
        return np.array([1.0, 0.0, t[0], 0.0, 1.0, t[1]])
    if model == AFFINE:
        A = np.column_stack([s, np.ones(n)])
        return np.concatenate([np.linalg.lstsq(A, d[:, 0], rcond=None)[0], np.linalg.lstsq(A, d[:, 1], rcond=None)[0]])
    A = np.zeros((2 * n, 4))
    A[:n, 0], A[:n, 1], A[:n, 2] = s[:, 0], -s[:, 1], 1.0
    A[n:, 0], A[n:, 1], A[n:, 3] = s[:, 1], s[:, 0], 1.0
    a, b, tx, ty = np.linalg.lstsq(A, np.concatenate([d[:, 0], d[:, 1]]), rcond=None)[0]
    return np.array([a, -b, tx, b, a, ty])


def exact_scene(N=40, seed=5):
    """integer points under an integer similarity (a, b) = (2, 1), t = (3, -4): exact in float32, no outliers"""
    rng = np.random.default_rng(seed)
    src = rng.permutation(200 * 100)[:N]
    src = np.stack([src % 200, src // 200], -1).astype(np.float32)
    dst = np.stack([2 * src[:, 0] - src[:, 1] + 3, src[:, 0] + 2 * src[:, 1] - 4], -1).astype(np.float32)
    return src, dst


def edge_cases():
    """[(name, src, dst, valid, model, hypotheses, threshold)]: the scenes every implementation must agree on"""
    f = np.float32
    out = []
    grid = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0)), -1).reshape(-1, 2).astype(f) * f(7)
    for model, m in ((TRANSLATION, 1), (SIMILARITY, 2), (AFFINE, 3)):
        for M in range(m):   # fewer valid than the sample: M of N = 5 valid
            v = np.zeros(5, np.uint8)
            v[:M] = 1
            out.append((f"M={M}<m={m}", grid[:5], grid[:5] + f(1), v, model, 8, 1.0))
    same = np.tile(f([[12.5, 7.25]]), (9, 1))
    out.append(("identical points, similarity", same, same + f(2), None, SIMILARITY, 16, 1.0))
    out.append(("identical points, affine", same, same + f(2), None, AFFINE, 16, 1.0))
    line = np.stack([np.arange(10.0), 2 * np.arange(10.0) + 1], -1).astype(f)
    out.append(("collinear points, affine", line, line + f([3, 4]), None, AFFINE, 32, 1.0))
    out.append(("collinear points, similarity", line, line + f([3, 4]), None, SIMILARITY, 32, 1.0))
    src, dst = exact_scene()
    for model in (TRANSLATION, SIMILARITY, AFFINE):
        d = src + f([3, -4]) if model == TRANSLATION else dst
        out.append((f"exact model, family {model}", src, d, None, model, 16, 1.0))
    # a residual exactly on the threshold: integer points under a translation, one displaced by (3, 4), threshold 5
    on = grid + f([2, 1])
    on[7] += f([3, 4])
    for model in (TRANSLATION, SIMILARITY, AFFINE):
        out.append((f"residual on the threshold, family {model}", grid, on, None, model, 64, 5.0))
    bad_s, bad_d = grid.copy(), (grid + f([2, 1])).copy()
    bad_s[3, 0], bad_s[11, 1], bad_d[4, 0], bad_d[20, 1], bad_d[21] = np.nan, np.inf, -np.inf, np.nan, (np.inf, np.nan)
    for model in (TRANSLATION, SIMILARITY, AFFINE):
        out.append((f"NaN and inf coordinates, family {model}", bad_s, bad_d, None, model, 16, 1.0))
    return out
