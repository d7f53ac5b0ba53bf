"""The statement of the homography fit (oflk_estimate_homography, oflk_tracks_homography) and of the perspective warp
(oflk_warp_perspective) in NumPy.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_homography.hpp) are held to it byte for byte.

One step, with hash index `index`: correspondences src[n] -> dst[n] (float32 (x, y)), a validity mask, Hn hypotheses, a
threshold in pixels and a seed.  A model is nine float32 in row-major order [h00 h01 h02; h10 h11 h12; h20 h21 h22] with
h22 == 1.0f exactly: dst = (h00 x + h01 y + h02, h10 x + h11 y + h12) / (h20 x + h21 y + h22).

1. Compaction, as motion_model's: the mask byte non-zero (no mask: always) and four finite coordinates, in slot order.
   M < 4: the failure result (nine NaNs, mask 0, counts (0, M, 0)).
2. Sampling.  m = 4 picks by motion_model's rule: pick j is r = draw(seed, index, h, j) % (M - j), mapped to the r-th position
   not yet picked, ascending: r is bumped once for each earlier pick, taken in ascending order, that is <= it (`sample`).
3. Minimal solve (`minimal`), float64 on the points converted to double, every operation rounded on its own.  The map of the
   unit square onto a quadrilateral (x0, y0) .. (x3, y3), in pick order (`square_to_quad`, Heckbert's formula):
       sx = (x0 - x1) + (x2 - x3), sy likewise;  dx1 = x1 - x2, dx2 = x3 - x2, dy1, dy2 likewise
       den = dx1 dy2 - dy1 dx2;  g = (sx dy2 - sy dx2) / den;  h = (dx1 sy - dy1 sx) / den
       Q = [(x1 - x0) + g x1, (x3 - x0) + h x3, x0;  (y1 - y0) + g y1, (y3 - y0) + h y3, y0;  g, h, 1]
   S is Q of the four source points, D of the four destination points.  Hm = D adj(S): the adjugate's entries are the nine
   cofactors written in `adjugate` (each a b - c d), the product's entries (r0 c0 + r1 c1) + r2 c2.  The nine entries
   divided by Hm[2][2] and rounded to float32.  Degenerate (score -1): den == 0 on either side, Hm[2][2] == 0, or a
   coefficient that is not finite after the rounding.
4. Score in float32, one operation at a time (`inlier_test`): w = (h20 px + h21 py) + h22;
   ex = ((h00 px + h01 py) + h02) / w - qx, ey likewise (IEEE division); r2 = ex ex + ey ey.  Inlier: w > 0 and
   r2 <= threshold * threshold (the product in float32).  The score counts the inliers among the valid; the best hypothesis
   has the largest score, ties to the lowest h.  Every hypothesis degenerate: the failure result.
5. Refit (`refit`) over the best hypothesis's inliers, float64, every sum in motion_model.lane_sum's order.
   (a) the count n and the four coordinate sums give the centroids cpx, cpy, cqx, cqy (sum / n)
   (b) lp = sum(|X - cpx| + |Y - cpy|), lq likewise on the destination;  sp = n / lp, sq = n / lq.  No square root
   (c) x = (X - cpx) sp, y = (Y - cpy) sp, u = (U - cqx) sq, v = (V - cqy) sq
   (d) the normal equations G h = b of the rows [x y 1 0 0 0 -xu -yu | u] and [0 0 0 x y 1 -xv -yv | v].  With
       xx = x x, xy = x y, yy = y y, r = u u + v v, the 22 sums are of
           xx, xy, yy, x, y;   xx u, xy u, yy u, x u, y u;   xx v, xy v, yy v, x v, y v;   xx r, xy r, yy r;   u, v, x r, y r
       (a three-factor term is the two-factor product times the third); the count fills G[2][2] and G[5][5] (`normal`)
   (e) Gaussian elimination without pivoting on the 8 x 9 array [G | b]: for k = 0 .. 7, for i = k+1 .. 7,
       f = G[i][k] / G[k][k], G[i][j] = G[i][j] - f G[k][j] for j = k+1 .. 8 ascending; then h[i] = (b[i] - the products
       G[i][j] h[j] subtracted one by one for j = i+1 .. 7 ascending) / G[i][i] for i = 7 .. 0 (`solve8`)
   (f) denormalised entry by entry (`denormalise`): A = Hn T_p with tx = sp cpx, ty = sp cpy: A[r][0] = Hn[r][0] sp,
       A[r][1] = Hn[r][1] sp, A[r][2] = Hn[r][2] - (Hn[r][0] tx + Hn[r][1] ty);  B = T_q^-1 A: B[0][c] = A[0][c] / sq + cqx A[2][c],
       B[1][c] = A[1][c] / sq + cqy A[2][c], B[2][c] = A[2][c];  the nine entries divided by B[2][2] and rounded to float32
   The best hypothesis's model is kept when there is no inlier, lp or lq is zero, a pivot is zero or not finite, B[2][2] is
   zero or a result is not finite in float32.
6. Outputs: model [9]; inlier [N]: step 4's test with the returned model on the valid correspondences, 0 elsewhere;
   counts = (sum of the mask, M, 1).

Perspective warp (`warp`; the affine one is stabilize_model.warp): map [F][9] float64, out[f][y][x] = sample(frame f, xs, ys),
    w = (m6 f64(x) + m7 f64(y)) + m8;  xs = ((m0 x + m1 y) + m2) / w;  ys = ((m3 x + m4 y) + m5) / w
two IEEE float64 divisions, not one reciprocal.  inside = w > 0 and 0 <= xs <= W-1 and 0 <= ys <= H-1 (a NaN anywhere: outside);
the sample is track_model.sample and 0 where outside; uint8 frames give (uint8) rint(sample), half to even.  A map whose
third row is (0, 0, 1) gives w == 1, so the bytes of stabilize_model.warp under its first two rows.
"""
import numpy as np

import motion_model as MM
from motion_model import draw, lane_sum, same, tracks_valid, valid_mask  # noqa: F401  (the statement's shared parts)
from track_model import sample as bilinear

SAMPLE = 4
LANES = MM.LANES
MAX_HYPOTHESES = MM.MAX_HYPOTHESES


def sample(seed, index, hyps, m, M):
    """(Hn, m) positions in 0 .. M-1, distinct per row, in pick order; m <= 3 is motion_model.sample"""
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
        elif j == 3:
            a, b, c = out[:, 0], out[:, 1], out[:, 2]
            lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
            mid = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))
            p = p + (p >= lo)
            p = p + (p >= mid)
            p = p + (p >= hi)
        out[:, j] = p
    return out


def square_to_quad(x, y):
    """x, y: four float64 arrays each (the corners in pick order) -> (the nine entries of Q row-major, den)"""
    x0, x1, x2, x3 = x
    y0, y1, y2, y3 = y
    sx = (x0 - x1) + (x2 - x3)
    sy = (y0 - y1) + (y2 - y3)
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dy1 * dx2
    g = (sx * dy2 - sy * dx2) / den
    h = (dx1 * sy - dy1 * sx) / den
    one = np.ones_like(den)
    return [(x1 - x0) + g * x1, (x3 - x0) + h * x3, x0,
            (y1 - y0) + g * y1, (y3 - y0) + h * y3, y0,
            g, h, one], den


def adjugate(s):
    """the nine cofactors of the row-major 3 x 3 s, transposed: s adj(s) = det(s) I"""
    a, b, c, d, e, f, g, h, i = s
    return [e * i - f * h, c * h - b * i, b * f - c * e,
            f * g - d * i, a * i - c * g, c * d - a * f,
            d * h - e * g, b * g - a * h, a * e - b * d]


def minimal(p, q):
    """p, q: (Hn, 4, 2) float64.  Returns ((Hn, 9) float32 coefficients, (Hn,) degenerate)"""
    with np.errstate(all="ignore"):
        S, dens = square_to_quad([p[:, k, 0] for k in range(4)], [p[:, k, 1] for k in range(4)])
        D, dend = square_to_quad([q[:, k, 0] for k in range(4)], [q[:, k, 1] for k in range(4)])
        A = adjugate(S)
        Hm = [(D[3 * r] * A[c] + D[3 * r + 1] * A[3 + c]) + D[3 * r + 2] * A[6 + c] for r in range(3) for c in range(3)]
        c32 = np.stack([e / Hm[8] for e in Hm], -1).astype(np.float32)
    bad = (dens == 0.0) | (dend == 0.0) | (Hm[8] == 0.0)
    return c32, bad | ~np.isfinite(c32).all(-1)


def inlier_test(c, px, py, qx, qy, thr2):
    """float32, one operation at a time; c[..., k] broadcasts against the points"""
    with np.errstate(all="ignore"):
        w = (c[..., 6] * px + c[..., 7] * py) + c[..., 8]
        ex = ((c[..., 0] * px + c[..., 1] * py) + c[..., 2]) / w - qx
        ey = ((c[..., 3] * px + c[..., 4] * py) + c[..., 5]) / w - qy
        r2 = ex * ex + ey * ey
        return (w > 0) & (r2 <= thr2)


def normalised(px, py, qx, qy, inl):
    """steps (a) - (c): (n, (cpx, cpy, cqx, cqy), (sp, sq), (lp, lq), (x, y, u, v))"""
    n = np.float64(int(inl.sum()))
    X, Y, U, V = (a.astype(np.float64) for a in (px, py, qx, qy))
    with np.errstate(all="ignore"):
        cpx, cpy, cqx, cqy = (lane_sum(a, inl) / n for a in (X, Y, U, V))
        lp = lane_sum(np.abs(X - cpx) + np.abs(Y - cpy), inl)
        lq = lane_sum(np.abs(U - cqx) + np.abs(V - cqy), inl)
        sp, sq = n / lp, n / lq
        xyuv = ((X - cpx) * sp, (Y - cpy) * sp, (U - cqx) * sq, (V - cqy) * sq)
    return n, (cpx, cpy, cqx, cqy), (sp, sq), (lp, lq), xyuv


def normal(n, x, y, u, v, inl):
    """step (d): the 8 x 9 array [G | b] in float64"""
    xx, xy, yy, r = x * x, x * y, y * y, u * u + v * v
    terms = [xx, xy, yy, x, y,
             xx * u, xy * u, yy * u, x * u, y * u,
             xx * v, xy * v, yy * v, x * v, y * v,
             xx * r, xy * r, yy * r,
             u, v, x * r, y * r]
    (Sxx, Sxy, Syy, Sx, Sy, Sxxu, Sxyu, Syyu, Sxu, Syu, Sxxv, Sxyv, Syyv, Sxv, Syv, Sxxr, Sxyr, Syyr, Su, Sv, Sxr,
     Syr) = (lane_sum(t, inl) for t in terms)
    G = np.zeros((8, 9))
    G[0, :3], G[0, 6:] = (Sxx, Sxy, Sx), (-Sxxu, -Sxyu, Sxu)
    G[1, :3], G[1, 6:] = (Sxy, Syy, Sy), (-Sxyu, -Syyu, Syu)
    G[2, :3], G[2, 6:] = (Sx, Sy, n), (-Sxu, -Syu, Su)
    G[3, 3:6], G[3, 6:] = (Sxx, Sxy, Sx), (-Sxxv, -Sxyv, Sxv)
    G[4, 3:6], G[4, 6:] = (Sxy, Syy, Sy), (-Sxyv, -Syyv, Syv)
    G[5, 3:6], G[5, 6:] = (Sx, Sy, n), (-Sxv, -Syv, Sv)
    G[6, :] = (-Sxxu, -Sxyu, -Sxu, -Sxxv, -Sxyv, -Sxv, Sxxr, Sxyr, -Sxr)
    G[7, :] = (-Sxyu, -Syyu, -Syu, -Sxyv, -Syyv, -Syv, Sxyr, Syyr, -Syr)
    return G


def solve8(G):
    """step (e) on a copy of [G | b]: ((8,) float64, ok)"""
    G = np.array(G, np.float64)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(8):
            piv = G[k, k]
            ok = ok and bool(piv != 0.0 and np.isfinite(piv))
            for i in range(k + 1, 8):
                f = G[i, k] / piv
                for j in range(k + 1, 9):
                    G[i, j] = G[i, j] - f * G[k, j]
        h = np.zeros(8)
        for i in range(7, -1, -1):
            s = G[i, 8]
            for j in range(i + 1, 8):
                s = s - G[i, j] * h[j]
            h[i] = s / G[i, i]
    return h, ok


def denormalise(h, c, s):
    """step (f): ((9,) float64 before the division by entry [2][2], that entry)"""
    cpx, cpy, cqx, cqy = c
    sp, sq = s
    Hn = [h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], np.float64(1.0)]
    with np.errstate(all="ignore"):
        tx, ty = sp * cpx, sp * cpy
        A = []
        for r in range(3):
            A += [Hn[3 * r] * sp, Hn[3 * r + 1] * sp, Hn[3 * r + 2] - (Hn[3 * r] * tx + Hn[3 * r + 1] * ty)]
        B = [A[k] / sq + cqx * A[6 + k] for k in range(3)] + [A[3 + k] / sq + cqy * A[6 + k] for k in range(3)] + A[6:]
    return np.array(B, np.float64), B[8]


def refit(best, px, py, qx, qy, inl, detail=None):
    """px .. qy: (M,) float32, inl (M,) bool -> (9,) float32"""
    n, c, s, l, (x, y, u, v) = normalised(px, py, qx, qy, inl)
    with np.errstate(all="ignore"):
        G = normal(n, x, y, u, v, inl)
        h, ok = solve8(G)
        B, b22 = denormalise(h, c, s)
        c32 = (B / b22).astype(np.float32)
    if detail is not None:
        detail.update(G=G, h=h, centroids=c, scales=s, xyuv=(x, y, u, v))
    if n == 0 or l[0] == 0.0 or l[1] == 0.0 or not ok or b22 == 0.0 or not np.isfinite(c32).all():
        return best
    return c32


def estimate(src, dst, valid=None, hypotheses=256, threshold=1.0, seed=0, index=0, detail=None):
    """one step: (model (9,) float32, inlier (N,) uint8, counts (3,) int32 = (n_inliers, n_valid, status)).  detail: a dict
    that receives the best hypothesis, its model, the scores and the refit's intermediates"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 2), np.asarray(dst, np.float32).reshape(-1, 2)
    N = len(src)
    assert hypotheses >= 1 and np.float32(threshold) > 0
    ok = valid_mask(src, dst, valid)
    idx = np.flatnonzero(ok)
    M = len(idx)
    fail = (np.full(9, np.nan, np.float32), np.zeros(N, np.uint8), np.array([0, M, 0], np.int32))
    if M < SAMPLE:
        return fail
    px, py, qx, qy = src[idx, 0], src[idx, 1], dst[idx, 0], dst[idx, 1]
    pos = sample(seed, index, hypotheses, SAMPLE, M)
    p = np.stack([px[pos], py[pos]], -1).astype(np.float64)
    q = np.stack([qx[pos], qy[pos]], -1).astype(np.float64)
    c, bad = minimal(p, q)
    thr2 = np.float32(threshold) * np.float32(threshold)
    score = np.full(hypotheses, -1, np.int64)
    for h0 in range(0, hypotheses, 64):   # in pieces: (64, M) float32 at a time
        score[h0:h0 + 64] = inlier_test(c[h0:h0 + 64, None, :], px[None], py[None], qx[None], qy[None], thr2).sum(1)
    score[bad] = -1
    best = int(np.argmax(score))   # the first of the largest
    if detail is not None:
        detail.update(best=best, best_model=c[best].copy(), score=score, positions=pos, idx=idx)
    if score[best] < 0:
        return fail
    inl = inlier_test(c[best], px, py, qx, qy, thr2)
    if detail is not None:
        detail.update(best_inliers=inl)
    out = refit(c[best], px, py, qx, qy, inl, detail)
    mask = np.zeros(N, np.uint8)
    mask[idx] = inlier_test(out, px, py, qx, qy, thr2)
    return out, mask, np.array([int(mask.sum()), M, 1], np.int32)


def estimate_batch(src, dst, valid=None, hypotheses=256, threshold=1.0, seed=0, step0=0):
    """(S, N, 2) steps, step s hashed with index step0 + s: (model (S, 9), inlier (S, N), counts (S, 3))"""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    S = src.shape[0]
    r = [estimate(src[s], dst[s], None if valid is None else np.asarray(valid)[s], hypotheses, threshold, seed, step0 + s)
         for s in range(S)]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


def tracks(tracks_, visible, born=None, hypotheses=256, threshold=1.0, seed=0, t0=0):
    """the T-1 steps of (T, K, 2) rows, step t from row t to row t + 1 with hash index t0 + t"""
    tr = np.asarray(tracks_, np.float32)
    return estimate_batch(tr[:-1], tr[1:], tracks_valid(visible, born), hypotheses, threshold, seed, t0)


# ---------------------------------------------------------------------------------------------------------------------
# the perspective warp
# ---------------------------------------------------------------------------------------------------------------------
def coordinates(m, H, W):
    """the source position of every output pixel under one 3 x 3 map: (xs, ys, w), (H, W) float64 each"""
    m = np.asarray(m, np.float64).reshape(9)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        w = (m[6] * x + m[7] * y) + m[8]
        return ((m[0] * x + m[1] * y) + m[2]) / w, ((m[3] * x + m[4] * y) + m[5]) / w, w


def warp(frames, maps):
    """frames (F, H, W) float32 or uint8, maps (F, 9) float64 -> (out like frames, inside (F, H, W) uint8)"""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    maps = np.asarray(maps, np.float64).reshape(F, 9)
    out, inside = np.zeros(frames.shape, frames.dtype), np.zeros(frames.shape, np.uint8)
    for f in range(F):
        xs, ys, w = coordinates(maps[f], H, W)
        with np.errstate(invalid="ignore"):
            ins = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        v = np.zeros((H, W), np.float32)
        v[ins] = bilinear(frames[f].astype(np.float32), xs[ins], ys[ins])
        out[f] = np.rint(v).astype(np.uint8) if frames.dtype == np.uint8 else v
        inside[f] = ins
    return out, inside


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = MM.PLANTED
PROJECTIVE_ROW = (2e-5, -1e-5, 1.0)


def planted_homography():
    """motion_model.planted_coefficients with the projective row (2e-5, -1e-5, 1): (9,) float64"""
    return np.concatenate([MM.planted_coefficients(), PROJECTIVE_ROW])


def apply(h, pts):
    """float64 points under the (9,) model h, the plain way"""
    h, p = np.asarray(h, np.float64).reshape(9), np.asarray(pts, np.float64)
    w = h[6] * p[..., 0] + h[7] * p[..., 1] + h[8]
    return np.stack([(h[0] * p[..., 0] + h[1] * p[..., 1] + h[2]) / w, (h[3] * p[..., 0] + h[4] * p[..., 1] + h[5]) / w], -1)


def planted_scene(N, share, seed, h=None):
    """motion_model.planted_scene's points and outliers (the same draws) under the planted homography, applied in float64 and
    rounded to float32.  (src, dst (N, 2) float32, inlier (N,) bool)"""
    rng = np.random.default_rng(seed)
    src = (rng.random((N, 2)) * [1919.0, 1079.0]).astype(np.float32)
    dst = apply(planted_homography() if h is None else h, src)
    out = np.zeros(N, bool)
    out[rng.permutation(N)[:int(round(share * N))]] = True
    d = rng.uniform(5.0, 65.0, (N, 2)) * rng.choice([-1.0, 1.0], (N, 2))
    dst = np.where(out[:, None], dst + d, dst).astype(np.float32)
    return src, dst, ~out


def lstsq_fit(px, py, qx, qy, inl):
    """The independent reference of the refit: float64 np.linalg.lstsq on the normalised design matrix of the statement's
    steps (a) - (c), denormalised by plain matrix products.  (9,) float64"""
    n, c, s, _, (x, y, u, v) = normalised(px, py, qx, qy, inl)
    x, y, u, v = (a[inl] for a in (x, y, u, v))
    k = len(x)
    A = np.zeros((2 * k, 8))
    A[:k, 0], A[:k, 1], A[:k, 2], A[:k, 6], A[:k, 7] = x, y, 1.0, -x * u, -y * u
    A[k:, 3], A[k:, 4], A[k:, 5], A[k:, 6], A[k:, 7] = x, y, 1.0, -x * v, -y * v
    h = np.linalg.lstsq(A, np.concatenate([u, v]), rcond=None)[0]
    Hn = np.append(h, 1.0).reshape(3, 3)
    Tp = np.array([[s[0], 0, -s[0] * c[0]], [0, s[0], -s[0] * c[1]], [0, 0, 1]])
    Tqi = np.array([[1 / s[1], 0, c[2]], [0, 1 / s[1], c[3]], [0, 0, 1]])
    B = Tqi @ Hn @ Tp
    return (B / B[2, 2]).reshape(9)


def edge_cases():
    """[(name, src, dst, valid, hypotheses, threshold)]: the scenes every implementation must agree on"""
    f = np.float32
    out = []
    grid = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0)), -1).reshape(-1, 2).astype(f) * f(7)
    for M in range(SAMPLE):   # fewer valid than the sample: M of N = 5 valid
        v = np.zeros(5, np.uint8)
        v[:M] = 1
        out.append((f"M={M}<4", grid[:5], grid[:5] + f(1), v, 8, 1.0))
    ident = np.tile(f([[12.5, 7.25]]), (9, 1))
    out.append(("identical points", ident, ident + f(2), None, 16, 1.0))
    line = np.stack([np.arange(10.0), 2 * np.arange(10.0) + 1], -1).astype(f)
    out.append(("collinear points", line, line + f([3, 4]), None, 32, 1.0))
    # samples with three collinear points among good ones: a grid has many collinear triples
    out.append(("collinear triples in the samples", grid, grid + f([2, 1]), None, 64, 1.0))
    src, dst = MM.exact_scene()   # integer points under an integer similarity: a homography whose third row is (0, 0, 1)
    out.append(("exact integer scene", src, dst, None, 16, 1.0))
    # a residual exactly on the threshold: integer points under a translation, one displaced by (3, 4), threshold 5
    on = grid + f([2, 1])
    on[7] += f([3, 4])
    out.append(("residual on the threshold", grid, on, None, 64, 5.0))
    bad_s, bad_d = grid.copy(), (grid + f([2, 1])).copy()
    bad_s[3, 0], bad_s[11, 1], bad_d[4, 0], bad_d[20, 1], bad_d[21] = np.nan, np.inf, -np.inf, np.nan, (np.inf, np.nan)
    out.append(("NaN and inf coordinates", bad_s, bad_d, None, 16, 1.0))
    # w <= 0 at valid points: points on both sides of the line w = 0 of [1 0 0; 0 1 0; -1/16 0 1], the far side mapped as the
    # formula maps it; such a point reprojects exactly and is still no inlier
    hw = np.array([1, 0, 0, 0, 1, 0, -1 / 16, 0, 1.0])
    gx = np.stack(np.meshgrid(np.arange(0.0, 40.0, 4.0), np.arange(0.0, 20.0, 4.0)), -1).reshape(-1, 2)
    gx = gx[gx[:, 0] != 16.0].astype(f)
    out.append(("w <= 0 at valid points", gx, apply(hw, gx).astype(f), None, 64, 1.0))
    return out
