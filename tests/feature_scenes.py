"""Scenes for the corner selection's rarer paths, and checks that each scene reaches its path (test infrastructure; the
product never imports this module).

Noise frames almost never tie, so on them the select kernel's radix descent stops inside the score bits and its batches
rarely hold conflicts.  The scenes here are built to do the opposite:

- lattice: identical 2 x 2 blobs every `step` px.  Each blob gives a 2 x 2 plateau of one score (four adjacent candidates),
  and every blob the same plateau, so at 1080p ~1.7e5 candidates share the top score and the descent cuts slabs inside
  the raster-index digits.
- chain_rows: rows of 2 x 2 blobs `CHAIN_STEP` px apart, rows `CHAIN_GAP` px apart.  At md = CHAIN_MD (step < md < 2 step,
  gap - 1 > md) a blob conflicts with its two neighbours in the row and nothing else, so in priority order the
  candidates form long chains, each conflicting with the one before it.
- exact_pairs: single-pixel dots, window 3: each dot is exactly one candidate, so candidate pairs lie at exact offsets.

Every frame is float32.  brute_select is the statement's greedy with no grid (each candidate against every accepted
point, float64); feature_model.select must equal it.
"""
from __future__ import annotations

import numpy as np

import feature_model as M

LATTICE_STEP = 7
CHAIN_STEP, CHAIN_GAP, CHAIN_MD = 7, 12, 10.0
CHAIN_ORDERS = ("increasing", "decreasing", "alternating")
PAIR_OFFSETS = ((3, 4), (4, 3), (5, 0), (0, 5), (2, 1), (1, 2), (2, 2))   # (dx, dy)
PAIR_SPACING = 16


def f32_next(v, toward):
    """the float32 next to v toward +inf or -inf, as a Python float (exact in float32: the C ABI's md)"""
    return float(np.nextafter(np.float32(v), np.float32(toward)))


def lattice(H=1080, W=1920, contrasts=(190.0,), step=LATTICE_STEP, bg=60.0, off=3, shift=(0, 0)):
    """2 x 2 blobs at (off + i*step, off + j*step) + shift on a flat background; blob (i, j) has contrasts[(i + j) %
    len(contrasts)]"""
    f = np.full((H, W), bg, np.float32)
    y0, x0 = off + shift[0], off + shift[1]
    for i, y in enumerate(range(y0, H - 1, step)):
        for j, x in enumerate(range(x0, W - 1, step)):
            f[y:y + 2, x:x + 2] = contrasts[(i + j) % len(contrasts)]
    return f


def chain_rows(order, H=1080, W=1920, bg=20.0, off=3):
    """rows of 2 x 2 blobs; order sets the priority along each row:
    increasing   every blob 190: ties, so priority follows the raster index (left to right)
    decreasing   blob k of row r at 100 + 0.1 (r n + k): each blob its own score, rising with x, so the row is taken right
                 to left
    alternating  even blobs on a high ramp, odd blobs on a low one (each blob its own score): high, low, high, ... along
                 the row"""
    assert order in CHAIN_ORDERS
    f = np.full((H, W), bg, np.float32)
    xs = list(range(off, W - 1, CHAIN_STEP))
    n = len(xs)
    for r, y in enumerate(range(off, H - 1, CHAIN_GAP)):
        for k, x in enumerate(xs):
            if order == "increasing":
                v = 190.0
            elif order == "decreasing":
                v = 100.0 + 0.1 * (r * n + k)
            else:
                v = 100.0 + 0.1 * (r * n + k) + (0.1 * n * (H // CHAIN_GAP + 1) if k % 2 == 0 else 0.0)
            f[y:y + 2, x:x + 2] = np.float32(v)
    return f


def exact_pairs(rows=6, cols=70, bg=60.0, fg=190.0):
    """rows x cols cells of PAIR_SPACING px, cell (i, j) a pair of single-pixel dots at offset PAIR_OFFSETS[j % 7] (window
    3: one candidate each; ~120 candidates lie between a dot and its partner one row down, so some pairs share a 256-key
    batch and some do not); returns (frame, [(dx, dy, (x, y), (x + dx, y + dy))])"""
    H, W = PAIR_SPACING * (rows + 1), PAIR_SPACING * (cols + 1)
    f = np.full((H, W), bg, np.float32)
    pairs = []
    for i in range(rows):
        for j in range(cols):
            dx, dy = PAIR_OFFSETS[j % len(PAIR_OFFSETS)]
            y, x = PAIR_SPACING * (i + 1) - 3, PAIR_SPACING * (j + 1) - 3
            f[y, x] = f[y + dy, x + dx] = fg
            pairs.append((dx, dy, (x, y), (x + dx, y + dy)))
    return f, pairs


def _noise(H, W, seed, scale=255.0):
    return (np.random.default_rng(seed).random((H, W)) * scale).astype(np.float32)


def bad_pixel_sites(H, W):
    """(y, x) of pixels in the interior, on the border and on the score kernel's 64 x 16 tile seams"""
    sites = [(H // 2, W // 2), (0, 0), (H - 1, W - 1), (0, W // 3), (H // 2, 0), (H // 2, W - 1), (H - 1, W // 5)]
    sites += [(H // 3, x) for x in (63, 64, 127, 128) if x < W]
    sites += [(y, W // 4 + 7) for y in (15, 16, 31, 32) if y < H]
    return sites


def value_frames(H, W, seed):
    """name -> float32 frame: values in [0, 1), in 0..65535, negative, around 1e19 (squared gradients overflow), around
    1e-20 (squared gradients underflow into subnormals), and a textured frame with NaN, +Inf and -Inf pixels at
    bad_pixel_sites"""
    rng = np.random.default_rng(seed)
    nf = (rng.random((H, W)) * 255).astype(np.float32)
    for i, (y, x) in enumerate(bad_pixel_sites(H, W)):
        nf[y, x] = (np.nan, np.inf, -np.inf)[i % 3]
    return {"unit": rng.random((H, W)).astype(np.float32),
            "u16": rng.integers(0, 65536, (H, W)).astype(np.float32),
            "negative": (-1000.0 - 300.0 * rng.random((H, W))).astype(np.float32),
            "huge": (4e19 * rng.random((H, W))).astype(np.float32),
            "tiny": (1e-20 * rng.random((H, W))).astype(np.float32),
            "nonfinite": nf}


GRID_SHAPES = [(1, 1), (2, 3), (5, 5), (7, 9), (17, 33), (64, 80), (240, 320)]


def grid_frame(H, W):
    return _noise(H, W, seed=H * 7 + W)


def grid_mds(H, W):
    """min_distance around the clamp of the grid's cell to max(H, W): one float32 step below it, at it, 1.5 below it (two
    cells), between it and the diagonal, and 1e30 (one cell)"""
    L = max(H, W)
    mds = [f32_next(L, -np.inf), float(L), float(np.float32((L + np.hypot(H, W)) / 2)), 1e30]
    return mds + ([L - 1.5] if L > 2 else [])


def small_frames(H=12, W=12):
    """eight unlike small frames: noise (three), empty, one blob, a lattice, a ramp (no corners) and noise with a NaN"""
    blob = np.full((H, W), 60.0, np.float32)
    blob[H // 2:H // 2 + 2, W // 3:W // 3 + 2] = 190.0
    ramp = (np.add.outer(np.arange(H), 3 * np.arange(W)) * 5.0).astype(np.float32)
    nan = _noise(H, W, 4)
    nan[H // 2, W // 2] = np.nan
    return [_noise(H, W, 1), _noise(H, W, 2), _noise(H, W, 3), np.zeros((H, W), np.float32), blob,
            lattice(H, W), ramp, nan]


TALL_H, TALL_W = 1048600, 24


def tall_frame():
    """TALL_H x TALL_W lattice; the blobs in the last 64 rows (230) and in rows 262 136 - 262 199 (210) outrank the rest
    (190): the score launch's 65 535th tile row starts at 1 048 560, the candidate launch's 65 535th row block at 262 140"""
    f = lattice(TALL_H, TALL_W)
    f[TALL_H - 64:][f[TALL_H - 64:] == 190.0] = 230.0
    f[262136:262200][f[262136:262200] == 190.0] = 210.0
    return f


def truncate(res, K):
    """the statement's result for max_corners K from its result for a larger K: the greedy stops after K acceptances"""
    n, xy, sc = res
    m = min(n, K)
    out_xy = np.full((K, 2), np.nan, np.float32)
    out_sc = np.zeros(K, np.float32)
    out_xy[:m], out_sc[:m] = xy[:m], sc[:m]
    return m, out_xy, out_sc


# ---------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------
def top_ties(S, q=0.0):
    """the number of candidates that share the top score"""
    ys, xs, _ = M.candidates(S, q)
    if not len(ys):
        return 0
    s = S[ys, xs]
    return int((s == s[0]).sum())


def conflict_runs(S, q, md):
    """the longest run of consecutive candidates in priority order, each within md (dx^2 + dy^2 < md^2) of the one before"""
    ys, xs, _ = M.candidates(S, q)
    md2 = float(np.float32(md)) ** 2
    d2 = (np.diff(xs) ** 2 + np.diff(ys) ** 2).astype(np.float64)
    best = run = 1 if len(ys) else 0
    for c in (d2 < md2).tolist():
        run = run + 1 if c else 1
        best = max(best, run)
    return best


def candidate_offsets(S, q=0.0):
    """the set of (dx, dy) between candidates that are not more than 5 px apart in x and y"""
    ys, xs, _ = M.candidates(S, q)
    pts = set(zip(xs.tolist(), ys.tolist()))
    out = set()
    for x, y in pts:
        for dy in range(0, 6):
            for dx in range(-5, 6):
                if (dy, dx) > (0, 0) and (x + dx, y + dy) in pts:
                    out.add((dx, dy))
    return out


def brute_select(S, q, md, K):
    """the greedy of the statement with no grid: each candidate in priority order against every accepted point, in
    float64.  Returns (count, xy (K, 2), score (K,)) as feature_model.select."""
    S = np.asarray(S, np.float32)
    ys, xs, _ = M.candidates(S, q)
    md2 = float(np.float32(md)) ** 2
    ax = np.empty(len(ys), np.float64)
    ay = np.empty(len(ys), np.float64)
    n = 0
    for y, x in zip(ys.tolist(), xs.tolist()):
        if n == K:
            break
        if n and (((ax[:n] - x) ** 2 + (ay[:n] - y) ** 2) < md2).any():
            continue
        ax[n], ay[n] = x, y
        n += 1
    xy = np.full((K, 2), np.nan, np.float32)
    sc = np.zeros(K, np.float32)
    xy[:n, 0], xy[:n, 1] = ax[:n], ay[:n]
    sc[:n] = S[ay[:n].astype(np.int64), ax[:n].astype(np.int64)]
    return n, xy, sc


def check_greedy_output(S, md, n, xy, sc):
    """what can be checked of a selection at full size without the quadratic greedy: the accepted points are candidates'
    pixels in priority order (score descending, then raster index), their scores are S there, no two lie closer than md,
    and rows from n on are (NaN, NaN), score 0"""
    from scipy.spatial import cKDTree

    S = np.asarray(S, np.float32)
    W = S.shape[1]
    p = xy[:n].astype(np.int64)
    assert np.array_equal(p.astype(np.float32), xy[:n]), "integer pixel positions"
    assert np.array_equal(sc[:n], S[p[:, 1], p[:, 0]])
    s = S[p[:, 1], p[:, 0]].astype(np.float64)
    r = p[:, 1] * W + p[:, 0]
    ok = (s[1:] < s[:-1]) | ((s[1:] == s[:-1]) & (r[1:] > r[:-1]))
    assert ok.all(), f"priority order broken at {np.flatnonzero(~ok)[:5]}"
    md = float(np.float32(md))
    if n > 1 and md > 1.0:
        pairs = cKDTree(p.astype(np.float64)).query_pairs(md, output_type="ndarray")
        if len(pairs):
            d2 = ((p[pairs[:, 0]] - p[pairs[:, 1]]) ** 2).sum(1).astype(np.float64)
            assert (d2 >= md * md).all(), f"{(d2 < md * md).sum()} accepted pairs closer than md"
    assert np.isnan(xy[n:]).all() and (sc[n:] == 0).all()
