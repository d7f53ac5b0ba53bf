"""The Shi-Tomasi corner statement in NumPy (test infrastructure; the product never imports this module).

One frame f (H, W): float32, or uint8 converted exactly to float32.  Window w = 2h+1, odd, 3 <= w <= 11.

Score map S (float32, H x W):
    Ix, Iy = the reference's compute_gradients(f, f): frame_avg = (f + f) / 2 (float32), Sobel/8 by
             scipy.signal.convolve2d(..., mode="same", boundary="symm")
    Pxx = Ix*Ix, Pxy = Ix*Iy, Pyy = Iy*Iy                                  (float32, each rounded)
    R[y,x] = ((P[y,x-h] + P[y,x-h+1]) + ...) + P[y,x+h]                    (float32, left to right)
    A[y,x] = ((R[y-h,x] + R[y-h+1,x]) + ...) + R[y+h,x]                    (float32, top to bottom)
    a, b, c = Axx, Axy, Ayy
    S = 0 where y < h, y >= H-h, x < h or x >= W-h (the pixels lucas_kanade_from_gradients skips); elsewhere, in float64
    with each operation rounded (a, b, c widened exactly):
        det = a*c - b*b;  tr = a + c;  d = a - c;  disc = sqrt(d*d + 4*b*b)
        S = f32(2*det / (tr + disc)) if det > 0 else 0                     (the smaller eigenvalue, cancellation-free)
    a non-finite S counts as 0.

Selection (goodFeaturesToTrack, made deterministic); q = quality_level, md = min_distance and K = max_corners, q and md
as the C ABI's float32:
    M = max(S); M == 0: no features
    candidate: S > 0, f64(S) > f64(q) * f64(M), and S >= each of its (up to) 8 neighbours
    priority: S descending, then the raster index y*W + x ascending (a total order)
    greedy in priority order: accept unless an accepted point lies at dx*dx + dy*dy < md*md (integer dx, dy; float64);
    stop after K acceptances
    output: count; xy [K][2] float32 (x, y) in acceptance order; score [K]; rows from count on (NaN, NaN), score 0.
oflk_corner_score and oflk_good_features must equal this byte for byte (NaN bit patterns aside).
"""
from __future__ import annotations

import math

import numpy as np
from scipy import signal

SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.float32) / 8.0
SOBEL_Y = np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], dtype=np.float32) / 8.0
WINDOWS = (3, 5, 7, 9, 11)


def gradients(f):
    """(Ix, Iy) of the reference's compute_gradients(f, f), float32"""
    f = np.asarray(f).astype(np.float32)
    avg = (f + f) / 2.0
    Ix = signal.convolve2d(avg, SOBEL_X, mode="same", boundary="symm")
    Iy = signal.convolve2d(avg, SOBEL_Y, mode="same", boundary="symm")
    assert Ix.dtype == Iy.dtype == np.float32
    return Ix, Iy


def _box(P, h):
    """the separable float32 window sums of P at the interior pixels: (H-2h, W-2h), rows left to right, then columns top
    to bottom"""
    H, W = P.shape
    w = 2 * h + 1
    R = P[:, 0:W - 2 * h].copy()
    for k in range(1, w):
        R = R + P[:, k:k + W - 2 * h]
    A = R[0:H - 2 * h].copy()
    for k in range(1, w):
        A = A + R[k:k + H - 2 * h]
    assert A.dtype == np.float32
    return A


def tensor(f, window_size=5):
    """(a, b, c) float32 at the interior pixels (H-2h, W-2h), or None if the frame has none"""
    h = window_size // 2
    Ix, Iy = gradients(f)
    H, W = Ix.shape
    if H < 2 * h + 1 or W < 2 * h + 1:
        return None
    return _box(Ix * Ix, h), _box(Ix * Iy, h), _box(Iy * Iy, h)


def min_eig64(a, b, c):
    """the float64 form of the statement (before the float32 rounding); 0 where det <= 0"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        det = a * c - b * b
        tr = a + c
        d = a - c
        disc = np.sqrt(d * d + 4.0 * b * b)
        s = (2.0 * det) / (tr + disc)
    return np.where(det > 0, s, 0.0)


def score(f, window_size=5):
    """S (H, W) float32"""
    assert window_size in WINDOWS
    f = np.asarray(f)
    H, W = f.shape
    h = window_size // 2
    S = np.zeros((H, W), np.float32)
    t = tensor(f, window_size)
    if t is None:
        return S
    with np.errstate(over="ignore", invalid="ignore"):
        s = min_eig64(*t).astype(np.float32)
    s[~np.isfinite(s)] = 0
    S[h:H - h, h:W - h] = s
    return S


def candidates(S, quality_level):
    """(ys, xs) of the candidates in priority order, and M"""
    S = np.asarray(S, np.float32)
    H, W = S.shape
    M = S.max() if S.size else np.float32(0)
    if not M > 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), M
    pad = np.full((H + 2, W + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = S
    ok = (S > 0) & (S.astype(np.float64) > float(np.float32(quality_level)) * float(M))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                ok &= S >= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ys, xs = np.nonzero(ok)
    order = np.lexsort((ys * W + xs, -S[ys, xs]))
    return ys[order], xs[order], M


def select(S, quality_level=0.01, min_distance=10.0, max_corners=100):
    """(count, xy (K, 2) float32, score (K,) float32): the plain sequential greedy over a grid of cells of side
    max(1, ceil(md))"""
    S = np.asarray(S, np.float32)
    K = int(max_corners)
    xy = np.full((K, 2), np.nan, np.float32)
    sc = np.zeros(K, np.float32)
    ys, xs, _ = candidates(S, quality_level)
    md = float(np.float32(min_distance))
    md2 = md * md
    c = max(1, math.ceil(md)) if md < 1e9 else 1 << 30
    grid = {}
    n = 0
    for y, x in zip(ys.tolist(), xs.tolist()):
        if n == K:
            break
        cy, cx = y // c, x // c
        near = False
        for gy in (cy - 1, cy, cy + 1):
            for gx in (cx - 1, cx, cx + 1):
                for (py, px) in grid.get((gy, gx), ()):
                    if float((px - x) * (px - x) + (py - y) * (py - y)) < md2:
                        near = True
        if near:
            continue
        grid.setdefault((cy, cx), []).append((y, x))
        xy[n] = (x, y)
        sc[n] = S[y, x]
        n += 1
    return n, xy, sc


def good_features(f, window_size=5, quality_level=0.01, min_distance=10.0, max_corners=100):
    return select(score(f, window_size), quality_level, min_distance, max_corners)
