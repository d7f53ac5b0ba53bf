"""The replenished-KLT statement in NumPy (test infrastructure; the product never imports this module).

K slots, each holding at most one live track at a time.  State per slot n: position (x, y) float32 and alive; every slot
starts dead.  detect_every = D >= 1.  For t = 0 .. T-1:

    step (t > 0):   every alive slot takes the step of pair t-1 of track_model (two samples of the forward flow, the
                    forward-backward test at the landing point, the position rounded to float32); a slot whose step
                    fails is dead from row t on
    detect (t % D == 0 and t < T-1):
                    free = the dead slots, ascending;  seeds = (rint(x_n), rint(y_n)) of the alive slots (float32
                    round-half-even, as integers; an alive position outside the frame, which the sequence never
                    produces, seeds nothing)
                    the candidates of frame t's score map are feature_model.candidates' (M over the whole, unmasked map),
                    in its priority order;  greedy in that order: accept unless a seed or an accepted point lies at
                    dx*dx + dy*dy < md*md (integers, float64, md as float32);  stop after len(free) acceptances
                    the i-th accepted point goes to slot free[i]: position (f32(x), f32(y)), alive, born[t][slot] = 1
                    detected[t] = the number of acceptances (0 on frames without detection)
    row t:          tracks[t][n] = (x, y) if alive else (NaN, NaN);  visible[t][n] = alive

oflk_replenish_features must equal `detect`, and oflk_pyramidal_sequence_klt_replenish must equal `sequence` on its own
flows and score maps, byte for byte (NaN bit patterns aside).
"""
from __future__ import annotations

import math

import numpy as np

import feature_model
import track_model


def seeds_of(xy, visible, H, W):
    """integer seeds (sx, sy) of the alive slots whose position lies in the frame"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    vis = np.asarray(visible).astype(bool)
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        ok = vis & (x >= 0) & (x <= np.float32(W - 1)) & (y >= 0) & (y <= np.float32(H - 1))
    sx, sy = np.rint(x[ok]), np.rint(y[ok])   # float32 round-half-even
    assert sx.dtype == np.float32
    return sx.astype(np.int64), sy.astype(np.int64)


def detect(S, xy, visible, quality_level=0.01, min_distance=10.0):
    """One detection on the score map S (H, W) with the slots' row (xy (K, 2), visible (K,)): (slots, points (n, 2)
    float32) -- the i-th accepted point (x, y) and the slot free[i] it goes to.  The greedy over a grid of cells of side
    max(1, ceil(md)), seeds and accepted points alike, as feature_model.select."""
    S = np.asarray(S, np.float32)
    H, W = S.shape
    free = np.flatnonzero(~np.asarray(visible).astype(bool))
    md = float(np.float32(min_distance))
    md2 = md * md
    c = max(1, math.ceil(md)) if md < 1e9 else 1 << 30
    grid = {}
    sx, sy = seeds_of(xy, visible, H, W)
    if md > 0:
        for x, y in zip(sx.tolist(), sy.tolist()):
            grid.setdefault((y // c, x // c), []).append((y, x))
    ys, xs, _ = feature_model.candidates(S, quality_level)
    pts = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        if len(pts) == len(free):
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
        pts.append((x, y))
    return free[:len(pts)], np.array(pts, np.float32).reshape(-1, 2)


def apply(slots, pts, t, qt, qxy):
    """the outputs of one detection as the entry points give them: (qt, qxy, born (K,) uint8, detected)"""
    qt, qxy = np.array(qt, np.int32, copy=True), np.array(qxy, np.float32, copy=True)
    born = np.zeros(len(qt), np.uint8)
    qt[slots] = t
    qxy[slots] = pts
    born[slots] = 1
    return qt, qxy, born, len(slots)


def sequence(scores, flows, K, detect_every, quality_level=0.01, min_distance=10.0, alpha=0.01, beta=0.5, state=None, t0=0,
             T=None):
    """The statement for frames t0 .. t0+B of a sequence of T frames (default: t0+B is its last frame): scores(t) -> S of
    frame t (asked for detection frames only), flows = (uf, vf, ub, vb) [B][H][W] of pairs t0 .. t0+B-1.  state = (row
    (K, 2), visible (K,)) of frame t0 from an earlier call (None: every slot dead).  Returns tracks (B+1, K, 2), visible,
    born (uint8), detected (B+1,) int32."""
    D, q, md = int(detect_every), quality_level, min_distance
    uf, vf, ub, vb = (np.asarray(a, np.float32) for a in flows)
    B = uf.shape[0]
    T = t0 + B + 1 if T is None else T   # the sequence's length: no detection on its last frame
    tracks = np.full((B + 1, K, 2), np.nan, np.float32)
    visible = np.zeros((B + 1, K), np.uint8)
    born = np.zeros((B + 1, K), np.uint8)
    detected = np.zeros(B + 1, np.int32)
    if state is None:
        xy, alive = np.full((K, 2), np.nan, np.float32), np.zeros(K, bool)
    else:
        xy, alive = np.array(state[0], np.float32, copy=True), np.asarray(state[1]).astype(bool).copy()
    for r in range(B + 1):
        t = t0 + r
        if r > 0:   # one step of track_model for the alive slots: a one-pair call continued from the row
            qt = np.full(K, -1, np.int64)
            tr, vis = track_model.track(uf[r - 1:r], vf[r - 1:r], ub[r - 1:r], vb[r - 1:r], qt, np.zeros((K, 2), np.float32),
                                        alpha, beta, t0=t - 1, prev=(xy, alive))
            xy, alive = tr[1], vis[1].astype(bool)
        if t % D == 0 and t < T - 1:
            slots, pts = detect(scores(t), xy, alive, q, md)
            xy = xy.copy()
            xy[slots] = pts
            alive[slots] = True
            born[r, slots] = 1
            detected[r] = len(slots)
        tracks[r, alive] = xy[alive]
        visible[r, alive] = 1
    return tracks, visible, born, detected


def sequence_in_two(scores, flows, K, D, cut, **kw):
    """`sequence` cut into two calls at frame `cut` (0 < cut < T-1): the first ends on row `cut` as if it were the last frame
    (no detection there), the second starts from that row and detects on it if it is a detection frame"""
    uf = np.asarray(flows[0])
    T = uf.shape[0] + 1
    q, md = kw.get("quality_level", 0.01), kw.get("min_distance", 10.0)
    a, b = kw.get("alpha", 0.01), kw.get("beta", 0.5)
    first = sequence(scores, tuple(f[:cut] for f in flows), K, D, q, md, a, b, None, 0, cut + 1)
    second = sequence(scores, tuple(f[cut:] for f in flows), K, D, q, md, a, b, (first[0][-1], first[1][-1]), cut, T)
    return tuple(np.concatenate([x[:-1], y]) for x, y in zip(first, second))
