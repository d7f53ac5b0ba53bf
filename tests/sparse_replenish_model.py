"""The replenished-KLT statement on the sparse tracker in NumPy (test infrastructure; the product never imports this module).

It states no arithmetic of its own: a step is sparse_model.track's (one pair, continued from the slots' row), the residual
is sparse_model.step's, a detection is replenish_model.detect on feature_model.score of the frame.

K = max_corners slots, each holding at most one live track; every slot starts dead.  D = detect_every >= 1.  The LK
window is the detection window (odd, 3 .. 11).  For t = 0 .. T-1:

    step (t > 0):   every alive slot takes the step of pair t-1 of the sparse-tracks statement: step forward, then step
                    backward from f32(q) if the forward step is ok; alive = ok and ok' and e2 <= alpha*m2 + beta and
                    r <= max_residual; the position becomes (f32(qx), f32(qy))
                    residual[t][n] = the forward step's r where that step was ok, for every slot alive on row t-1,
                    whether or not the track then survives
                    every other entry of residual is NaN: a slot dead on row t-1 (so a point born on row t in a slot that
                    was dead has NaN there), a forward step that was not ok, and all of row 0.  A slot whose track ends on
                    row t and which the detection of row t fills again keeps the ended track's residual on that row: the
                    step writes the row, the detection does not touch it
    detect (t % D == 0 and t < T-1):
                    replenish_model.detect on feature_model.score(frame t, window): the free slots ascending, the seeds
                    rint of the alive slots' positions after the step, the greedy stopped after len(free) acceptances;
                    the i-th accepted point goes to slot free[i]: position (f32 x, f32 y), alive, born[t][slot] = 1
                    detected[t] = the number accepted
    row t:          tracks[t][n] = (x, y) if alive else (NaN, NaN);  visible[t][n] = alive

With D >= T, tracks and visible are those of the detection on frame 0 followed by sparse_model.track.  Positions are float32
between steps and a call's last row is never a detection row of that call, so the result does not depend on how the
sequence is cut into calls.
"""
from __future__ import annotations

import numpy as np

import feature_model
import replenish_model
import sparse_model

F32 = np.float32
NAMES = ("tracks", "visible", "born", "detected", "residual")


def sequence(frames, K, detect_every, quality_level=0.01, min_distance=10.0, num_levels=3, window_size=5, num_iterations=3,
             alpha=0.01, beta=0.5, max_residual=4.0, state=None, t0=0, T=None, pyramids=None):
    """The statement for the B+1 frames given, which are frames t0 .. t0+B of a sequence of T frames (default: t0+B is its
    last frame).  state = (row (K, 2), visible (K,)) of frame t0 from an earlier call (None: every slot dead).  Returns
    tracks (B+1, K, 2), visible, born (uint8), detected (B+1,) int32, residual (B+1, K) float32; row 0 of residual is NaN
    (for t0 > 0 it belongs to the earlier call).  uint8 frames are their float32 values."""
    D = int(detect_every)
    raw = np.asarray(frames)
    f32 = raw.astype(F32)
    B = f32.shape[0] - 1
    sparse_model.check_config(f32.shape[1:], num_levels, window_size, num_iterations)
    T = t0 + B + 1 if T is None else T
    pyr = pyramids if pyramids is not None else [sparse_model.pyramid(f, num_levels) for f in f32]
    tracks = np.full((B + 1, K, 2), np.nan, F32)
    visible = np.zeros((B + 1, K), np.uint8)
    born = np.zeros((B + 1, K), np.uint8)
    detected = np.zeros(B + 1, np.int32)
    residual = np.full((B + 1, K), np.nan, F32)
    if state is None:
        xy, alive = np.full((K, 2), np.nan, F32), np.zeros(K, bool)
    else:
        xy, alive = np.array(state[0], F32, copy=True), np.asarray(state[1]).astype(bool).copy()
    before = np.full(K, -1, np.int64)   # every slot is a query of an earlier frame: the row is its state
    for r in range(B + 1):
        t = t0 + r
        if r > 0:
            i = np.flatnonzero(alive)
            _, _, _, ok, res = sparse_model.step(pyr[r - 1], pyr[r], xy[i, 0], xy[i, 1], window_size, num_iterations)
            residual[r, i[ok]] = res[ok]
            tr, vis = sparse_model.track(f32[r - 1:r + 1], before, np.zeros((K, 2), F32), num_levels, window_size, num_iterations,
                                         alpha, beta, max_residual, t0=t - 1, prev=(xy, alive), pyramids=pyr[r - 1:r + 1])
            xy, alive = tr[1], vis[1].astype(bool)
        if t % D == 0 and t < T - 1:
            slots, pts = replenish_model.detect(feature_model.score(raw[r], window_size), xy, alive, quality_level, min_distance)
            xy = xy.copy()
            xy[slots] = pts
            alive[slots] = True
            born[r, slots] = 1
            detected[r] = len(slots)
        tracks[r, alive] = xy[alive]
        visible[r, alive] = 1
    return tracks, visible, born, detected, residual


def join(first, second):
    """the outputs of two calls, the second continued from the first's last row, as those of one: the second's row 0
    replaces the first's last row, except in residual, whose row of that frame the first call wrote"""
    out = [np.concatenate([a[:-1], b]) for a, b in zip(first[:4], second[:4])]
    out.append(np.concatenate([first[4], second[4][1:]]))
    return tuple(out)


def sequence_in_two(frames, K, D, cut, pyramids=None, **kw):
    """`sequence` cut into two calls at frame `cut` (0 < cut < T-1): the first ends on row `cut` as if it were the last frame
    (no detection there), the second starts from that row and detects on it if it is a detection frame"""
    frames = np.asarray(frames)
    T = frames.shape[0]
    pa, pb = (None, None) if pyramids is None else (pyramids[:cut + 1], pyramids[cut:])
    first = sequence(frames[:cut + 1], K, D, state=None, t0=0, T=cut + 1, pyramids=pa, **kw)
    second = sequence(frames[cut:], K, D, state=(first[0][-1], first[1][-1]), t0=cut, T=T, pyramids=pb, **kw)
    return join(first, second)


def same(got, want, what=""):
    """byte for byte, NaN bit patterns normalised"""
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype == bool or w.dtype == bool:
            g, w = g.astype(np.uint8), w.astype(np.uint8)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == F32:
            g, w = g.copy(), w.copy()
            g[np.isnan(g)] = F32(np.nan)
            w[np.isnan(w)] = F32(np.nan)
        bad = np.flatnonzero(np.frombuffer(g.tobytes(), np.uint8) != np.frombuffer(w.tobytes(), np.uint8))
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} bytes, first at byte {bad[0]}"
