"""The online sparse KLT tracker's statement in NumPy (test infrastructure; the product never imports this module).

It states no arithmetic of its own: a step is sparse_model.track's (one pair, continued from the slots' row), the residual
is sparse_model.step's, a detection is replenish_model.detect on feature_model.score of the frame -- the pieces
sparse_replenish_model.sequence is built from, composed for frames that arrive one at a time.

K = max_corners slots, each holding at most one live track; every slot starts dead.  D = detect_every >= 0.  Push of frame t:

    step (t > 0):   every alive slot takes the step of pair t-1 of the sparse-replenish statement; residual[n] as there
    detect (D > 0 and t % D == 0):
                    that statement's detection on frame t with the rows after the step -- now, not when the next frame
                    arrives: the tracker knows no last frame, so the sequence statement's t < T-1 falls away
    row t:          xy[n] = the position or (NaN, NaN); visible[n]; born[n] = 1 where a track began in slot n on this frame;
                    birth[n] = the frame on which the slot's current track began (defined where visible[n]); residual[n],
                    all NaN on frame 0; detected = the points accepted on this frame

add_points after the push of frame t: points that are not finite or lie outside [0, W-1] x [0, H-1] are dropped; the i-th
remaining point goes to the i-th dead slot, ascending, while dead slots last: position (x + 0, y + 0), visible, born = 1,
birth = t.  From the next push on it is an ordinary track.
"""
from __future__ import annotations

import numpy as np

import feature_model
import replenish_model
import sparse_model

F32 = np.float32
NAMES = ("xy", "visible", "born", "birth", "residual", "detected")


class Tracker:
    def __init__(self, K, detect_every, quality_level=0.01, min_distance=10.0, num_levels=3, window_size=5, num_iterations=3,
                 alpha=0.01, beta=0.5, max_residual=4.0):
        assert int(detect_every) >= 0
        self.K, self.D = int(K), int(detect_every)
        self.q, self.md = quality_level, min_distance
        self.L, self.w, self.it = num_levels, window_size, num_iterations
        self.alpha, self.beta, self.mr = alpha, beta, max_residual
        self.reset()

    def reset(self):
        K = self.K
        self.t = -1
        self.xy, self.alive = np.full((K, 2), np.nan, F32), np.zeros(K, bool)
        self.born, self.birth = np.zeros(K, np.uint8), np.full(K, -1, np.int32)
        self.residual, self.detected = np.full(K, np.nan, F32), 0
        self.frame = self.pyr = None

    def row(self):
        """(xy (K, 2) float32, visible (K,) uint8, born (K,) uint8, birth (K,) int32, residual (K,) float32, detected)"""
        xy = np.full((self.K, 2), np.nan, F32)
        xy[self.alive] = self.xy[self.alive]
        return xy, self.alive.astype(np.uint8), self.born.copy(), self.birth.copy(), self.residual.copy(), int(self.detected)

    def push(self, frame, pyramid=None):
        """the next frame (uint8 frames are their float32 values); pyramid: sparse_model.pyramid of it, if the caller has it"""
        raw = np.asarray(frame)
        f32 = raw.astype(F32)
        K = self.K
        sparse_model.check_config(f32.shape, self.L, self.w, self.it)
        pyr = pyramid if pyramid is not None else sparse_model.pyramid(f32, self.L)
        t = self.t + 1
        self.born = np.zeros(K, np.uint8)
        self.residual = np.full(K, np.nan, F32)
        self.detected = 0
        if t > 0:
            i = np.flatnonzero(self.alive)
            _, _, _, ok, res = sparse_model.step(self.pyr, pyr, self.xy[i, 0], self.xy[i, 1], self.w, self.it)
            self.residual[i[ok]] = res[ok]
            tr, vis = sparse_model.track(np.stack([self.frame, f32]), np.full(K, -1, np.int64), np.zeros((K, 2), F32), self.L, self.w,
                                         self.it, self.alpha, self.beta, self.mr, t0=t - 1, prev=(self.xy, self.alive),
                                         pyramids=[self.pyr, pyr])
            self.xy, self.alive = tr[1], vis[1].astype(bool)
        if self.D > 0 and t % self.D == 0:
            slots, pts = replenish_model.detect(feature_model.score(raw, self.w), self.xy, self.alive, self.q, self.md)
            self.xy = self.xy.copy()
            self.xy[slots] = pts
            self.alive[slots] = True
            self.born[slots] = 1
            self.birth[slots] = t
            self.detected = len(slots)
        self.t, self.frame, self.pyr = t, f32, pyr
        return self.row()

    def add_points(self, pts):
        """returns the slots that took a point, in the points' order"""
        assert self.t >= 0, "no frame has been pushed"
        pts = np.asarray(pts, F32).reshape(-1, 2)
        H, W = self.frame.shape
        pts = pts[sparse_model._inside(pts[:, 0], pts[:, 1], H, W)]   # NaN and infinities compare as outside
        free = np.flatnonzero(~self.alive)
        n = min(len(free), len(pts))
        slots = free[:n]
        self.xy = self.xy.copy()
        self.xy[slots] = pts[:n] + F32(0)
        self.alive[slots] = True
        self.born[slots] = 1
        self.birth[slots] = self.t
        return slots


def pushes(frames, K, detect_every, pyramids=None, **kw):
    """the rows of pushing `frames` one by one, stacked in sparse_replenish_model's order -- tracks (T, K, 2), visible, born
    (T, K), detected (T,) int32, residual (T, K) -- and birth (T, K) int32"""
    tr = Tracker(K, detect_every, **kw)
    rows = [tr.push(f, None if pyramids is None else pyramids[i]) for i, f in enumerate(frames)]
    xy, vis, born, birth, res, det = (np.stack([r[j] for r in rows]) for j in range(6))
    return (xy, vis, born, det.astype(np.int32), res), birth


def check_birth(visible, born, birth):
    """birth, where visible, is the frame of the slot's last born mark at or before that row"""
    last = np.full(visible.shape[1], -1, np.int64)
    for t in range(visible.shape[0]):
        last[born[t] != 0] = t
        v = visible[t] != 0
        assert (last[v] >= 0).all() and np.array_equal(birth[t][v], last[v]), f"birth on row {t}"
