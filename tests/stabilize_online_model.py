"""The statement of online video stabilisation (oflk_stabilize_trajectory_ring, oflk_stabilizer_*) in NumPy: the ring of step
models and the schedule of a fixed-lag stabiliser.

Test infrastructure: the product never imports this file.  k_stab_online (csrc/oflk_stabilize.hpp) is held to it byte for byte.

It is stabilize_model's trajectory, read in the order in which a stream delivers its steps.  The window of frame f is
r_f = min(r, f, T-1-f) and reads steps f - r_f .. f + r_f - 1, so frame f is final once frame f + r has been pushed (while the
stream is open, r_f = min(r, f)), and the last r frames are final once the stream has ended and T is known.

Ring: step s lives at slot s % cap, cap >= max(2 r, 1): model (cap, 6) float32 and counts (cap, 3) int32.  The window of a frame
that may be asked for spans at most 2 r consecutive steps, so no slot it reads has been overwritten.  Nothing but ring
contents is read: the slots start as garbage (a shift of (100, -50) with status 1, which would move every frame that read
it) and stay so until written.

Schedule: the push of frame t writes step t-1 (t >= 1) into slot (t-1) % cap and, for t >= r, emits frame t - r with the
open-stream window; the flush emits frames T - min(r, T) .. T-1, ascending, with the true T = the frames pushed.
"""
import numpy as np

import stabilize_model as SM


def frame(ring_model, ring_counts, cap, f, T, w):
    """(correction (6,) float32, map (6,) float64) of frame f from the ring; T < 0: the stream is open"""
    w = np.asarray(w, np.float64)
    r = len(w) - 1
    assert cap >= max(2 * r, 1) and f >= 0 and (T < 0 or f < T)
    rf = min(r, f) if T < 0 else min(r, f, T - 1 - f)
    slots = [s % cap for s in range(f - rf, f + rf)]          # steps f - rf .. f + rf - 1: window position j holds step f - rf + j
    model = np.asarray(ring_model, np.float32).reshape(cap, 6)[slots]
    counts = None if ring_counts is None else np.asarray(ring_counts).reshape(cap, 3)[slots]
    A, B, _ = SM.steps(model, counts)
    acc, ws = w[0] * SM.IDENTITY, w[0]
    F, G = SM.IDENTITY.copy(), SM.IDENTITY.copy()
    with np.errstate(all="ignore"):
        for i in range(1, rf + 1):
            F = SM.compose(A[rf + i - 1], F)                  # step f + i - 1
            acc = acc + w[i] * F
            ws = ws + w[i]
            G = SM.compose(B[rf - i], G)                      # step f - i
            acc = acc + w[i] * G
            ws = ws + w[i]
        c = (acc / ws).astype(np.float32)
    m, ok = SM.invert(c.astype(np.float64))
    if not (ok and np.isfinite(c).all()):
        c, m = SM.IDENTITY.astype(np.float32), SM.IDENTITY.copy()
    return c, m


def trajectory_ring(ring_model, ring_counts, cap, f0, n, T, w):
    """oflk_stabilize_trajectory_ring: (correction (n, 6) float32, map (n, 6) float64) of frames f0 .. f0 + n - 1"""
    assert n >= 1 and (T >= 0 or n == 1) and (T < 0 or f0 + n <= T)
    rows = [frame(ring_model, ring_counts, cap, f0 + i, T, w) for i in range(n)]
    return np.stack([c for c, _ in rows]), np.stack([m for _, m in rows])


def fill_ring(model, counts, cap, upto):
    """the ring after steps 0 .. upto-1 of `model` / `counts` were written in order: (ring_model, ring_counts)"""
    ring_model, ring_counts = np.tile(np.float32([1, 0, 100, 0, 1, -50]), (cap, 1)), np.ones((cap, 3), np.int32)
    for s in range(upto):
        ring_model[s % cap] = model[s]
        if counts is not None:
            ring_counts[s % cap] = counts[s]
    return ring_model, ring_counts


class Stream:
    """the stabiliser's schedule on step models: push(model, counts) per frame, flush() at the end"""

    def __init__(self, w, cap=None):
        self.w = np.asarray(w, np.float64)
        self.r = len(self.w) - 1
        self.cap = max(2 * self.r, 1) if cap is None else cap
        assert self.cap >= max(2 * self.r, 1)
        self.model, self.counts = fill_ring(None, None, self.cap, 0)
        self.t = -1
        self.flushed = False

    def push(self, model=None, counts=None):
        """frame t arrives with the model and counts of step t-1 (ignored for t = 0): None, or (index, correction, map)"""
        assert not self.flushed
        self.t += 1
        if self.t >= 1:
            self.model[(self.t - 1) % self.cap] = model
            self.counts[(self.t - 1) % self.cap] = counts
        if self.t < self.r:
            return None
        return (self.t - self.r,) + frame(self.model, self.counts, self.cap, self.t - self.r, -1, self.w)

    def flush(self):
        """[(index, correction, map)] of the frames not yet emitted, ascending"""
        T = self.t + 1
        n = 0 if self.flushed else min(self.r, T)
        self.flushed = True
        return [(f,) + frame(self.model, self.counts, self.cap, f, T, self.w) for f in range(T - n, T)]


def run(model, counts, T, w, cap=None):
    """T pushes and a flush: (indices in emission order, correction (T, 6) float32, map (T, 6) float64)"""
    st = Stream(w, cap)
    got = []
    for t in range(T):
        e = st.push(None if t == 0 else model[t - 1], None if t == 0 else counts[t - 1])
        if e is not None:
            got.append(e)
    got += st.flush()
    return ([e[0] for e in got], np.stack([e[1] for e in got]) if got else np.zeros((0, 6), np.float32),
            np.stack([e[2] for e in got]) if got else np.zeros((0, 6), np.float64))
