"""The statement of the video mosaic (oflk_mosaic_chain, oflk_mosaic_canvas, oflk_mosaic_accumulate, oflk_mosaic_resolve and the
calls made of them) in NumPy.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_mosaic.hpp) are held to it byte for byte, a
NaN equal to a NaN.  Every operation is float64 unless stated and rounded on its own; nothing is contracted, there is no
transcendental, and nothing depends on how a call is cut.

1. The chain (`chain`).  model [T-1][9] float32 and counts [T-1][3] (or None) as oflk_tracks_homography writes them, an anchor
   frame a in [0, T-1], the frame size H, W and a finite positive float64 extent.
   step s        A_s = the nine coefficients as double;  B_s = adj(A_s) / adj(A_s)[2][2], the adjugate by
                 homography_model.adjugate and nine divisions (`step`).  Held: counts[s][2] == 0, a coefficient of A_s not
                 finite, adj[2][2] == 0 or a coefficient of B_s not finite; then A_s = B_s = I and held[s] = 1
   composition   C = X o Y (Y first): C[r][c] = (X[r][0] Y[0][c] + X[r][1] Y[1][c]) + X[r][2] Y[2][c], then all nine divided
                 by C[2][2] (`compose`)
   chains        P_t maps anchor coordinates to frame t's: P_a = I, P_t = A_{t-1} o P_{t-1} (t > a), P_t = B_t o P_{t+1} (t < a)
                 Q_t maps frame t's to the anchor's:       Q_a = I, Q_t = Q_{t-1} o B_{t-1} (t > a), Q_t = Q_{t+1} o A_t (t < a)
                 Q is a chain of its own, not an inversion of P
   box           the corners (0,0), (W-1,0), (W-1,H-1), (0,H-1) of frame t under Q_t by the warp's formula,
                 w = (q6 x + q7 y) + q8, X = ((q0 x + q1 y) + q2) / w, Y likewise;  box[t] = (xmin, ymin, xmax, ymax), each
                 min / max taken as min(min(c0, c1), min(c2, c3))
   dropped       a corner's w <= 0, anything in P_t, Q_t, the corners' w, X or Y not finite, or |X| or |Y| > extent.  A frame
                 beyond a dropped one (further from the anchor on that side) is dropped too.  The anchor is never dropped.
                 box of a dropped frame: four NaNs.  from_anchor and to_anchor of a dropped frame hold what the chain
                 computed (it runs on through a dropped frame), whatever that is
   outputs       from_anchor [T][9] = P, to_anchor [T][9] = Q, box [T][4] float64;  held [T-1], dropped [T] bytes
2. The canvas (`canvas`), integers on the host: x0 = floor(min xmin), y0 = floor(min ymin) over the frames not dropped,
   Wc = ceil(max xmax) - x0 + 1, Hc likewise.
3. Accumulation (`accumulate`).  Per canvas pixel a float64 sum, a float64 wsum and an int32 count, all zero on an empty
   canvas.  Canvas pixel (x, y) has fx = f64(x0 + x), fy = f64(y0 + y), the sums formed in integers.  For f = 0 .. F-1
   ascending with skip[f] == 0, m = map[f]:
       w = (m6 fx + m7 fy) + m8;  xs = ((m0 fx + m1 fy) + m2) / w;  ys = ((m3 fx + m4 fy) + m5) / w
       inside = w > 0 and 0 <= xs <= W-1 and 0 <= ys <= H-1 (a NaN anywhere: outside)
   -- oflk_warp_perspective's, with (fx, fy) for the pixel indices.  Where inside, s = the float32 bilinear sample of frame f
   at (xs, ys) (track_model.sample), and
       mean      sum += f64(s);  wsum += 1
       feather   g = min(min(xs, (W-1) - xs), min(ys, (H-1) - ys)) + 1;  sum += g f64(s) (the product rounded, then the sum);
                 wsum += g
       first     only when count == 0: sum = f64(s), wsum = 1
       last      sum = f64(s), wsum = 1
   and count += 1 in every mode.  Samples are added one by one in frame order, so a canvas accumulated in several calls holds
   what one call gives.
4. Resolve (`resolve`): where count > 0, v = f32(sum / wsum); float32 output: v; uint8 output (`saturate`): 0 if v is a NaN,
   otherwise min(max(rint(v), 0), 255), rint half to even -- -0.5 gives 0, 254.5 gives 254, 255.5 gives 255, +-inf give 255
   and 0.  Elsewhere 0.  The state is not changed.  v leaves [0, 255] under an exposure (mosaic_exposure_model) and when a
   state accumulated from float32 frames is resolved to bytes; inside [0, 255] the rule is rint alone.
"""
import numpy as np

import homography_model as HM
from homography_model import adjugate
from track_model import sample as bilinear

MEAN, FEATHER, FIRST, LAST = 0, 1, 2, 3
BLENDS = {"mean": MEAN, "feather": FEATHER, "first": FIRST, "last": LAST}
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])


def step(model, counts, s):
    """(A_s, B_s, held): (9,) float64 each"""
    a = np.asarray(model[s], np.float32).astype(np.float64).reshape(9)
    with np.errstate(all="ignore"):
        adj = [np.float64(v) for v in adjugate(list(a))]
        b = np.array([v / adj[8] for v in adj], np.float64)
    ok = counts is None or counts[s][2] != 0
    ok = ok and np.isfinite(a).all() and adj[8] != 0.0 and np.isfinite(b).all()
    if not ok:
        return IDENTITY.copy(), IDENTITY.copy(), True
    return a, b, False


def compose(x, y):
    """X o Y, Y first, normalised by its last entry"""
    with np.errstate(all="ignore"):
        c = [(x[3 * r] * y[k] + x[3 * r + 1] * y[3 + k]) + x[3 * r + 2] * y[6 + k] for r in range(3) for k in range(3)]
        return np.array([v / c[8] for v in c], np.float64)


def corners(q, H, W):
    """the four corners of a frame under q: (X (4,), Y (4,), w (4,))"""
    cx = np.array([0.0, W - 1.0, W - 1.0, 0.0])
    cy = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    with np.errstate(all="ignore"):
        w = (q[6] * cx + q[7] * cy) + q[8]
        return ((q[0] * cx + q[1] * cy) + q[2]) / w, ((q[3] * cx + q[4] * cy) + q[5]) / w, w


def chain(model, counts, T, anchor, H, W, extent):
    """-> (from_anchor (T, 9), to_anchor (T, 9), box (T, 4) float64, held (T-1,), dropped (T,) uint8)"""
    assert T >= 1 and 0 <= anchor < T and H >= 2 and W >= 2 and np.isfinite(extent) and extent > 0
    P, Q = np.zeros((T, 9)), np.zeros((T, 9))
    box = np.full((T, 4), np.nan)
    held, dropped = np.zeros(max(T - 1, 0), np.uint8), np.zeros(T, np.uint8)
    steps = [step(model, counts, s) for s in range(T - 1)]
    for s in range(T - 1):
        held[s] = steps[s][2]
    P[anchor], Q[anchor] = IDENTITY, IDENTITY

    def finish(t, gone):
        X, Y, w = corners(Q[t], H, W)
        with np.errstate(invalid="ignore"):
            bad = bool((w <= 0).any()) or not (np.isfinite(P[t]).all() and np.isfinite(Q[t]).all() and np.isfinite(w).all()
                                               and np.isfinite(X).all() and np.isfinite(Y).all())
            bad = bad or bool((np.abs(X) > extent).any() or (np.abs(Y) > extent).any())
        gone = (gone or bad) and t != anchor
        dropped[t] = gone
        if not gone:
            box[t] = (min(min(X[0], X[1]), min(X[2], X[3])), min(min(Y[0], Y[1]), min(Y[2], Y[3])),
                      max(max(X[0], X[1]), max(X[2], X[3])), max(max(Y[0], Y[1]), max(Y[2], Y[3])))
        return gone

    finish(anchor, False)
    gone = False
    for t in range(anchor + 1, T):
        P[t] = compose(steps[t - 1][0], P[t - 1])
        Q[t] = compose(Q[t - 1], steps[t - 1][1])
        gone = finish(t, gone)
    gone = False
    for t in range(anchor - 1, -1, -1):
        P[t] = compose(steps[t][1], P[t + 1])
        Q[t] = compose(Q[t + 1], steps[t][0])
        gone = finish(t, gone)
    return P, Q, box, held, dropped


def canvas(box, dropped):
    """-> (x0, y0, Wc, Hc), Python integers"""
    keep = np.asarray(dropped) == 0
    b = np.asarray(box, np.float64)[keep]
    x0, y0 = int(np.floor(b[:, 0].min())), int(np.floor(b[:, 1].min()))
    return x0, y0, int(np.ceil(b[:, 2].max())) - x0 + 1, int(np.ceil(b[:, 3].max())) - y0 + 1


def empty_state(Hc, Wc):
    return {"sum": np.zeros((Hc, Wc)), "wsum": np.zeros((Hc, Wc)), "count": np.zeros((Hc, Wc), np.int32)}


def coordinates(m, x0, y0, Hc, Wc):
    """(xs, ys, w) of every canvas pixel under one map"""
    m = np.asarray(m, np.float64).reshape(9)
    fx = (np.int64(x0) + np.arange(Wc, dtype=np.int64)).astype(np.float64)[None, :]
    fy = (np.int64(y0) + np.arange(Hc, dtype=np.int64)).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        w = (m[6] * fx + m[7] * fy) + m[8]
        return ((m[0] * fx + m[1] * fy) + m[2]) / w, ((m[3] * fx + m[4] * fy) + m[5]) / w, w


def accumulate(state, frames, maps, skip, x0, y0, blend):
    """adds the F frames to the state, in place; returns it"""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    maps = np.asarray(maps, np.float64).reshape(F, 9)
    S, Ws, C = state["sum"], state["wsum"], state["count"]
    Hc, Wc = S.shape
    for f in range(F):
        if skip is not None and skip[f]:
            continue
        xs, ys, w = coordinates(maps[f], x0, y0, Hc, Wc)
        with np.errstate(invalid="ignore"):
            ins = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        if not ins.any():
            continue
        s = bilinear(frames[f].astype(np.float32), xs[ins], ys[ins]).astype(np.float64)
        if blend == MEAN:
            S[ins] = S[ins] + s
            Ws[ins] = Ws[ins] + 1.0
        elif blend == FEATHER:
            g = np.minimum(np.minimum(xs[ins], (W - 1.0) - xs[ins]), np.minimum(ys[ins], (H - 1.0) - ys[ins])) + 1.0
            S[ins] = S[ins] + g * s
            Ws[ins] = Ws[ins] + g
        elif blend == FIRST:
            new = C[ins] == 0
            S[ins] = np.where(new, s, S[ins])
            Ws[ins] = np.where(new, 1.0, Ws[ins])
        elif blend == LAST:
            S[ins] = s
            Ws[ins] = 1.0
        else:
            raise ValueError(blend)
        C[ins] = C[ins] + 1
    return state


def saturate(v):
    """the resolve's uint8 conversion of float32 values: 0 for a NaN, otherwise rint (half to even) held to [0, 255].  The NaN
    is replaced and the value clipped before the cast, so the cast never leaves uint8's domain and nothing here warns"""
    v = np.asarray(v, np.float32)
    r = np.rint(np.where(np.isnan(v), np.float32(0), v))
    return np.minimum(np.maximum(r, np.float32(0)), np.float32(255)).astype(np.uint8)


def resolve(state, u8):
    """-> (out (Hc, Wc) float32 or uint8, count (Hc, Wc) int32)"""
    some = state["count"] > 0
    with np.errstate(all="ignore"):   # the division and its rounding to float32 only: inf / inf, an overflow
        v = np.where(some, (state["sum"] / np.where(some, state["wsum"], 1.0)).astype(np.float32), np.float32(0))
    return (saturate(v) if u8 else v.astype(np.float32)), state["count"].copy()


def composite(frames, maps, skip, x0, y0, Hc, Wc, blend, cuts=()):
    """accumulate (cut into calls at the frame indices `cuts`) and resolve: (out, count)"""
    frames = np.asarray(frames)
    F = frames.shape[0]
    maps = np.asarray(maps, np.float64).reshape(F, 9)
    st = empty_state(Hc, Wc)
    edges = [0, *cuts, F]
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi > lo:
            accumulate(st, frames[lo:hi], maps[lo:hi], None if skip is None else skip[lo:hi], x0, y0, blend)
    return resolve(st, frames.dtype == np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def translation(dx, dy):
    """the model that maps (x, y) to (x + dx, y + dy): (9,) float64"""
    return np.array([1.0, 0.0, dx, 0.0, 1.0, dy, 0.0, 0.0, 1.0])


def planted_steps(S, seed=0, scale=1.0):
    """S step models near the identity: a small rotation, zoom, shift and projective row each, float32 (S, 9) with h22 == 1"""
    rng = np.random.default_rng(seed)
    out = np.zeros((S, 9), np.float32)
    for s in range(S):
        a = rng.uniform(-0.01, 0.01) * scale
        z = 1.0 + rng.uniform(-0.01, 0.01) * scale
        out[s] = [z * np.cos(a), -z * np.sin(a), rng.uniform(-6, 6) * scale, z * np.sin(a), z * np.cos(a),
                  rng.uniform(-4, 4) * scale, rng.uniform(-2e-5, 2e-5) * scale, rng.uniform(-2e-5, 2e-5) * scale, 1.0]
    return out


def pan_frames(image, F, H, W, dx, dy=0, x_start=0, y_start=0):
    """F frames of H x W cut from `image` at integer offsets (x_start + f dx, y_start + f dy); the maps from the image's
    coordinates to each frame's (translations): (frames, maps (F, 9))"""
    frames = np.stack([image[y_start + f * dy:y_start + f * dy + H, x_start + f * dx:x_start + f * dx + W] for f in range(F)])
    maps = np.stack([translation(-(x_start + f * dx), -(y_start + f * dy)) for f in range(F)])
    return np.ascontiguousarray(frames), maps


def smooth_field(H, W, seed, octaves=((1.5, 1.0), (4.0, 0.6))):
    """a seeded textured uint8 image: white noise blurred at two scales with a separable box filter run three times, stretched to
    the full byte range.  No transcendental, the same bytes everywhere"""
    rng = np.random.default_rng(seed)
    acc = np.zeros((H, W))
    for radius, weight in octaves:
        n = rng.random((H, W))
        r = int(round(radius))
        k = np.ones(2 * r + 1) / (2 * r + 1)
        for _ in range(3):
            n = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="wrap"), k, mode="valid"), 0, n)
            n = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="wrap"), k, mode="valid"), 1, n)
        n = (n - n.min()) / (n.max() - n.min())
        acc += weight * n
    acc = (acc - acc.min()) / (acc.max() - acc.min())
    return np.rint(acc * 255.0).astype(np.uint8)


planted_homography = HM.planted_homography
