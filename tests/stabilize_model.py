"""The statement of video stabilisation (oflk_stabilize_trajectory, oflk_warp_affine, oflk_stabilize_sequence) in NumPy.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_stabilize.hpp) are held to it byte for byte.

Every operation is float64 unless stated, rounded on its own, in the order written here.

Trajectory: one correction per frame from the T-1 step models.
    inputs        model (T-1, 6) float32 [a00 a01 tx; a10 a11 ty], step s mapping frame s to frame s+1 (motion_model.tracks);
                  counts (T-1, 3) or None; weights[0 .. r] float64, finite and positive, given by the caller; T >= 1
    inverse       det = a00*a11 - a01*a10; i00 = a11/det, i01 = -a01/det, i10 = -a10/det, i11 = a00/det;
                  itx = -(i00*tx + i01*ty), ity = -(i10*tx + i11*ty)                                          (`invert`)
    step s        A_s = the coefficients as double, B_s = its inverse.  Held when counts[s][2] == 0, a coefficient is not
                  finite, det == 0 or a coefficient of B_s is not finite: A_s = B_s = identity, held[s] = 1       (`steps`)
    composition   C = A o F (F first): c00 = A00*F00 + A01*F10, c01 = A00*F01 + A01*F11, ctx = (A00*Ftx + A01*Fty) + Atx,
                  the second row likewise                                                                     (`compose`)
    frame t       r_t = min(r, t, T-1-t).  acc = weights[0] * I (six products), ws = weights[0], F = G = I; for i = 1 .. r_t:
                  F = A_{t+i-1} o F; acc += weights[i] * F; ws += weights[i]; G = B_{t-i} o G; acc += weights[i] * G;
                  ws += weights[i].  correction[t] = f32(acc / ws); map[t] = invert(f64(correction[t])).  det == 0 or
                  anything not finite: both are the identity.
The stated inverse of the identity has -0.0 where -a01/det, -a10/det and the negated translations are formed: map[t] of an
unmoved frame equals the identity as values (-0.0 == 0.0), correction[t] bit for bit.

Warp: out[f][y][x] = sample(frame f, xs, ys), xs = (m0*f64(x) + m1*f64(y)) + m2, ys = (m3*f64(x) + m4*f64(y)) + m5, m = map[f];
sample is track_model.sample (map_coordinates, order 1, cval 0, float32 result); inside = 0 <= xs <= W-1 and 0 <= ys <= H-1
(closed, float64), and the sample is 0 where not inside.  float32 frames give float32, uint8 frames (uint8) rint(sample).
"""
import numpy as np

from track_model import sample

MAX_RADIUS = 64
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def weights(radius, sigma=None):
    """the Gaussian window the Python shims form (the C ABI takes any finite positive weights)"""
    if sigma is None:
        sigma = radius / 2 if radius > 0 else 1.0
    return np.exp(-0.5 * (np.arange(radius + 1) / sigma) ** 2)


def invert(a):
    """(6,) float64 -> ((6,) float64, ok)"""
    with np.errstate(all="ignore"):
        a00, a01, tx, a10, a11, ty = (np.float64(v) for v in a)
        det = a00 * a11 - a01 * a10
        i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
        itx = -(i00 * tx + i01 * ty)
        ity = -(i10 * tx + i11 * ty)
        b = np.array([i00, i01, itx, i10, i11, ity], np.float64)
    return b, bool(det != 0.0 and np.isfinite(b).all())


def compose(a, f):
    """a o f: f first"""
    with np.errstate(all="ignore"):
        return np.array([a[0] * f[0] + a[1] * f[3], a[0] * f[1] + a[1] * f[4], (a[0] * f[2] + a[1] * f[5]) + a[2],
                         a[3] * f[0] + a[4] * f[3], a[3] * f[1] + a[4] * f[4], (a[3] * f[2] + a[4] * f[5]) + a[5]], np.float64)


def steps(model, counts=None):
    """(A (S, 6), B (S, 6) float64, held (S,) uint8)"""
    model = np.asarray(model, np.float32).reshape(-1, 6)
    S = len(model)
    A, B, held = np.tile(IDENTITY, (S, 1)), np.tile(IDENTITY, (S, 1)), np.zeros(S, np.uint8)
    for s in range(S):
        a = model[s].astype(np.float64)
        b, ok = invert(a)
        ok = ok and np.isfinite(a).all() and (counts is None or int(np.asarray(counts)[s][2]) != 0)
        if ok:
            A[s], B[s] = a, b
        else:
            held[s] = 1
    return A, B, held


def trajectory(model, counts, T, w):
    """(correction (T, 6) float32, map (T, 6) float64, held (T-1,) uint8); the radius is len(w) - 1"""
    w = np.asarray(w, np.float64)
    r = len(w) - 1
    assert T >= 1 and 0 <= r <= MAX_RADIUS and np.isfinite(w).all() and (w > 0).all()
    A, B, held = steps(np.zeros((0, 6), np.float32) if T == 1 else model, counts)
    assert len(A) == T - 1
    corr, mp = np.empty((T, 6), np.float32), np.empty((T, 6), np.float64)
    for t in range(T):
        rt = min(r, t, T - 1 - t)
        acc, ws = w[0] * IDENTITY, w[0]
        F, G = IDENTITY.copy(), IDENTITY.copy()
        with np.errstate(all="ignore"):
            for i in range(1, rt + 1):
                F = compose(A[t + i - 1], F)
                acc = acc + w[i] * F
                ws = ws + w[i]
                G = compose(B[t - i], G)
                acc = acc + w[i] * G
                ws = ws + w[i]
            c = (acc / ws).astype(np.float32)
        m, ok = invert(c.astype(np.float64))
        if not (ok and np.isfinite(c).all()):
            c, m = IDENTITY.astype(np.float32), IDENTITY.copy()
        corr[t], mp[t] = c, m
    return corr, mp, held


def coordinates(m, H, W):
    """the source position (xs, ys) of every output pixel under one map, (H, W) float64 each"""
    m = np.asarray(m, np.float64)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        return (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]


def warp(frames, maps):
    """frames (F, H, W) float32 or uint8, maps (F, 6) float64 -> (out like frames, inside (F, H, W) uint8)"""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    maps = np.asarray(maps, np.float64).reshape(F, 6)
    out, inside = np.zeros(frames.shape, frames.dtype), np.zeros(frames.shape, np.uint8)
    for f in range(F):
        xs, ys = coordinates(maps[f], H, W)
        with np.errstate(invalid="ignore"):
            ins = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        v = np.zeros((H, W), np.float32)
        v[ins] = sample(frames[f].astype(np.float32), xs[ins], ys[ins])
        out[f] = np.rint(v).astype(np.uint8) if frames.dtype == np.uint8 else v
        inside[f] = ins
    return out, inside


def sequence(frames, K, D, q, md, family, hyps, thr, seed, w, **kw):
    """the chain of statements: sparse_replenish_model.sequence, motion_model.tracks (t0 = 0), trajectory, warp.
    Returns (out, correction, model, counts, held)"""
    import motion_model as MM
    import sparse_replenish_model as RM

    frames = np.asarray(frames)
    tr, vis, born, _, _ = RM.sequence(frames, K, D, q, md, **kw)
    model, _, counts = MM.tracks(tr, vis, born, family, hyps, thr, seed, 0)
    corr, mp, held = trajectory(model, counts, len(frames), w)
    return warp(frames, mp)[0], corr, model, counts, held


def same(got, want, what=""):
    """byte for byte; a NaN equals a NaN"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.dtype}{g.shape} against {w.dtype}{w.shape}"
    if g.dtype.kind == "f":
        bits = np.uint32 if g.dtype == np.float32 else np.uint64
        eq = (g.view(bits) == w.view(bits)) | (np.isnan(g) & np.isnan(w))
    else:
        eq = g == w
    assert eq.all(), f"{what}: differs at {np.argwhere(~eq)[:5].tolist()}: got {g[~eq][:5]}, want {w[~eq][:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def noisy_models(S, family, seed):
    """S step models of a family around motion_model.planted_coefficients, per-step noise; float32 (S, 6)"""
    import motion_model as MM

    rng = np.random.default_rng(seed)
    c = np.tile(MM.planted_coefficients(), (S, 1))
    if family == MM.TRANSLATION:
        c[:, [0, 4]], c[:, [1, 3]] = 1.0, 0.0
    elif family == MM.SIMILARITY:
        a, b = c[:, 0] + rng.normal(0, 0.004, S), c[:, 3] + rng.normal(0, 0.004, S)
        c[:, 0], c[:, 1], c[:, 3], c[:, 4] = a, -b, b, a
    else:
        c[:, [0, 1, 3, 4]] += rng.normal(0, 0.004, (S, 4))
    c[:, [2, 5]] += rng.normal(0, 1.5, (S, 2))
    return c.astype(np.float32)


def jitter_scene(seed, T=14, H=64, W=80):
    """T uint8 frames cut from a Gaussian-smoothed (sigma 1.2) random texture, moved by a pan of 1 px per frame plus an
    integer jitter in [-2, 2] per axis.  Returns (frames, path (T, 2)): the content of frame t sits at path[t] (x, y)
    relative to frame 0, so step t's true model is the translation path[t + 1] - path[t]"""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    pad = T + 8
    tex = gaussian_filter(rng.random((H + 2 * pad, W + 2 * pad)), 1.2)
    tex = np.rint(255 * (tex - tex.min()) / (tex.max() - tex.min())).astype(np.uint8)
    path = np.stack([np.arange(T), np.zeros(T, np.int64)], -1) + rng.integers(-2, 3, (T, 2))
    path -= path[0]
    frames = np.stack([tex[pad - py:pad - py + H, pad - px:pad - px + W] for px, py in path])
    return frames, path
