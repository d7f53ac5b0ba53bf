"""The point-track statement in NumPy (test infrastructure; the product never imports this module).

T frames, the forward flows F[t] = (uf[t], vf[t]) of pair t (frames t -> t+1) and the backward flows G[t] = (ub[t], vb[t])
(frames t+1 -> t).  Query n is (t_q, x_q, y_q): an int frame index and a float32 position, x along W.  sample(img, x, y)
is scipy.ndimage.map_coordinates(img, [[y], [x]], order=1, mode="constant", cval=0.0) at float64 coordinates with a float32
result (the reference's warp_image at one point).  Every float32 operation is rounded on its own, as fb_model.one_direction:

    rows t < t_q:                                           track = (NaN, NaN), visible = 0
    x_q, y_q not finite or outside [0, W-1] x [0, H-1]:     every row NaN / 0
    row t_q:                (x, y) = (x_q + 0, y_q + 0), visible = 1       (a query at -0 reads as +0)
    for t = t_q .. T-2:
        us = sample(uf[t], x, y);  vs = sample(vf[t], x, y)
        qx = f64(x) + f64(us);     qy = f64(y) + f64(vs)
        inside = 0 <= qx <= W-1 and 0 <= qy <= H-1                        (float64, closed)
        bu = sample(ub[t], qx, qy); bv = sample(vb[t], qx, qy)
        eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev
        m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
        ok = inside and e2 <= f32(alpha)*m2 + f32(beta)
        if not ok: rows t+1 .. T-1 = NaN / 0; stop
        (x, y) = (f32(qx), f32(qy)); row t+1 = (x, y), visible = 1        (round to nearest even)

Positions are carried as float32 between steps, so the last written row is the whole state of a track: `track` continues
from a row of an earlier call (t0 > 0), and a sequence cut into chunks gives the same tracks.  oflk_track_points must equal
this byte for byte (NaN bit patterns aside).
"""
from __future__ import annotations

import numpy as np
from scipy.ndimage import map_coordinates


def sample(img, x, y):
    """map_coordinates of the (H, W) float32 image at the float64 points (x, y) (1-D), as float32"""
    img = np.ascontiguousarray(img, np.float32)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.size == 0:
        return np.zeros(0, np.float32)
    out = map_coordinates(img, [y, x], order=1, mode="constant", cval=0.0)
    assert out.dtype == np.float32
    return out


def track(uf, vf, ub, vb, qt, qxy, alpha=0.01, beta=0.5, t0=0, prev=None):
    """(tracks (B+1, N, 2) float32, visible (B+1, N) uint8): rows of frames t0 .. t0+B for flows [B][H][W] of pairs
    t0 .. t0+B-1.  prev = (row (N, 2), visible (N,)) of frame t0 from an earlier call, read for queries with qt < t0 (the
    device form's row 0); qt None: every query at frame 0."""
    uf, vf, ub, vb = (np.asarray(a, np.float32) for a in (uf, vf, ub, vb))
    B, H, W = uf.shape
    qxy = np.asarray(qxy, np.float32).reshape(-1, 2)
    N = qxy.shape[0]
    qt = np.zeros(N, np.int64) if qt is None else np.asarray(qt, np.int64)
    tracks = np.full((B + 1, N, 2), np.nan, np.float32)
    visible = np.zeros((B + 1, N), np.uint8)
    alive = np.zeros(N, bool)
    x, y = np.zeros(N, np.float32), np.zeros(N, np.float32)
    qx, qy = qxy[:, 0], qxy[:, 1]
    with np.errstate(invalid="ignore"):
        q_in = (qx >= 0) & (qx <= np.float32(W - 1)) & (qy >= 0) & (qy <= np.float32(H - 1))
    a32, b32 = np.float32(alpha), np.float32(beta)
    before = qt < t0
    if before.any():
        assert prev is not None, "queries before t0 need the previous call's row"
        prow, pvis = np.asarray(prev[0], np.float32), np.asarray(prev[1]).astype(bool)
        alive[before] = pvis[before]
        x[before], y[before] = prow[before, 0], prow[before, 1]
    for r in range(B + 1):
        if r > 0:   # step of pair t0 + r - 1 for the points alive on row r - 1
            i = np.flatnonzero(alive)
            px, py = x[i], y[i]
            us, vs = sample(uf[r - 1], px, py), sample(vf[r - 1], px, py)
            fx = px.astype(np.float64) + us.astype(np.float64)
            fy = py.astype(np.float64) + vs.astype(np.float64)
            inside = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
            bu, bv = sample(ub[r - 1], fx, fy), sample(vb[r - 1], fx, fy)
            eu, ev = us + bu, vs + bv
            e2 = eu * eu + ev * ev
            m2 = (us * us + vs * vs) + (bu * bu + bv * bv)
            ok = inside & (e2 <= a32 * m2 + b32)
            assert e2.dtype == m2.dtype == np.float32
            alive[i] = ok
            x[i], y[i] = fx.astype(np.float32), fy.astype(np.float32)
        start = qt == t0 + r   # a query starts on its own row
        alive[start] = q_in[start]
        x[start], y[start] = qx[start] + np.float32(0), qy[start] + np.float32(0)
        tracks[r, alive, 0], tracks[r, alive, 1] = x[alive], y[alive]
        visible[r, alive] = 1
    return tracks, visible


def smooth_flows(B, H, W, seed, scale=3.0):
    """four smooth random flows (uf, vf, ub, vb) [B][H][W] of up to +-scale px, G close to -F so that most steps pass the
    test and some fail"""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)

    def field():
        f = np.stack([gaussian_filter(rng.standard_normal((H, W)), 2.0, mode="wrap") for _ in range(B)])
        return f / max(np.abs(f).max(), 1e-12)

    uf, vf = field() * scale, field() * scale
    ub = -uf + 0.3 * scale * field()
    vb = -vf + 0.3 * scale * field()
    return tuple(a.astype(np.float32) for a in (uf, vf, ub, vb))


# ---- the occluder scene (fb_model.occluder_scene) and what its tracks must show ----------------------------------------
SCENE = dict(H=96, W=128, size=36, step=(3, 1))


def scene_queries(corners, T, H, W, size, step):
    """query sets on the occluder scene, each (N, 3) (t, x, y) float32:
    square: frame-0 pixels at least 12 px inside the square; background: frame-0 pixels at least 8 px from every position
    of the square and from the frame's border; covered[t]: frame-t background pixels the square covers in frame t+1"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    y0, x0 = corners[0]
    m = 12
    sq = (yy >= y0 + m) & (yy < y0 + size - m) & (xx >= x0 + m) & (xx < x0 + size - m)
    bg = (xx >= 8) & (xx < W - 8) & (yy >= 8) & (yy < H - 8)
    for (cy, cx) in corners:
        bg &= ~((yy >= cy - 8) & (yy < cy + size + 8) & (xx >= cx - 8) & (xx < cx + size + 8))

    def at(mask, t):
        ys, xs = np.nonzero(mask)
        return np.stack([np.full(len(xs), t), xs, ys], 1).astype(np.float32)

    import fb_model

    covered = [at(fb_model.scene_regions(corners, t, H, W, size, step, 6)[0], t) for t in range(T - 1)]
    return at(sq, 0), at(bg, 0), covered


def check_scene_tracks(run, T, corners, H, W, size, step):
    """the meaning of tracks on the occluder scene; run(queries) -> (tracks (T, N, 2), visible (T, N) bool).  The bounds
    come from this statement on the CPU oracle's flows of fb_model.occluder_scene(5) (3/5/3, alpha 0.01, beta 0.5), where
    the square's pixels follow its (3, 1) px steps with a median drift of 0.3-0.6 px and >= 86 % stay visible, 94 % of the
    far background stays visible within 1 px (99th percentile), and 16-23 % of the covered strip passes its first step."""
    square, background, covered = scene_queries(corners, T, H, W, size, step)
    tr, vis = run(square)
    want = square[None, :, 1:] + np.arange(T, dtype=np.float32)[:, None, None] * np.asarray(step, np.float32)
    dev = np.abs(tr - want).max(2)
    for t in range(T):
        assert vis[t].mean() >= 0.8, ("square visible", t, vis[t].mean())
        assert np.median(dev[t][vis[t]]) <= 0.75, ("square drift", t, np.median(dev[t][vis[t]]))
        assert dev[t][vis[t]].max() <= 2.5, ("square drift max", t, dev[t][vis[t]].max())
    tr, vis = run(background)
    dev = np.abs(tr - background[None, :, 1:]).max(2)
    for t in range(T):
        assert vis[t].mean() >= 0.9, ("background visible", t, vis[t].mean())
        assert np.percentile(dev[t][vis[t]], 99) <= 1.25, ("background still", t)
    for t, q in enumerate(covered):
        tr, vis = run(q)
        assert len(q) > 100 and vis[t].all() and not vis[:t].any()
        assert vis[t + 1].mean() <= 0.35, ("covered strip visible after the step", t, vis[t + 1].mean())
        assert not vis[t + 1:][:, ~vis[t + 1]].any()   # an ended track stays ended
