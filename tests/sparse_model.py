"""The sparse pyramidal Lucas-Kanade statement in NumPy/SciPy (test infrastructure; the product never imports this module).

Points in, points + status + residual out (the shape of OpenCV's calcOpticalFlowPyrLK), built from the reference's own
operations.  The pyramids are oflk_oracle.build_gaussian_pyramid of each frame: level 0 is the coarsest, level L-1 the frame
itself, sizes (h_l, w_l) = pyramid_dims at scale 0.5.  sample(img, x, y) is track_model.sample (map_coordinates, order 1,
cval 0, float64 coordinates, float32 result).  Window w = 2h+1, odd, 3 <= w <= 11; K >= 1 iterations.

    step(A, B, x, y), (x, y) float32 inside [0, W-1] x [0, H-1]:
        g = (0, 0)                                                              float32
        for l = 0 .. L-1:
            l > 0:  g = (g.x * f32(w_l / w_{l-1}), g.y * f32(h_l / h_{l-1}))    upsample_flow's ratios
            (xl, yl) = (f64(x), f64(y)) at l = L-1, else
                       (f64(x) * (w_l - 1) / (W - 1), f64(y) * (h_l - 1) / (H - 1))      float64: multiply, then divide
            P[j][i] = sample(A_l, xl + i, yl + j),  i, j in [-(h+1), h+1]       once per level
            for k = 0 .. K-1:
                Q[j][i] = sample(B_l, (xl + f64(g.x)) + i, (yl + f64(g.y)) + j)
                (du, dv) = centre pixel (h+1, h+1) of the reference's lucas_kanade_single_scale(P, Q, w)
                solved = abs(det) > 1e-4 of that pixel
                g = g + (du, dv)
                leave the level when abs(du) < f32(0.01) and abs(dv) < f32(0.01)
        qx = f64(x) + f64(g.x);  qy = f64(y) + f64(g.y)
        ok = solved (last evaluated iteration of the finest level) and qx, qy finite and 0 <= qx <= W-1 and 0 <= qy <= H-1
        residual = f32(np.sum(abs(Pc - Qc)) / f32(w*w)),  Pc the w x w centre of the finest P,
                   Qc[j][i] = sample(B, qx + i, qy + j),  i, j in [-h, h]       float32, np.sum of the contiguous array
    a point that is not finite or outside the frame: ok = 0, NaN position, NaN residual

    tracks (rows, queries, t0, NaN conventions as track_model.track), for an alive point (x, y) on pair t:
        (qx, qy, g, ok, r)  = step(frame t, frame t+1, x, y)
        (_, _, g', ok', _)  = step(frame t+1, frame t, f32(qx), f32(qy))        only if ok
        us, vs = g;  bu, bv = g'
        eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
        alive = ok and ok' and e2 <= f32(alpha)*m2 + f32(beta) and r <= f32(max_residual)
        (x, y) = (f32(qx), f32(qy))

All points of a call go through one map_coordinates call per level and iteration, and their (w+2)^2 patches are laid out as
the tiles of one mosaic image on which the CPU oracle's lucas_kanade_single_scale runs once: a tile's centre pixel reads only
its own tile (the Sobel taps of the centre window stay inside it, the `symm` ring is never read), so it is exactly the stated
value, in the arithmetic the oracle is already pinned to.
"""
from __future__ import annotations

import math

import numpy as np

import oflk_oracle as O
from track_model import sample

F32 = np.float32


def sample_patches(img, x, y, r):
    """(M, 2r+1, 2r+1) float32: [m][j][i] = sample(img, x[m] + i, y[m] + j) for i, j in [-r, r]; x, y float64 (M,)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    o = np.arange(-r, r + 1)
    S = 2 * r + 1
    xs = np.broadcast_to(x[:, None, None] + o[None, None, :], (x.size, S, S))
    ys = np.broadcast_to(y[:, None, None] + o[None, :, None], (x.size, S, S))
    return sample(img, xs.ravel(), ys.ravel()).reshape(x.size, S, S)


def _solved(ix, iy):
    """abs(det) > 1e-4 of the windows' gradients (M, n), in the reference's float32 operations"""
    ix, iy = np.ascontiguousarray(ix, F32), np.ascontiguousarray(iy, F32)
    sxx, syy, sxy = (np.sum(np.ascontiguousarray(a), axis=1) for a in (ix * ix, iy * iy, ix * iy))
    det = sxx * syy - sxy * sxy
    assert det.dtype == F32
    return np.abs(det) > F32(1e-4)


def centre_flow(P, Q, w):
    """(du, dv, solved) (M,) of the patches P, Q (M, w+2, w+2): the mosaic route"""
    P, Q = np.ascontiguousarray(P, F32), np.ascontiguousarray(Q, F32)
    M, S, _ = P.shape
    assert S == w + 2 and Q.shape == P.shape
    if M == 0:
        return np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, bool)
    cols = int(math.ceil(math.sqrt(M)))
    rows = (M + cols - 1) // cols

    def mosaic(a):
        t = np.zeros((rows * cols, S, S), F32)
        t[:M] = a
        return np.ascontiguousarray(t.reshape(rows, cols, S, S).transpose(0, 2, 1, 3).reshape(rows * S, cols * S))

    mp, mq = mosaic(P), mosaic(Q)
    u, v = O.lucas_kanade_single_scale(mp, mq, w)
    ix, iy, _ = O.compute_gradients(mp, mq)
    m = np.arange(M)
    cy, cx = (m // cols) * S + S // 2, (m % cols) * S + S // 2

    def windows(a):
        t = a.reshape(rows, S, cols, S).transpose(0, 2, 1, 3).reshape(rows * cols, S, S)[:M]
        return t[:, 1:-1, 1:-1].reshape(M, w * w)

    solved = _solved(windows(ix), windows(iy))
    du, dv = u[cy, cx], v[cy, cx]
    assert not (du[~solved].any() or dv[~solved].any())
    return du, dv, solved


def centre_flow_one(P, Q, w):
    """the same for one pair of patches, patch by patch: the oracle on the (w+2)^2 patch itself"""
    P, Q = np.ascontiguousarray(P, F32), np.ascontiguousarray(Q, F32)
    u, v = O.lucas_kanade_single_scale(P, Q, w)
    ix, iy, _ = O.compute_gradients(P, Q)
    c = w // 2 + 1
    sxx = np.sum(np.ascontiguousarray(ix[1:-1, 1:-1] * ix[1:-1, 1:-1]))
    syy = np.sum(np.ascontiguousarray(iy[1:-1, 1:-1] * iy[1:-1, 1:-1]))
    sxy = np.sum(np.ascontiguousarray(ix[1:-1, 1:-1] * iy[1:-1, 1:-1]))
    det = sxx * syy - sxy * sxy
    return u[c, c], v[c, c], bool(np.abs(det) > F32(1e-4))


def check_config(shape, num_levels, window_size, num_iterations):
    """the statement's refusals that depend on the shape: raises ValueError"""
    H, W = shape
    if num_levels < 1 or num_iterations < 1:
        raise ValueError("levels and iterations must be >= 1")
    if window_size % 2 == 0 or not 3 <= window_size <= 11:
        raise ValueError("window outside the odd sizes 3..11")
    if min(min(d) for d in O.pyramid_dims(H, W, num_levels)) < 2:
        raise ValueError("a pyramid level with a dimension below 2")


def pyramid(frame, num_levels):
    return O.build_gaussian_pyramid(np.ascontiguousarray(frame, F32), num_levels)


def step(pa, pb, x, y, w, K):
    """one step of the points (x, y) (float32 (M,), all inside the frame) from pyramid pa to pyramid pb:
    (qx, qy float64, g (M, 2) float32, ok bool, residual float32)"""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    M, L, h = x.size, len(pa), w // 2
    H, W = pa[-1].shape
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    gx, gy = np.zeros(M, F32), np.zeros(M, F32)
    solved = np.zeros(M, bool)
    P = None
    for l in range(L):
        hl, wl = pa[l].shape
        if l > 0:
            hp, wp = pa[l - 1].shape
            gx, gy = gx * F32(wl / wp), gy * F32(hl / hp)
        if l == L - 1:
            xl, yl = x64, y64
        else:
            xl, yl = x64 * (wl - 1) / (W - 1), y64 * (hl - 1) / (H - 1)
        P = sample_patches(pa[l], xl, yl, h + 1)
        act = np.ones(M, bool)
        solved = np.zeros(M, bool)
        for _ in range(K):
            i = np.flatnonzero(act)
            if i.size == 0:
                break
            Q = sample_patches(pb[l], xl[i] + gx[i].astype(np.float64), yl[i] + gy[i].astype(np.float64), h + 1)
            du, dv, s = centre_flow(P[i], Q, w)
            solved[i] = s
            gx[i], gy[i] = gx[i] + du, gy[i] + dv
            act[i] = ~((np.abs(du) < F32(0.01)) & (np.abs(dv) < F32(0.01)))
        assert gx.dtype == gy.dtype == F32
    qx, qy = x64 + gx.astype(np.float64), y64 + gy.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = solved & np.isfinite(qx) & np.isfinite(qy) & (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    Pc = P[:, 1:-1, 1:-1]
    Qc = sample_patches(pb[-1], qx, qy, h)
    d = np.ascontiguousarray(np.abs(Pc - Qc).reshape(M, w * w))
    residual = np.sum(d, axis=1) / F32(w * w)
    assert d.dtype == F32 and residual.dtype == F32
    return qx, qy, np.stack([gx, gy], 1), ok, residual


def _inside(x, y, H, W):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= F32(W - 1)) & (y >= 0) & (y <= F32(H - 1))


def sparse_lk(prev, curr, pts, num_levels=3, window_size=5, num_iterations=3):
    """(next_pts (N, 2) float32, status (N,) uint8, residual (N,) float32) of one pair"""
    prev, curr = np.asarray(prev, F32), np.asarray(curr, F32)
    check_config(prev.shape, num_levels, window_size, num_iterations)
    pts = np.asarray(pts, F32).reshape(-1, 2)
    N = pts.shape[0]
    H, W = prev.shape
    nxt = np.full((N, 2), np.nan, F32)
    status = np.zeros(N, np.uint8)
    res = np.full(N, np.nan, F32)
    i = np.flatnonzero(_inside(pts[:, 0], pts[:, 1], H, W))
    qx, qy, _, ok, r = step(pyramid(prev, num_levels), pyramid(curr, num_levels), pts[i, 0], pts[i, 1], window_size,
                            num_iterations)
    nxt[i, 0], nxt[i, 1] = qx.astype(F32), qy.astype(F32)
    status[i] = ok
    res[i] = r
    return nxt, status, res


def track(frames, qt, qxy, num_levels=3, window_size=5, num_iterations=3, alpha=0.01, beta=0.5, max_residual=4.0, t0=0,
          prev=None, pyramids=None):
    """(tracks (B+1, N, 2) float32, visible (B+1, N) uint8): rows of frames t0 .. t0+B of the B+1 frames given (frames
    t0 .. t0+B of the sequence).  prev = (row, visible) of frame t0 from an earlier call, read for queries with qt < t0;
    qt None: every query at frame 0.  pyramids: the frames' pyramids, if the caller has them."""
    frames = np.asarray(frames, F32)
    B, H, W = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
    check_config((H, W), num_levels, window_size, num_iterations)
    pyr = pyramids if pyramids is not None else [pyramid(f, num_levels) for f in frames]
    qxy = np.asarray(qxy, F32).reshape(-1, 2)
    N = qxy.shape[0]
    qt = np.zeros(N, np.int64) if qt is None else np.asarray(qt, np.int64)
    tracks = np.full((B + 1, N, 2), np.nan, F32)
    visible = np.zeros((B + 1, N), np.uint8)
    alive = np.zeros(N, bool)
    x, y = np.zeros(N, F32), np.zeros(N, F32)
    q_in = _inside(qxy[:, 0], qxy[:, 1], H, W)
    a32, b32, r32 = F32(alpha), F32(beta), F32(max_residual)
    before = qt < t0
    if before.any():
        assert prev is not None, "queries before t0 need the previous call's row"
        prow, pvis = np.asarray(prev[0], F32), np.asarray(prev[1]).astype(bool)
        alive[before] = pvis[before]
        x[before], y[before] = prow[before, 0], prow[before, 1]
    for r in range(B + 1):
        if r > 0:
            i = np.flatnonzero(alive)
            fx, fy, g, ok, res = step(pyr[r - 1], pyr[r], x[i], y[i], window_size, num_iterations)
            nx, ny = fx.astype(F32), fy.astype(F32)
            j = np.flatnonzero(ok)
            _, _, gb, okb, _ = step(pyr[r], pyr[r - 1], nx[j], ny[j], window_size, num_iterations)
            us, vs, bu, bv = g[j, 0], g[j, 1], gb[:, 0], gb[:, 1]
            eu, ev = us + bu, vs + bv
            e2 = eu * eu + ev * ev
            m2 = (us * us + vs * vs) + (bu * bu + bv * bv)
            assert e2.dtype == m2.dtype == F32
            keep = np.zeros(i.size, bool)
            with np.errstate(invalid="ignore"):
                keep[j] = okb & (e2 <= a32 * m2 + b32) & (res[j] <= r32)
            alive[i] = keep
            x[i], y[i] = nx, ny
        start = qt == t0 + r
        alive[start] = q_in[start]
        x[start], y[start] = qxy[start, 0] + F32(0), qxy[start, 1] + F32(0)
        tracks[r, alive, 0], tracks[r, alive, 1] = x[alive], y[alive]
        visible[r, alive] = 1
    return tracks, visible


# ---- scenes ----------------------------------------------------------------------------------------------------------
def sinusoid_texture(H, W, dx=0.0, dy=0.0, seed=0, n=16, lo=16.0, hi=48.0):
    """a smooth analytic texture (n sinusoids of wavelength lo .. hi px, random directions and phases) rendered at the
    coordinates shifted by (dx, dy) -- its content moves by exactly (dx, dy) -- and rounded to 8 bits (uint8)"""
    rng = np.random.default_rng(seed)
    lam, th, ph = rng.uniform(lo, hi, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    amp = rng.uniform(0.5, 1.0, n)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = xx - dx, yy - dy
    f = sum(a * np.sin(2 * np.pi * (x * np.cos(t) + y * np.sin(t)) / l + p) for a, l, t, p in zip(amp, lam, th, ph))
    f = 127.5 + f * (100.0 / np.abs(amp).sum()) * 2.2
    return np.rint(np.clip(f, 0, 255)).astype(np.uint8)


def check_scene_sparse_tracks(run, T, corners, H, W, size, step, run_no_residual=None):
    """the meaning of sparse tracks on the occluder scene (fb_model.occluder_scene(5), 3/5/3, alpha 0.01, beta 0.5,
    max_residual 4.0); run(queries) -> (tracks (T, N, 2), visible (T, N) bool).  The statement's own values: square and
    background fully visible with a worst deviation of 0.014 / 0.018 px, and 0, 0, 0 and 3.5 % of the four covered strips
    alive one frame later; run_no_residual (max_residual = inf): 55 % of covered strip 0 survives, which is why the
    residual test is part of the tracker."""
    from track_model import scene_queries

    square, background, covered = scene_queries(corners, T, H, W, size, step)
    assert len(square) == 144 and len(background) == 5436 and [len(c) for c in covered] == [141] * 4
    tr, vis = run(square)
    want = square[None, :, 1:] + np.arange(T, dtype=np.float32)[:, None, None] * np.asarray(step, np.float32)
    for t in range(T):
        assert vis[t].mean() >= 0.99, ("square visible", t, vis[t].mean())
        assert np.abs(tr[t] - want[t])[vis[t]].max() <= 0.1, ("square deviation", t)
    tr, vis = run(background)
    for t in range(T):
        assert vis[t].mean() >= 0.99, ("background visible", t, vis[t].mean())
        assert np.abs(tr[t] - background[:, 1:])[vis[t]].max() <= 0.1, ("background drift", t)
    for t, q in enumerate(covered):
        tr, vis = run(q)
        assert vis[t].all() and not vis[:t].any()
        assert vis[t + 1].mean() <= 0.10, ("covered strip visible after the step", t, vis[t + 1].mean())
        assert not vis[t + 1:][:, ~vis[t + 1]].any()   # an ended track stays ended
    if run_no_residual is not None:
        _, vis = run_no_residual(covered[0])
        assert vis[1].mean() > 0.5, ("covered strip 0 without the residual test", vis[1].mean())
