"""The frame-interpolation statement in NumPy (test infrastructure; the product never imports this module).

Pair b has frames A = frame b and B = frame b+1, each float32 or uint8, F = (uf, vf) the flow A -> B and G = (ub, vb) the
flow B -> A.  The output time tau is a double in the open interval (0, 1).  sample(img, x, y) is track_model.sample
(map_coordinates, order 1, cval 0, float64 points, float32 result) with one case stated on top of it: a coordinate that is
not inside [0, W-1] x [0, H-1] -- the negated closed comparison in float64, so NaN and the infinities are not inside --
samples as 0 and reads no tap.  Every float32 and float64 operation is rounded on its own.  For output pixel (x, y),
R = refine >= 1:

    side(img, F, G, s):                         s = f64(tau) for the A side, 1.0 - f64(tau) for the B side
        px = f64(x); py = f64(y)
        repeat R times:
            us = sample(F.u, px, py); vs = sample(F.v, px, py)
            px = f64(x) - s * f64(us); py = f64(y) - s * f64(vs)
        us = sample(F.u, px, py); vs = sample(F.v, px, py)
        qx = px + f64(us); qy = py + f64(vs)
        bu = sample(G.u, qx, qy); bv = sample(G.v, qx, qy)
        eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
        ok = inside(px, py) and inside(qx, qy) and e2 <= f32(alpha)*m2 + f32(beta)
        return sample(img, px, py), ok

    a, ok_a = side(A, F, G, tau);   b, ok_b = side(B, G, F, 1 - tau);   t = f32(tau)
    both: out = a + t*(b - a)   only ok_a: out = a   only ok_b: out = b   neither: out = A[y][x] + t*(B[y][x] - A[y][x])
    status = ok_a | (ok_b << 1)
    uint8 frames: (unsigned char) rintf(out), half to even;  float32 frames: out

oflk_interpolate_frames must equal this byte for byte.
"""
from __future__ import annotations

import numpy as np

import track_model


def inside(x, y, H, W):
    with np.errstate(invalid="ignore"):
        return ~(~((x >= 0) & (x <= W - 1)) | ~((y >= 0) & (y <= H - 1)))


def sample(img, x, y):
    """track_model.sample at the points inside the frame; 0, and no tap read, at every other point (NaN, inf included)"""
    H, W = img.shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ok = inside(x, y, H, W)
    out = np.zeros(x.shape, np.float32)
    out[ok] = track_model.sample(img, x[ok], y[ok])
    return out


def side(img, Fu, Fv, Gu, Gv, s, alpha, beta, refine):
    """(value (H, W) float32, ok (H, W) bool) of one side; s a float64"""
    H, W = Fu.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x0, y0 = xx.ravel(), yy.ravel()
    s = np.float64(s)
    px, py = x0.copy(), y0.copy()
    with np.errstate(all="ignore"):
        for _ in range(refine):
            us, vs = sample(Fu, px, py), sample(Fv, px, py)
            px = x0 - s * us.astype(np.float64)
            py = y0 - s * vs.astype(np.float64)
        us, vs = sample(Fu, px, py), sample(Fv, px, py)
        qx = px + us.astype(np.float64)
        qy = py + vs.astype(np.float64)
        bu, bv = sample(Gu, qx, qy), sample(Gv, qx, qy)
        eu, ev = us + bu, vs + bv
        e2 = eu * eu + ev * ev
        m2 = (us * us + vs * vs) + (bu * bu + bv * bv)
        assert e2.dtype == m2.dtype == np.float32
        ok = inside(px, py, H, W) & inside(qx, qy, H, W) & (e2 <= np.float32(alpha) * m2 + np.float32(beta))
    return sample(np.asarray(img, np.float32), px, py).reshape(H, W), ok.reshape(H, W)


def interpolate_pair(A, B, uf, vf, ub, vb, tau, alpha=0.01, beta=0.5, refine=2):
    """(out (H, W) in the frames' type, status (H, W) uint8) at time tau between A and B"""
    u8 = A.dtype == np.uint8
    tau = np.float64(tau)
    Af, Bf = np.asarray(A, np.float32), np.asarray(B, np.float32)
    uf, vf, ub, vb = (np.ascontiguousarray(f, np.float32) for f in (uf, vf, ub, vb))
    a, ok_a = side(Af, uf, vf, ub, vb, tau, alpha, beta, refine)
    b, ok_b = side(Bf, ub, vb, uf, vf, np.float64(1.0) - tau, alpha, beta, refine)
    t = np.float32(tau)
    out = Af + t * (Bf - Af)
    both = ok_a & ok_b
    out[both] = (a + t * (b - a))[both]
    out[ok_a & ~ok_b] = a[ok_a & ~ok_b]
    out[ok_b & ~ok_a] = b[ok_b & ~ok_a]
    assert out.dtype == np.float32
    status = ok_a.astype(np.uint8) | (ok_b.astype(np.uint8) << 1)
    return (np.rint(out).astype(np.uint8) if u8 else out), status


def interpolate(frames, uf, vf, ub, vb, taus, alpha=0.01, beta=0.5, refine=2):
    """(new (B, n, H, W) in the frames' type, status (B, n, H, W) uint8) of frames (B+1, H, W) and flows (B, H, W)"""
    frames = np.asarray(frames)
    Bn, n = frames.shape[0] - 1, len(taus)
    new = np.empty((Bn, n) + frames.shape[1:], frames.dtype)
    status = np.empty(new.shape, np.uint8)
    for b in range(Bn):
        for j, tau in enumerate(taus):
            new[b, j], status[b, j] = interpolate_pair(frames[b], frames[b + 1], uf[b], vf[b], ub[b], vb[b], tau, alpha, beta,
                                                       refine)
    return new, status


def cross_fade(A, B, tau):
    """what a caller has without flows: A + f32(tau) * (B - A) in float32"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    return A + np.float32(tau) * (B - A)


def oracle_flows(O, frames, levels=3, window=5, iters=3):
    """the CPU oracle's flows (uf, vf, ub, vb), each (T-1, H, W), of a float32 frame sequence"""
    fl = [[], [], [], []]
    for t in range(len(frames) - 1):
        for lst, a in zip(fl, O.lucas_kanade_pyramidal(frames[t], frames[t + 1], levels, window, iters) +
                          O.lucas_kanade_pyramidal(frames[t + 1], frames[t], levels, window, iters)):
            lst.append(a)
    return [np.stack(x) for x in fl]


def pan_scene(dx, dy, H=96, W=128, seed=0):
    """(A, middle, B) float32 in [20, 235]: a multi-octave texture under a pan of (dx, dy) px between A and B, with the true
    frame at tau = 0.5.  The texture is four octaves of smoothed noise (sigma 16, 8, 4, 2 at twice the frames' resolution,
    each scaled by its sigma, weights 8, 4, 2, 1) on a canvas with a margin; a frame is the 2 x 2 box average of a crop of
    that canvas, and the crops of A, the middle and B lie (dx, dy) canvas px apart -- half a pan each in frame px, so that
    the middle frame is exact for odd pans too.  The scene moves by +(dx, dy): B[y, x] shows what A[y - dy, x - dx] did."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    m = 4 * max(abs(dx), abs(dy), 1)
    noise = rng.standard_normal((4, 2 * H + 2 * m, 2 * W + 2 * m))
    canvas = sum(w * s * gaussian_filter(noise[i], s) for i, (w, s) in enumerate(((8, 16), (4, 8), (2, 4), (1, 2))))
    canvas = (canvas - canvas.min()) / (canvas.max() - canvas.min()) * 215.0 + 20.0

    def frame(ox, oy):   # the crop whose content has moved by (ox, oy) canvas px
        c = canvas[m - oy:m - oy + 2 * H, m - ox:m - ox + 2 * W]
        return np.ascontiguousarray(c.reshape(H, 2, W, 2).mean(axis=(1, 3)), np.float32)

    return frame(0, 0), frame(dx, dy), frame(2 * dx, 2 * dy)
