"""The temporal-denoising statement in NumPy (test infrastructure; the product never imports this module).

Frames are [T][H][W], float32 or uint8.  F_s = (uf[s], vf[s]) is the flow from frame s to frame s+1 and G_s = (ub[s], vb[s])
the flow from frame s+1 to frame s.  sample and inside are interp_model's: a point that is not inside [0, W-1] x [0, H-1]
samples as 0 and reads no tap.  R = radius is in [1, 4]; h2 = f32(strength) * f32(strength).  Every float32 and float64
operation is rounded on its own.

    for output frame t, pixel (x, y):
      c = f32(frame[t][y][x]);  num = c;  den = 1.0f;  count = 0
      two chains, backward (sgn = -1) and forward (sgn = +1), each: (px, py) = (f64(x), f64(y)), alive
      for k = 1 .. R:   for sgn in (-1, +1), in this order:
        s' = t + sgn*k;  the chain has ended, or s' < 0, or s' > T-1: nothing
        forward:  (A, B) = (F_{s'-1}, G_{s'-1});   backward: (A, B) = (G_{s'}, F_{s'})
        us = sample(A.u, px, py); vs = sample(A.v, px, py)
        qx = px + f64(us); qy = py + f64(vs)
        bu = sample(B.u, qx, qy); bv = sample(B.v, qx, qy)
        eu = us + bu; ev = vs + bv; e2 = eu*eu + ev*ev; m2 = (us*us + vs*vs) + (bu*bu + bv*bv)
        ok = inside(qx, qy) and e2 <= f32(alpha)*m2 + f32(beta)
        not ok: the chain ends (no sample from this frame or any beyond it on this side)
        ok: (px, py) = (qx, qy);  v = sample(frame[s'], qx, qy);  d = v - c;  w = 1.0f - (d*d) / h2
            if w > 0:  num = num + w*v;  den = den + w;  count += 1        (a NaN w is not > 0)
      out = num / den     (float32 division, correctly rounded)
      uint8 frames: out clamped to [0, 255], then (unsigned char) rintf, half to even

oflk_denoise_frames_host must equal this byte for byte, out and count.
"""
from __future__ import annotations

import numpy as np

from interp_model import inside, sample

MAX_RADIUS = 4
# the quality scenes' seeds: the texture, the mover's texture and the noise
SCENE_SEED, MOVER_SEED, NOISE_SEED = 0, 1, 2
SIGMA = 10.0


def denoise_frame(frames, uf, vf, ub, vb, t, strength, radius=2, alpha=0.01, beta=4.0):
    """(out (H, W) float32 before the uint8 conversion, count (H, W) uint8) of output frame t; frames (T, H, W) float32"""
    T, H, W = frames.shape
    h2 = np.float32(strength) * np.float32(strength)
    al, be = np.float32(alpha), np.float32(beta)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    c = frames[t].ravel().copy()
    num, den, count = c.copy(), np.ones(H * W, np.float32), np.zeros(H * W, np.uint8)
    chains = {-1: [xx.ravel().copy(), yy.ravel().copy(), np.ones(H * W, bool)],
              +1: [xx.ravel().copy(), yy.ravel().copy(), np.ones(H * W, bool)]}
    with np.errstate(all="ignore"):
        for k in range(1, radius + 1):
            for sgn in (-1, +1):
                s = t + sgn * k
                px, py, alive = chains[sgn]
                if s < 0 or s > T - 1 or not alive.any():
                    continue
                if sgn > 0:
                    Au, Av, Bu, Bv = uf[s - 1], vf[s - 1], ub[s - 1], vb[s - 1]
                else:
                    Au, Av, Bu, Bv = ub[s], vb[s], uf[s], vf[s]
                i = np.flatnonzero(alive)          # a chain that has ended takes no sample
                x, y = px[i], py[i]
                us, vs = sample(Au, x, y), sample(Av, x, y)
                qx, qy = x + us.astype(np.float64), y + vs.astype(np.float64)
                bu, bv = sample(Bu, qx, qy), sample(Bv, qx, qy)
                eu, ev = us + bu, vs + bv
                e2 = eu * eu + ev * ev
                m2 = (us * us + vs * vs) + (bu * bu + bv * bv)
                assert e2.dtype == m2.dtype == np.float32
                ok = inside(qx, qy, H, W) & (e2 <= al * m2 + be)
                alive[i[~ok]] = False
                i, qx, qy = i[ok], qx[ok], qy[ok]
                px[i], py[i] = qx, qy
                v = sample(frames[s], qx, qy)
                d = v - c[i]
                w = np.float32(1.0) - (d * d) / h2
                assert w.dtype == np.float32
                take = w > 0
                j = i[take]
                num[j] = num[j] + w[take] * v[take]
                den[j] = den[j] + w[take]
                count[j] += 1
        out = num / den
    assert out.dtype == np.float32
    return out.reshape(H, W), count.reshape(H, W)


def denoise(frames, uf, vf, ub, vb, strength, radius=2, alpha=0.01, beta=4.0):
    """(out (T, H, W) in the frames' type, count (T, H, W) uint8) of frames (T, H, W) and flows (T-1, H, W)"""
    frames = np.asarray(frames)
    assert 1 <= radius <= MAX_RADIUS and frames.ndim == 3
    u8 = frames.dtype == np.uint8
    f32 = np.ascontiguousarray(frames, np.float32)
    uf, vf, ub, vb = (np.ascontiguousarray(f, np.float32) for f in (uf, vf, ub, vb))
    out, count = np.empty(f32.shape, np.float32), np.empty(f32.shape, np.uint8)
    for t in range(len(f32)):
        out[t], count[t] = denoise_frame(f32, uf, vf, ub, vb, t, strength, radius, alpha, beta)
    if u8:
        out = np.rint(np.clip(out, np.float32(0), np.float32(255))).astype(np.uint8)
    return out, count


def average_in_place(frames, radius=2):
    """what a caller has without flows: the mean of the frames t-radius .. t+radius that exist, where they lie (float32)"""
    f = np.asarray(frames, np.float32)
    T = len(f)
    return np.stack([f[max(t - radius, 0):min(t + radius, T - 1) + 1].mean(axis=0, dtype=np.float64) for t in range(T)]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the quality scenes: clean frames with a known motion, and the same frames with Gaussian noise
# ---------------------------------------------------------------------------------------------------------------------
def _texture(rng, h, w):
    """interp_model.pan_scene's texture on an h x w canvas: four octaves of smoothed noise, scaled to [20, 235]"""
    from scipy.ndimage import gaussian_filter

    noise = rng.standard_normal((4, h, w))
    canvas = sum(wt * s * gaussian_filter(noise[i], s) for i, (wt, s) in enumerate(((8, 16), (4, 8), (2, 4), (1, 2))))
    return (canvas - canvas.min()) / (canvas.max() - canvas.min()) * 215.0 + 20.0


def pan_sequence(dx, dy, T=7, H=96, W=128, seed=SCENE_SEED):
    """T clean float32 frames: the multi-octave texture under a pan of (dx, dy) px a frame.  A frame is the 2 x 2 box average
    of a crop of a canvas at twice the resolution; frame t's crop has moved by 2 t (dx, dy) canvas px, so the scene moves by
    +(dx, dy) frame px a frame, exactly."""
    m = 2 * T * max(abs(dx), abs(dy), 1)
    canvas = _texture(np.random.default_rng(seed), 2 * H + 2 * m, 2 * W + 2 * m)

    def frame(t):
        oy, ox = m - 2 * t * dy, m - 2 * t * dx
        return np.ascontiguousarray(canvas[oy:oy + 2 * H, ox:ox + 2 * W].reshape(H, 2, W, 2).mean(axis=(1, 3)), np.float32)

    return np.stack([frame(t) for t in range(T)])


def mover_sequence(step=9, T=7, H=96, W=128, size=(28, 20)):
    """(clean frames, touched (H, W) bool): pan_sequence(0, 0) with a textured rectangle of size (height, width) crossing it at
    `step` px a frame along x, and the pixels the rectangle covers in any frame"""
    frames = pan_sequence(0, 0, T, H, W)
    h, w = size
    patch = _texture(np.random.default_rng(MOVER_SEED), 4 * h, 4 * w)[:h, :w]
    patch = ((patch - patch.min()) / (patch.max() - patch.min()) * 215.0 + 20.0).astype(np.float32)
    touched = np.zeros((H, W), bool)
    y0, x0 = (H - h) // 2, 16
    for t in range(T):
        x = x0 + step * t
        frames[t, y0:y0 + h, x:x + w] = patch
        touched[y0:y0 + h, x:x + w] = True
    return frames, touched


def noisy(frames, sigma=SIGMA, seed=NOISE_SEED):
    """the frames with Gaussian noise of `sigma` grey levels (float32, not clipped)"""
    rng = np.random.default_rng(seed)
    return (frames + sigma * rng.standard_normal(frames.shape)).astype(np.float32)


def relative_error(got, clean, noisy_frames, mask=None, margin=12):
    """the mean squared error of `got` against the clean frames over that of the noisy input, `margin` px inside the border
    (and inside `mask` (H, W) where one is given)"""
    T, H, W = clean.shape
    m = np.zeros((H, W), bool)
    m[margin:H - margin, margin:W - margin] = True
    if mask is not None:
        m &= mask
    e = ((np.asarray(got, np.float64) - clean) ** 2)[:, m].mean()
    return e / ((np.asarray(noisy_frames, np.float64) - clean) ** 2)[:, m].mean()
