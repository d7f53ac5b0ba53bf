"""The forward-backward consistency statement in NumPy (test infrastructure; the product never imports this module).

Pair t has F = (uf, vf), the flow of frames t -> t+1, and G = (ub, vb), the flow of frames t+1 -> t.  float32 except where
stated, every operation rounded on its own:

    bu = warp_image(ub, uf, vf); bv = warp_image(vb, uf, vf)      the reference's warp_image (oflk_oracle.warp_image)
    eu = uf + bu;  ev = vf + bv
    e2 = eu*eu + ev*ev                                             each product rounded, then the sum
    err_f = sqrt(e2)                                               correctly rounded
    m2 = (uf*uf + vf*vf) + (bu*bu + bv*bv)                         in this order
    inside = (0 <= x + uf <= W-1) & (0 <= y + vf <= H-1)           float64, as warp_image forms its coordinates
    valid_f = inside & (e2 <= f32(alpha)*m2 + f32(beta))           product, then sum

err_b / valid_b: the same on frame t+1's grid with F and G exchanged.  oflk_fb_consistency must equal this bit for bit.
"""
from __future__ import annotations

import numpy as np

import oflk_oracle as O


def one_direction(u, v, pu, pv, alpha=0.01, beta=0.5):
    """(err, valid) of flow (u, v) against the partner flow (pu, pv), all (H, W)"""
    u, v, pu, pv = (np.ascontiguousarray(a, np.float32) for a in (u, v, pu, pv))
    H, W = u.shape
    bu = O.warp_image(pu, u, v)
    bv = O.warp_image(pv, u, v)
    eu = u + bu
    ev = v + bv
    e2 = eu * eu + ev * ev
    err = np.sqrt(e2)
    m2 = (u * u + v * v) + (bu * bu + bv * bv)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = xx + u.astype(np.float64)   # int64 + float32 -> float64, as warp_image
    y = yy + v.astype(np.float64)
    inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    valid = inside & (e2 <= np.float32(alpha) * m2 + np.float32(beta))
    assert e2.dtype == err.dtype == m2.dtype == np.float32
    return err, valid


def fb_check(uf, vf, ub, vb, alpha=0.01, beta=0.5):
    """(err_f, err_b, valid_f, valid_b) of flows of shape (H, W) or (B, H, W); valid as uint8 0 / 1"""
    uf, vf, ub, vb = (np.asarray(a, np.float32) for a in (uf, vf, ub, vb))
    if uf.ndim == 2:
        return tuple(r[0] for r in fb_check(uf[None], vf[None], ub[None], vb[None], alpha, beta))
    out = [[], [], [], []]
    for b in range(uf.shape[0]):
        ef, qf = one_direction(uf[b], vf[b], ub[b], vb[b], alpha, beta)
        eb, qb = one_direction(ub[b], vb[b], uf[b], vf[b], alpha, beta)
        for lst, r in zip(out, (ef, eb, qf.astype(np.uint8), qb.astype(np.uint8))):
            lst.append(r)
    return tuple(np.stack(lst) for lst in out)


def occluder_scene(T=3, H=96, W=128, size=36, step=(3, 1), seed=0):
    """T frames (float32 in [0, 255]): a textured square of `size` px moving by `step` = (dx, dy) whole px per frame over a
    textured static background, and the square's top-left corner in every frame"""
    rng = np.random.default_rng(seed)
    from scipy.ndimage import gaussian_filter

    bg = gaussian_filter(rng.random((H, W)) * 255.0, 1.5)
    fg = gaussian_filter(rng.random((size, size)) * 255.0, 1.5)
    bg = (bg - bg.min()) / (bg.max() - bg.min()) * 200.0 + 20.0
    fg = (fg - fg.min()) / (fg.max() - fg.min()) * 200.0 + 30.0
    x0, y0 = W // 4, H // 4
    frames, corners = [], []
    for t in range(T):
        x, y = x0 + step[0] * t, y0 + step[1] * t
        f = bg.copy()
        f[y:y + size, x:x + size] = fg
        frames.append(f.astype(np.float32))
        corners.append((y, x))
    return np.stack(frames), corners


def scene_regions(corners, t, H, W, size, step, margin):
    """boolean masks on frame t's grid: the background strip the square covers in frame t+1 (not covered in frame t), and
    the pixels at least `margin` px from both squares' boundaries"""
    (y, x), (y1, x1) = corners[t], corners[t + 1]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sq0 = (yy >= y) & (yy < y + size) & (xx >= x) & (xx < x + size)
    sq1 = (yy >= y1) & (yy < y1 + size) & (xx >= x1) & (xx < x1 + size)
    covered = sq1 & ~sq0
    near = np.zeros((H, W), bool)
    for (cy, cx) in ((y, x), (y1, x1)):
        near |= (yy >= cy - margin) & (yy < cy + size + margin) & (xx >= cx - margin) & (xx < cx + size + margin) & ~(
            (yy >= cy + margin) & (yy < cy + size - margin) & (xx >= cx + margin) & (xx < cx + size - margin))
    far = ~near & (xx >= margin) & (xx < W - margin) & (yy >= margin) & (yy < H - margin)
    return covered, far
