"""The statement of frame interpolation on colour and NV12 video in NumPy (include/oflk.h repeats it), on top of
tests/interp_model.py, whose side, sample, inside, status cases and rounding these are.  Test infrastructure; the product
never imports this module.

Packed colour.  Frames uint8 (B+1, H, W, C), C = 3 or 4, flows (B, H, W) float32 taken as given.  For every channel c,
new[..., c] is interp_model.interpolate on the planes frames[..., c] under these flows, and status is that call's: ok depends
on the flows only, so it is the same for every channel.  A fourth channel is interpolated like the others.

NV12.  Frames (B+1, 3H/2, W) uint8 (nv12_model.planes), H and W even and >= 4.  The Y plane of new is
interp_model.interpolate on the Y planes, and status is that call's.  Chroma: CH = H/2, CW = W/2, P_c[f] = UV[f][:, :, c].
The siting gives (sx, sy) (nv12_model.SITINGS).  Output chroma sample (column i, row j) sits at the luma position
X = f64(2 i) + sx, Y = f64(2 j) + sy, both exact, and runs interp_model.side's solve with (f64(x), f64(y)) replaced by (X, Y):
the same flows, R, forward-backward test and inside tests against the H x W luma frame.  That gives (px, py) and ok of the A
side (s = f64(tau)) and of the B side (s = 1.0 - f64(tau)).  A side's value for channel c is sample(P_c, cx, cy) with

    cx = clamp(0.5 * (px - sx), 0, CW - 1);  cy = clamp(0.5 * (py - sy), 0, CH - 1)     one subtraction, one product, float64
    clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v)

The clamp is there because a point inside the luma frame lies up to half a chroma sample beyond the chroma plane's first or
last row or column; the sample's cval 0 there would bleed saturated green into the frame's edge.  Where (px, py) is not inside
the luma frame ok is 0, the value is not used and is put as 0 here.  Blending with t = f32(tau): both sides ok a + t*(b - a);
only one its value; neither P_c[A][j][i] + t*(P_c[B][j][i] - P_c[A][j][i]); then rint to uint8.  The chroma positions' ok bits
are not returned.
"""
from __future__ import annotations

import numpy as np

import interp_model as M
import nv12_model as NM


def interpolate_packed(frames, uf, vf, ub, vb, taus, alpha=0.01, beta=0.5, refine=2):
    """(new (B, n, H, W, C) uint8, status (B, n, H, W) uint8) of frames (B+1, H, W, C) uint8 and flows (B, H, W)"""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] in (3, 4)
    per = [M.interpolate(np.ascontiguousarray(frames[..., c]), uf, vf, ub, vb, taus, alpha, beta, refine)
           for c in range(frames.shape[3])]
    for _, st in per[1:]:
        assert np.array_equal(st, per[0][1])
    return np.stack([p[0] for p in per], axis=-1), per[0][1]


def clamp(v, lo, hi):
    return np.where(v < lo, np.float64(lo), np.where(v > hi, np.float64(hi), v))


def solve_at(x0, y0, Fu, Fv, Gu, Gv, s, alpha, beta, refine):
    """interp_model.side's solve from the float64 start positions (x0, y0) (1-D): (px, py, ok)"""
    H, W = Fu.shape
    s = np.float64(s)
    px, py = x0.copy(), y0.copy()
    with np.errstate(all="ignore"):
        for _ in range(refine):
            us, vs = M.sample(Fu, px, py), M.sample(Fv, px, py)
            px = x0 - s * us.astype(np.float64)
            py = y0 - s * vs.astype(np.float64)
        us, vs = M.sample(Fu, px, py), M.sample(Fv, px, py)
        qx = px + us.astype(np.float64)
        qy = py + vs.astype(np.float64)
        bu, bv = M.sample(Gu, qx, qy), M.sample(Gv, qx, qy)
        eu, ev = us + bu, vs + bv
        e2 = eu * eu + ev * ev
        m2 = (us * us + vs * vs) + (bu * bu + bv * bv)
        assert e2.dtype == m2.dtype == np.float32
        ok = M.inside(px, py, H, W) & M.inside(qx, qy, H, W) & (e2 <= np.float32(alpha) * m2 + np.float32(beta))
    return px, py, ok


def chroma_side(P, Fu, Fv, Gu, Gv, s, sx, sy, alpha, beta, refine, clamped=True):
    """(value (CH, CW, 2) float32, ok (CH, CW) bool) of one side of the chroma planes P (CH, CW, 2) uint8.  clamped=False
    leaves the clamp out (what the statement is not: the no-green test shows the difference)"""
    H, W = Fu.shape
    CH, CW = P.shape[:2]
    jj, ii = np.meshgrid(np.arange(CH, dtype=np.float64), np.arange(CW, dtype=np.float64), indexing="ij")
    x0 = 2.0 * ii.ravel() + np.float64(sx)
    y0 = 2.0 * jj.ravel() + np.float64(sy)
    px, py, ok = solve_at(x0, y0, Fu, Fv, Gu, Gv, s, alpha, beta, refine)
    with np.errstate(all="ignore"):
        cx = 0.5 * (px - np.float64(sx))
        cy = 0.5 * (py - np.float64(sy))
        if clamped:
            cx, cy = clamp(cx, 0.0, CW - 1), clamp(cy, 0.0, CH - 1)
    lum = M.inside(px, py, H, W)
    val = np.zeros((CH * CW, 2), np.float32)
    for c in range(2):
        val[lum, c] = M.sample(np.ascontiguousarray(P[..., c], np.float32), cx[lum], cy[lum])
    return val.reshape(CH, CW, 2), ok.reshape(CH, CW)


def chroma_value(PA, PB, uf, vf, ub, vb, tau, siting="left", alpha=0.01, beta=0.5, refine=2, clamped=True):
    """the (CH, CW, 2) float32 chroma, before its conversion to uint8, of the frame at time tau between the frames whose chroma
    planes are PA and PB"""
    sx, sy = NM.SITINGS[siting]
    tau = np.float64(tau)
    uf, vf, ub, vb = (np.ascontiguousarray(f, np.float32) for f in (uf, vf, ub, vb))
    a, ok_a = chroma_side(PA, uf, vf, ub, vb, tau, sx, sy, alpha, beta, refine, clamped)
    b, ok_b = chroma_side(PB, ub, vb, uf, vf, np.float64(1.0) - tau, sx, sy, alpha, beta, refine, clamped)
    t = np.float32(tau)
    Af, Bf = np.asarray(PA, np.float32), np.asarray(PB, np.float32)
    out = Af + t * (Bf - Af)
    both = ok_a & ok_b
    out[both] = (a + t * (b - a))[both]
    out[ok_a & ~ok_b] = a[ok_a & ~ok_b]
    out[ok_b & ~ok_a] = b[ok_b & ~ok_a]
    assert out.dtype == np.float32
    return out


def chroma_pair(PA, PB, uf, vf, ub, vb, tau, siting="left", alpha=0.01, beta=0.5, refine=2, clamped=True):
    """the (CH, CW, 2) uint8 chroma of the frame at time tau between the frames whose chroma planes are PA and PB"""
    return np.rint(chroma_value(PA, PB, uf, vf, ub, vb, tau, siting, alpha, beta, refine, clamped)).astype(np.uint8)


def interpolate_nv12(frames, uf, vf, ub, vb, taus, siting="left", alpha=0.01, beta=0.5, refine=2, clamped=True):
    """(new (B, n, 3H/2, W) uint8, status (B, n, H, W) uint8) of frames (B+1, 3H/2, W) uint8 and flows (B, H, W)"""
    y, uv = NM.planes(frames)
    new_y, status = M.interpolate(np.ascontiguousarray(y), uf, vf, ub, vb, taus, alpha, beta, refine)
    Bn, n = len(y) - 1, len(taus)
    new_uv = np.empty((Bn, n) + uv.shape[1:], np.uint8)
    for b in range(Bn):
        for j, tau in enumerate(taus):
            new_uv[b, j] = chroma_pair(uv[b], uv[b + 1], uf[b], vf[b], ub[b], vb[b], tau, siting, alpha, beta, refine, clamped)
    H, W = y.shape[1:]
    new = NM.from_planes(new_y.reshape(Bn * n, H, W), new_uv.reshape((Bn * n,) + uv.shape[1:]))
    return new.reshape(Bn, n, 3 * H // 2, W), status
