"""The statement of robust direct image alignment (oflk_align_refine_robust, oflk_align_sequence_robust, oflk_align_weights
and their host forms) in NumPy: Huber weights on the residuals, iteratively reweighted least squares.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_align.hpp, the robust form) are held to it
byte for byte, a NaN equal to a NaN.

It is align_model's statement (photometric=False) or align_photo_model's (photometric=True) with what follows changed;
everything not named here is theirs, operation for operation.  All of it is float64, every operation rounded on its own.

delta = f64(f32(robust_delta)), finite and > 0, in grey levels; one delta for every level.

2r. `sums_robust(l, M_l[, g, b])`: counted, r, sd and the columns c are the base statement's (plain: c = sd, NQ = NP;
    photometric: c = [g sd[0], .., g sd[NP-1], a, 1.0], NQ = NP + 2).  Per counted pixel
        ar = |r|
        w = ar > delta ? delta / ar : 1.0
        rho = ar > delta ? delta (ar - delta 0.5) : (r r) 0.5
        wc[i] = w c[i]
    A NaN r fails the comparison: w = 1 and the NaN poisons the sums as it does in the base statement.  The
    align_sums(NQ) + 2 sums (31 / 48 plain AFFINE / HOMOGRAPHY, 48 / 69 photometric), in this order:
    wc[i] c[j] for i = 0 .. NQ-1, j = i .. NQ-1;  wc[i] r for i = 0 .. NQ-1;  r r;  1.0;  rho;  w.  The order of every sum is
    align_model.ordered_sum's.
4r. The base statement's iteration on the weighted [G | b]; its freezes and the g, b update are unchanged.  The weights come
    from the current residual on every pass, at every level.
5r. before and after are sum(rho) / count at full resolution, the photometric before at (g, b) = (1, 0); status 2 when not
    after <= before.  stats (8,) float64, eight zeros for a refused step:
        [mean rho before, mean rho after, counted share, accepted updates, r r / count before, r r / count after,
         sum(w) / count before, sum(w) / count after]
    photo as align_photo_model's; (1.0f, 0.0f) without photometric.

`weights(a, b, model, kind, delta[, gain, bias])`: (H, W) float32 at full resolution: f32(w) at counted pixels and 0.0f
elsewhere, r formed as above (the float32 difference when gain and bias are not given, f64(v) - (g a + b) with g = f64(f32(gain)),
b = f64(f32(bias)) when they are).
"""
import numpy as np

import align_model as AM
import align_photo_model as APM
import homography_model as HM
from track_model import sample as bilinear

ONE = np.array([1.0, 0.0], np.float32)


def n_sums(kind, photometric=False):
    NQ = AM.n_params(kind) + (2 if photometric else 0)
    return NQ * (NQ + 1) // 2 + NQ + 2 + 2


def check_delta(robust_delta):
    with np.errstate(all="ignore"):
        delta = np.float64(np.float32(robust_delta))
    if not (np.isfinite(delta) and delta > 0):
        raise ValueError(f"robust_delta must be finite and > 0, got {robust_delta!r}")
    return delta


def _residual(lv, m, kind, photometric, g, b):
    """counted (H, W) bool, r (H, W) float64, the columns c (NQ arrays) of the base statements"""
    NP = AM.n_params(kind)
    H, W = lv.H, lv.W
    xs, ys, w = HM.coordinates(m, H, W)
    with np.errstate(all="ignore"):
        ok = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        v = np.zeros((H, W), np.float32)
        v[ok] = bilinear(lv.B, xs[ok], ys[ok])
        sd = [lv.gx * lv.xh, lv.gx * lv.yh, lv.gx, lv.gy * lv.xh, lv.gy * lv.yh, lv.gy]
        if NP == 8:
            t = sd[0] + sd[4]
            sd += [-(t * lv.xh), -(t * lv.yh)]
        if photometric:
            g, b = np.float64(g), np.float64(b)
            a = lv.A.astype(np.float64)
            r = v.astype(np.float64) - (g * a + b)
            c = [g * s for s in sd] + [a, np.ones((H, W))]
        else:
            r = (v - lv.A).astype(np.float64)
            c = sd
    return ok, r, [np.broadcast_to(x, (H, W)) for x in c]


def huber(r, delta):
    """w, rho of step 2r"""
    with np.errstate(all="ignore"):
        ar = np.abs(r)
        big = ar > delta
        w = np.where(big, delta / ar, 1.0)
        rho = np.where(big, delta * (ar - delta * 0.5), (r * r) * 0.5)
    return w, rho


def sums_robust(lv, m, kind, delta, photometric=False, g=1.0, b=0.0):
    """step 2r: (NS,) float64"""
    ok, r, c = _residual(lv, m, kind, photometric, g, b)
    NQ = len(c)
    with np.errstate(all="ignore"):
        w, rho = huber(r, delta)
        wc = [w * x for x in c]
        terms = [wc[i] * c[j] for i in range(NQ) for j in range(i, NQ)] + [wc[i] * r for i in range(NQ)]
        terms += [r * r, np.ones((lv.H, lv.W)), rho, w]
        return AM.ordered_sum(np.stack(terms), ok)


def refine_pyramids(pa, pb, model, robust_delta, status=1, kind=AM.HOMOGRAPHY, iterations=5, min_share=0.25, photometric=False):
    """one step on the two pyramids: (model like the input, status int, stats (8,) float64, photo (2,) float32)"""
    delta = check_delta(robust_delta)
    NP = AM.n_params(kind)
    NQ = NP + (2 if photometric else 0)
    model = np.asarray(model, np.float32).reshape(-1)
    assert model.size == (9 if kind == AM.HOMOGRAPHY else 6) and iterations >= 1
    if status == 0 or not np.isfinite(model).all():
        return model.copy(), 0, np.zeros(8), ONE.copy()
    m = [np.float64(c) for c in model] + ([np.float64(0.0), np.float64(0.0), np.float64(1.0)] if kind == AM.AFFINE else [])
    g, b = np.float64(1.0), np.float64(0.0)
    lvs = [AM.Level(x, y) for x, y in zip(pa, pb)]
    H, W = lvs[-1].H, lvs[-1].W
    share = np.float64(np.float32(min_share))
    with np.errstate(all="ignore"):
        S0 = sums_robust(lvs[-1], m, kind, delta, photometric, g, b)
        before = S0[-2] / S0[-3]
        frozen, accepted = False, 0
        for lv in lvs:
            if frozen:
                break
            sx, sy = np.float64(lv.W) / np.float64(W), np.float64(lv.H) / np.float64(H)
            m = AM.to_level(m, sx, sy)
            for _ in range(iterations):
                S = sums_robust(lv, m, kind, delta, photometric, g, b)
                if S[-3] < share * np.float64(lv.W * lv.H):
                    frozen = True
                    break
                q, ok = AM.solve(AM.normal_equations(S, NQ), NQ)
                if not ok:
                    frozen = True
                    break
                N, ok = AM.update(m, q, lv, NP)
                gn, bn = g, b
                if photometric:
                    gn, bn = g + q[NP], b + q[NP + 1]
                    ok = ok and bool(np.isfinite(gn) and np.isfinite(bn) and gn > 0)
                if not ok:
                    frozen = True
                    break
                m, g, b, accepted = N, gn, bn, accepted + 1
            m = AM.from_level(m, sx, sy)
        S1 = sums_robust(lvs[-1], m, kind, delta, photometric, g, b)
        after = S1[-2] / S1[-3]
        stats = np.array([before, after, S1[-3] / np.float64(W * H), accepted, S0[-4] / S0[-3], S1[-4] / S1[-3],
                          S0[-1] / S0[-3], S1[-1] / S1[-3]], np.float64)
        if accepted == 0:
            return model.copy(), 0, stats, ONE.copy()
        if not after <= before:
            return model.copy(), 2, stats, ONE.copy()
        out = np.array([c / m[8] for c in m] if kind == AM.HOMOGRAPHY else m[:6], np.float64).astype(np.float32)
    return out, 1, stats, np.array([g, b], np.float64).astype(np.float32)


def refine(a, b, model, robust_delta, status=None, kind=AM.HOMOGRAPHY, levels=3, iterations=5, min_share=0.25, photometric=False):
    """a, b (S, H, W) float32 or uint8, model (S, 6 | 9), status (S,) or None -> (model (S, nc) float32, status (S,) int32,
    stats (S, 8) float64, photo (S, 2) float32)"""
    a, b = np.asarray(a), np.asarray(b)
    model = np.asarray(model, np.float32).reshape(len(a), -1)
    return APM._stack([refine_pyramids(AM.pyramids(a[s], levels), AM.pyramids(b[s], levels), model[s], robust_delta,
                                       1 if status is None else int(status[s]), kind, iterations, min_share, photometric)
                       for s in range(len(a))])


def sequence(frames, model, robust_delta, status=None, kind=AM.HOMOGRAPHY, levels=3, iterations=5, min_share=0.25, photometric=False):
    """frames (T, H, W): the T-1 steps t -> t + 1, every frame's pyramid built once"""
    frames = np.asarray(frames)
    model = np.asarray(model, np.float32).reshape(len(frames) - 1, -1)
    pyr = [AM.pyramids(f, levels) for f in frames]
    return APM._stack([refine_pyramids(pyr[t], pyr[t + 1], model[t], robust_delta, 1 if status is None else int(status[t]), kind,
                                       iterations, min_share, photometric) for t in range(len(frames) - 1)])


def weights(a, b, model, kind, robust_delta, gain=None, bias=None):
    """the weight map of one step at full resolution: (H, W) float32"""
    delta = check_delta(robust_delta)
    model = np.asarray(model, np.float32).reshape(-1)
    assert model.size == (9 if kind == AM.HOMOGRAPHY else 6) and (gain is None) == (bias is None)
    m = [np.float64(c) for c in model] + ([np.float64(0.0), np.float64(0.0), np.float64(1.0)] if kind == AM.AFFINE else [])
    lv = AM.Level(np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32))
    photometric = gain is not None
    ok, r, _ = _residual(lv, m, kind, photometric, np.float32(gain) if photometric else 1.0, np.float32(bias) if photometric else 0.0)
    w, _ = huber(r, delta)
    return np.where(ok, w, 0.0).astype(np.float32)


same = APM.same
