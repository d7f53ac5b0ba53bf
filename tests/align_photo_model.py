"""The statement of direct image alignment with a photometric gain and bias (oflk_align_refine_photo,
oflk_align_sequence_photo and their host forms) in NumPy.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_align.hpp, the photometric form) are held to
it byte for byte, a NaN equal to a NaN.

It is align_model's statement with what follows changed; everything not named here is that file's, operation for operation.
A step carries two more float64 values, g = 1.0 and b = 0.0 at the start: "B under the model looks like g A + b".

2'. `sums_photo(l, M_l, g, b)`: counted, xs, ys, Gx, Gy, xh, yh and sd[0 .. NP-1] are align_model.sums'.
        v = sample(B_l, xs, ys) in float32;  a = f64(A_l[y][x])
        r = f64(v) - (g a + b), formed in float64, every operation rounded on its own
        c = [g sd[0], .., g sd[NP-1], a, 1.0]: NQ = NP + 2 columns
    and the align_sums(NQ) = NQ (NQ + 1) / 2 + NQ + 2 sums (46 AFFINE, 67 HOMOGRAPHY) over the counted pixels, in this order:
    c[i] c[j] for i = 0 .. NQ-1, j = i .. NQ-1;  c[i] r for i = 0 .. NQ-1;  r r;  1.0.  The order of every sum is
    align_model.ordered_sum's, unchanged.
3'. before: r r / count of sums_photo(L - 1, M, 1, 0) with the input model.
4'. An iteration: S = sums_photo(l, M_l, g, b); the count test (a); [G | rhs] of the sums eliminated without pivoting on NQ
    rows (b), giving q; steps (c), (d) on q[0 .. NP-1] unchanged; then g' = g + q[NP], b' = b + q[NP + 1].  (Minimise
    sum (r + g sd.dp - a dg - db)^2: with c as above the normal equations solve for [-dp, dg, db], so the geometric part of q
    keeps the plain statement's sign and the photometric part is added.)  The step freezes on align_model's four conditions,
    or when g' or b' is not finite, or when g' <= 0.  A step that freezes keeps M_l, g and b.  g and b are not rescaled
    between levels.
5'. after: r r / count of sums_photo(L - 1, M, g, b) with the final model and the final g, b.  Model, status and stats by
    align_model's rules.  photo = (f32(g), f32(b)) where the status is 1, otherwise (1.0f, 0.0f); a refused step (status_in 0
    or a model that is not finite) has (1, 0) too.
"""
import numpy as np

import align_model as AM
import homography_model as HM
from track_model import sample as bilinear


def n_sums(kind):
    NQ = AM.n_params(kind) + 2
    return NQ * (NQ + 1) // 2 + NQ + 2


def sums_photo(lv, m, kind, g, b):
    """step 2': (NS,) float64"""
    NP = AM.n_params(kind)
    NQ = NP + 2
    H, W = lv.H, lv.W
    g, b = np.float64(g), np.float64(b)
    xs, ys, w = HM.coordinates(m, H, W)
    with np.errstate(all="ignore"):
        ok = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        v = np.zeros((H, W), np.float32)
        v[ok] = bilinear(lv.B, xs[ok], ys[ok])
        a = lv.A.astype(np.float64)
        r = v.astype(np.float64) - (g * a + b)
        sd = [lv.gx * lv.xh, lv.gx * lv.yh, lv.gx, lv.gy * lv.xh, lv.gy * lv.yh, lv.gy]
        if NP == 8:
            t = sd[0] + sd[4]
            sd += [-(t * lv.xh), -(t * lv.yh)]
        c = [g * s for s in sd] + [a, np.ones((H, W))]
        c = [np.broadcast_to(x, (H, W)) for x in c]
        terms = [c[i] * c[j] for i in range(NQ) for j in range(i, NQ)] + [c[i] * r for i in range(NQ)]
        terms += [r * r, np.ones((H, W))]
        return AM.ordered_sum(np.stack(terms), ok)


def refine_pyramids(pa, pb, model, status=1, kind=AM.HOMOGRAPHY, iterations=5, min_share=0.25):
    """one step on the two pyramids: (model like the input, status int, stats (4,) float64, photo (2,) float32)"""
    NP, L = AM.n_params(kind), len(pa)
    NQ = NP + 2
    none = np.array([1.0, 0.0], np.float32)
    model = np.asarray(model, np.float32).reshape(-1)
    assert model.size == (9 if kind == AM.HOMOGRAPHY else 6) and iterations >= 1
    if status == 0 or not np.isfinite(model).all():
        return model.copy(), 0, np.zeros(4), none
    m = [np.float64(c) for c in model] + ([np.float64(0.0), np.float64(0.0), np.float64(1.0)] if kind == AM.AFFINE else [])
    g, b = np.float64(1.0), np.float64(0.0)
    lvs = [AM.Level(x, y) for x, y in zip(pa, pb)]
    H, W = lvs[-1].H, lvs[-1].W
    share = np.float64(np.float32(min_share))
    with np.errstate(all="ignore"):
        S = sums_photo(lvs[-1], m, kind, g, b)
        before = S[-2] / S[-1]
        frozen, accepted = False, 0
        for lv in lvs:
            if frozen:
                break
            sx, sy = np.float64(lv.W) / np.float64(W), np.float64(lv.H) / np.float64(H)
            m = AM.to_level(m, sx, sy)
            for _ in range(iterations):
                S = sums_photo(lv, m, kind, g, b)
                if S[-1] < share * np.float64(lv.W * lv.H):
                    frozen = True
                    break
                q, ok = AM.solve(AM.normal_equations(S, NQ), NQ)
                if not ok:
                    frozen = True
                    break
                N, ok = AM.update(m, q, lv, NP)
                gn, bn = g + q[NP], b + q[NP + 1]
                if not (ok and np.isfinite(gn) and np.isfinite(bn) and gn > 0):
                    frozen = True
                    break
                m, g, b, accepted = N, gn, bn, accepted + 1
            m = AM.from_level(m, sx, sy)
        S = sums_photo(lvs[-1], m, kind, g, b)
        after = S[-2] / S[-1]
        stats = np.array([before, after, S[-1] / np.float64(W * H), accepted], np.float64)
        if accepted == 0:
            return model.copy(), 0, stats, none
        if not after <= before:
            return model.copy(), 2, stats, none
        out = np.array([c / m[8] for c in m] if kind == AM.HOMOGRAPHY else m[:6], np.float64).astype(np.float32)
    return out, 1, stats, np.array([g, b], np.float64).astype(np.float32)


def _stack(r):
    return (np.stack([x[0] for x in r]), np.array([x[1] for x in r], np.int32), np.stack([x[2] for x in r]),
            np.stack([x[3] for x in r]))


def refine(a, b, model, status=None, kind=AM.HOMOGRAPHY, levels=3, iterations=5, min_share=0.25):
    """a, b (S, H, W) float32 or uint8, model (S, 6 | 9), status (S,) or None -> (model (S, nc) float32, status (S,) int32,
    stats (S, 4) float64, photo (S, 2) float32)"""
    a, b = np.asarray(a), np.asarray(b)
    model = np.asarray(model, np.float32).reshape(len(a), -1)
    return _stack([refine_pyramids(AM.pyramids(a[s], levels), AM.pyramids(b[s], levels), model[s],
                                   1 if status is None else int(status[s]), kind, iterations, min_share) for s in range(len(a))])


def sequence(frames, model, status=None, kind=AM.HOMOGRAPHY, levels=3, iterations=5, min_share=0.25):
    """frames (T, H, W): the T-1 steps t -> t + 1, every frame's pyramid built once"""
    frames = np.asarray(frames)
    model = np.asarray(model, np.float32).reshape(len(frames) - 1, -1)
    pyr = [AM.pyramids(f, levels) for f in frames]
    return _stack([refine_pyramids(pyr[t], pyr[t + 1], model[t], 1 if status is None else int(status[t]), kind, iterations,
                                   min_share) for t in range(len(frames) - 1)])


def same(got, want, what=""):
    """model, status, stats, photo byte for byte; a NaN equals a NaN"""
    AM.same(got[:3], want[:3], what)
    g, w = np.asarray(got[3]), np.asarray(want[3])
    assert g.shape == w.shape and g.dtype == w.dtype == np.float32, f"{what}: photo {g.shape} {g.dtype} != {w.shape} {w.dtype}"
    eq = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    assert eq.all(), f"{what}: photo differs at {np.argwhere(~eq)[:5].tolist()}: got {g[~eq][:5]}, want {w[~eq][:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def exposed(frame, gain, bias):
    """gain frame + bias as float32 (the product and the sum in float32)"""
    return (np.float32(gain) * np.asarray(frame, np.float32) + np.float32(bias)).astype(np.float32)


def pan_scene(T=8, H=96, W=128, step=5, seed=3, contrast=(40.0, 0.5)):
    """The 8-frame pan of a static scene under a changing exposure.  The source smooth_field(104, 171, seed) is compressed to
    40 + 0.5 v (contrast=(0.0, 1.0): left at 0 .. 255, so that exposed frames clip); frame t is the (H, W) window `step` px
    further right from offset (4, 4), exposed with gain 1 + 0.03 t and bias -2 t, rounded and clipped to uint8.
    -> (frames (T, H, W) uint8, source float64, gains (T,), biases (T,))"""
    import mosaic_model as MM

    src = contrast[0] + contrast[1] * MM.smooth_field(104, 171, seed).astype(np.float64)
    t = np.arange(T, dtype=np.float64)
    gains, biases = 1.0 + 0.03 * t, -2.0 * t
    frames = np.stack([np.clip(np.rint(gains[k] * src[4:4 + H, 4 + step * k:4 + step * k + W] + biases[k]), 0, 255).astype(np.uint8)
                       for k in range(T)])
    return frames, src, gains, biases
