"""The masked flow metrics statement in NumPy (test infrastructure; the product never imports this module).

What oflk_flow_metrics / oflk_plan_metrics compute for one pair: predicted flow (u, v) float32 (H, W), constant truth
(ut, vt) taken as float32, slice bounds (y0, y1, x0, x1) of mask[y0:y1, x0:x1] = True:

    rectangle    per bound i of an axis of length n:  i < 0 -> i + n, then clip to [0, n]; empty when y1 <= y0 or x1 <= x0
    per pixel    float32, every operation rounded on its own, in the reference's order (python/flow_metrics.py:14-163):
                   eu = up - ut;  ev = vp - vt;  sq = eu*eu + ev*ev;  len = sqrt(sq)
                   mag2 = up*up + vp*vp;  norm_p = sqrt(mag2 + 1);  norm_t = sqrt(ut*ut + vt*vt + 1)
                   c = (up*ut + vp*vt + 1) / (norm_p * norm_t), clipped to [-1, 1]; a NaN c stays NaN (np.clip)
    sums         of |eu|, |ev|, sq, len and arccos(float64(c)) * 57.29577951308232 over the rectangle, in float64.  The
                 model adds exactly (math.fsum); the device adds n non-negative terms in some order, so it is within
                 (n - 1) * 2^-53 relative of the model
    outputs      mae_u, mae_v, epe, aae = float32(sum / n);  rmse = sqrt(float32(sum_sq / n)) in float32;  n == 0 gives
                 NaN (0 / 0).  aae is 0.0 exactly when sqrt(ut^2 + vt^2) < 1e-6 (float64) and every pixel of the
                 rectangle has sqrt(mag2) < float32(1e-6): a NaN pixel has not, an empty rectangle has.

`pair_metrics` takes three hooks (clip, all_small, keep) so that tests/test_metrics_cpu.py can state a kernel mistake as
a change of one of them; the defaults are the statement.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

KEYS = ("mae_u", "mae_v", "rmse", "epe", "aae")
RAD2DEG = 57.29577951308232
SMALL = np.float32(1e-6)


def bound(i: int, n: int) -> int:
    """one slice bound on an axis of length n"""
    i = int(i)
    if i < 0:
        i += n
    return min(max(i, 0), n)


def rectangle(region, H: int, W: int):
    """(y0, y1, x0, x1) with 0 <= . <= H / W; the rectangle is empty when y1 <= y0 or x1 <= x0"""
    y0, y1, x0, x1 = region
    return bound(y0, H), bound(y1, H), bound(x0, W), bound(x1, W)


def count(rect) -> int:
    y0, y1, x0, x1 = rect
    return max(y1 - y0, 0) * max(x1 - x0, 0)


def clip_keep_nan(c):
    """np.clip's rule, spelled out: comparisons with NaN are false, so NaN passes through"""
    one = np.float32(1.0)
    return np.where(c < -one, -one, np.where(c > one, one, c)).astype(np.float32)


def all_small_per_pixel(mag) -> bool:
    """np.all(mag < 1e-6): every pixel must pass the comparison itself"""
    return bool(np.all(mag < SMALL))


def pixel_terms(up, vp, ut, vt, clip=clip_keep_nan):
    """(|eu|, |ev|, sq, len, c, mag) of flattened float32 predictions against the float32 truth"""
    up, vp = np.asarray(up, np.float32), np.asarray(vp, np.float32)
    ut, vt, one = np.float32(ut), np.float32(vt), np.float32(1.0)
    with np.errstate(all="ignore"):
        eu, ev = up - ut, vp - vt
        sq = eu * eu + ev * ev
        ln = np.sqrt(sq)
        mag2 = up * up + vp * vp
        norm_p = np.sqrt(mag2 + one)
        norm_t = np.sqrt(ut * ut + vt * vt + one)
        c = clip((up * ut + vp * vt + one) / (norm_p * norm_t))
        mag = np.sqrt(mag2)
    for a in (eu, ev, sq, ln, mag2, norm_p, c, mag):
        assert a.dtype == np.float32
    assert norm_t.dtype == np.float32
    return np.abs(eu), np.abs(ev), sq, ln, c, mag


def exact_sum(a) -> float:
    """the float64 nearest the exact sum of non-negative float64 terms; NaN if any term is, else inf if any is"""
    a = np.asarray(a, np.float64)
    if np.isnan(a).any():
        return math.nan
    if np.isinf(a).any():
        return math.inf
    step = 1 << 20   # one exact sum over all terms, fed a block at a time to bound the memory of the Python floats
    return math.fsum(itertools.chain.from_iterable(a[i:i + step].tolist() for i in range(0, a.size, step)))


def _f32_mean(total: float, n: int) -> np.float32:
    with np.errstate(all="ignore"):
        return np.float32(np.float64(total) / np.float64(n))


def pair_metrics(u, v, ut, vt, region, clip=clip_keep_nan, all_small=all_small_per_pixel, keep=None, rect=None):
    """dict of the five outputs as Python floats (each a float32 value).  Hooks: `clip` the cosine's clip, `all_small` the
    "nothing predicted" test on the rectangle's magnitudes, `keep` a function (n -> index array) choosing which flattened
    rectangle elements are summed (n stays the rectangle's count), `rect` a replacement for the clipped rectangle."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    H, W = u.shape
    y0, y1, x0, x1 = rectangle(region, H, W) if rect is None else rect
    n = count((y0, y1, x0, x1))
    if n:
        up, vp = u[y0:y1, x0:x1].reshape(-1), v[y0:y1, x0:x1].reshape(-1)
    else:
        up = vp = np.zeros(0, np.float32)
    if keep is not None:
        idx = keep(n)
        up, vp = up[idx], vp[idx]
    au, av, sq, ln, c, mag = pixel_terms(up, vp, ut, vt, clip)
    with np.errstate(all="ignore"):
        ang = np.arccos(c.astype(np.float64)) * RAD2DEG
    out = {"mae_u": _f32_mean(exact_sum(au), n), "mae_v": _f32_mean(exact_sum(av), n),
           "rmse": np.sqrt(_f32_mean(exact_sum(sq), n)), "epe": _f32_mean(exact_sum(ln), n),
           "aae": _f32_mean(exact_sum(ang), n)}
    assert all(x.dtype == np.float32 for x in out.values())
    mt = math.sqrt(float(np.float32(ut)) ** 2 + float(np.float32(vt)) ** 2)
    if mt < 1e-6 and all_small(mag):
        out["aae"] = np.float32(0.0)
    return {k: float(out[k]) for k in KEYS}


def batch_metrics(u, v, ut, vt, region, **hooks):
    """(B, 5) float64 array as the device returns it"""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    ut, vt = np.asarray(ut, np.float32).reshape(-1), np.asarray(vt, np.float32).reshape(-1)
    out = np.empty((u.shape[0], 5), np.float64)
    for b in range(u.shape[0]):
        m = pair_metrics(u[b], v[b], ut[b], vt[b], region, **hooks)
        out[b] = [m[k] for k in KEYS]
    return out


def kind(x: float) -> str:
    """class of an output: 'nan', '+inf', '-inf', 'zero' (exact 0.0) or 'finite'"""
    x = float(x)
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "+inf" if x > 0 else "-inf"
    return "zero" if x == 0.0 else "finite"


def ulps_apart(a: float, b: float) -> int:
    """distance of two finite float32 values in units in the last place (0 = equal)"""
    ia = int(np.float32(a).view(np.int32))
    ib = int(np.float32(b).view(np.int32))
    ia = ia if ia >= 0 else -(ia & 0x7FFFFFFF)
    ib = ib if ib >= 0 else -(ib & 0x7FFFFFFF)
    return abs(ia - ib)


def reference_bound(n: int, key: str, value: float, term_error: float) -> float:
    """How far a finite reference value (NumPy float32 pairwise means, float32 arccos / rad2deg) may lie from this model's:
    NumPy's float32 mean is within (ceil(n / 8192) + 32) * 2^-24 relative of the exact mean of non-negative terms (oflk.h,
    oflk_device_mean_error(OFLK_SUM_HOST, ...)), plus 2^-23 for the final roundings of the two sides; for `aae` each term of
    the reference's mean is off by at most `term_error` degrees (measured by tests/golden/make_golden_metrics.py over the
    scenes' own cosines, a property of NumPy), taken twice over."""
    rel = (math.ceil(n / 8192) + 32) * 2.0 ** -24 + 2.0 ** -23
    return rel * abs(value) + (2.0 * term_error if key == "aae" else 0.0)


def agrees_with_reference(got: float, ref, n: int, key: str, term_error: float) -> bool:
    """`ref` as the fixture stores it (a float, or "nan" / "inf" / "-inf"): NaN where the reference has NaN, the same
    infinity, aae == 0.0 exactly where it has 0.0, else within reference_bound"""
    ref = float(ref)
    if math.isnan(ref):
        return math.isnan(got)
    if math.isinf(ref) or math.isinf(got) or math.isnan(got):
        return got == ref
    if key == "aae" and ref == 0.0:
        return got == 0.0
    return abs(got - ref) <= reference_bound(n, key, ref, term_error)
