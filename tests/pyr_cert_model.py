"""CPU statement of the certified pyramid arithmetic (k_pyr_down<PIX, PYR_CERTIFIED>): the fused
17-tap sum t', the guard that proves float32(t') == float32(t) for SciPy's sum t, and the frames the tests share.

    t   x[8] w0, then t = t + (x[8-k] + x[8+k]) * w[k] for k = 8 .. 1, every operation rounded   (scipy_sum)
    t'  the same with t' = fma(x[8-k] + x[8+k], w[k], t')                                         (fma_sum)

The FMA is modelled with fractions.Fraction and one rounding to double.  The guard mirrors the device's bit for bit:
the same thresholds, tested on the same bit patterns."""
import functools
from fractions import Fraction

import numpy as np

DELTA = 1 << 11          # fp64 ulps kept clear around a float32 rounding boundary (c R with c = 32, R = 64)
LOW29 = (1 << 29) - 1


def weights():
    """the half kernel SciPy builds for sigma = 2 (radius 8): w[k] at distance k"""
    x = np.arange(-8, 9)
    phi = np.exp(-0.5 / 4.0 * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[8:], np.float64)


def scipy_sum(x, w):
    """x [N, 17] float32 -> t [N] float64 in SciPy's operation order (NumPy never contracts)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = x[:, 8] * w[0]
        for k in range(8, 0, -1):
            t = t + (x[:, 8 - k] + x[:, 8 + k]) * w[k]
    return t


def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))   # only NaN / inf matter here, not the rounding
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))   # the sign of an exact zero
    return float(r)


def fma_sum(x, w):
    """x [N, 17] float32 -> t' [N] float64"""
    x = np.asarray(x, np.float32).astype(np.float64)
    out = np.empty(len(x), np.float64)
    wl = [float(v) for v in w]
    with np.errstate(all="ignore"):
        pairs = np.stack([x[:, 8 - k] + x[:, 8 + k] for k in range(8, 0, -1)], axis=1)   # the rounded fp64 pair sums
        t0 = x[:, 8] * w[0]
    for i in range(len(x)):
        if not x[i].any():
            out[i] = t0[i]   # an all-zero window: every operation is exact in both forms
            continue
        t = float(t0[i])
        for j, k in enumerate(range(8, 0, -1)):
            t = _fma(float(pairs[i, j]), wl[k], t)
        out[i] = t
    return out


def window_max(x):
    """largest |value| per window as the device takes it: fmaxf from 0, which drops a NaN"""
    return np.fmax.reduce(np.abs(np.asarray(x, np.float32)), axis=1, initial=np.float32(0))


def f32(t):
    with np.errstate(all="ignore"):
        return np.asarray(t, np.float64).astype(np.float32)


def guard_safe(tp, M):
    """the device's test (PyrCert::safe for one value): True only where float32(t') == float32(t) is proven"""
    tp = np.asarray(tp, np.float64)
    M = np.asarray(M, np.float32)
    lo = tp.view(np.uint64) & np.uint64(0xFFFFFFFF)
    y = ((lo + np.uint64((DELTA - (1 << 28)) & 0xFFFFFFFF)) << np.uint64(3)) & np.uint64(0xFFFFFFFF)
    ab = f32(tp).view(np.uint32) & np.uint32(0x7FFFFFFF)
    with np.errstate(all="ignore"):
        thr = np.fmax(M * np.float32(0.03125), np.float32(2.0 ** -125)).astype(np.float32).view(np.uint32)
    magnitude = ((ab >= thr) & (ab < np.uint32(0x7F000000))) | ((M == 0) & (ab == 0))
    return (y > np.uint64((2 * DELTA) << 3)) & magnitude


def midpoint_distance(t):
    """signed distance, in fp64 ulps, of t's low 29 mantissa bits from 2^28 (a float32 rounding boundary)"""
    lo29 = (np.asarray(t, np.float64).view(np.uint64) & np.uint64(LOW29)).astype(np.int64)
    return lo29 - (1 << 28)


def flag_vertical(img, cols=None):
    """the vertical pass over a whole image as the device's threads see it: a thread owns 12 consecutive rows of one
    column, M is the largest |value| of its 28 window rows.  Returns (flagged [H, len(cols)] bool, t' as float32)."""
    img = np.asarray(img, np.float32)
    H, W = img.shape
    cols = np.arange(W) if cols is None else np.asarray(cols)
    w = weights()
    nseg = (H + 11) // 12
    pad = np.pad(img[:, cols], ((8, 8 + nseg * 12 - H), (0, 0)), mode="symmetric")   # SciPy's "reflect"
    flagged = np.zeros((nseg * 12, len(cols)), bool)
    val = np.zeros((nseg * 12, len(cols)), np.float32)
    for s in range(nseg):
        regs = pad[s * 12: s * 12 + 28]                                         # [28, C]
        M = np.fmax.reduce(np.abs(regs), axis=0, initial=np.float32(0))
        for o in range(12):
            tp = fma_sum(regs[o: o + 17].T, w)
            flagged[s * 12 + o] = ~guard_safe(tp, M)
            val[s * 12 + o] = f32(tp)
    return flagged[:H], val[:H]


# ---------------------------------------------------------------------------------------------------------------
# adversarial windows: SciPy's t within a few fp64 ulps of a float32 rounding boundary
# ---------------------------------------------------------------------------------------------------------------
KINDS = ("u8", "uniform", "normal")
BANDS = ((0, 0), (1, 1), (2, 16), (17, 256))     # |distance| classes, in fp64 ulps


def random_windows(kind, n, rng):
    if kind == "u8":
        return rng.integers(0, 256, (n, 17)).astype(np.float32)
    if kind == "uniform":
        return rng.random((n, 17), dtype=np.float32)
    return rng.standard_normal((n, 17)).astype(np.float32)


def adversarial_windows(kind, seed, bases=6):
    """windows of one kind steered onto a boundary: tap 16 takes t to the nearest boundary as far as float32 allows,
    the tiny tap 0 sweeps the last few hundred ulps.  Returns {(band, side): [windows]} with side -1 / 0 / +1."""
    rng = np.random.default_rng(seed)
    w = weights()
    found = {}
    for base in random_windows(kind, bases, rng):
        x = base.copy()
        x[0] = 0.0
        t0 = scipy_sum(x[None], w)[0]
        if not np.isfinite(t0) or t0 == 0:
            continue
        mid = ((np.float64(t0).view(np.uint64) & ~np.uint64(LOW29)) | np.uint64(1 << 28)).view(np.float64)
        x[16] = np.float32(np.float64(x[16]) + (mid - t0) / w[8])
        t1 = scipy_sum(x[None], w)[0]
        v0 = (mid - t1) / w[8]
        q = np.spacing(abs(mid)) / w[8] / 4.0
        cand = np.repeat(x[None], 4097, axis=0)
        cand[:, 0] = (v0 + q * np.arange(-2048, 2049)).astype(np.float32)
        d = midpoint_distance(scipy_sum(cand, w))
        for lo, hi in BANDS:
            for side in ((0,) if lo == 0 else (-1, 1)):
                sel = np.flatnonzero((np.abs(d) >= lo) & (np.abs(d) <= hi) & (np.sign(d) == side))
                if len(sel):
                    pick = sel[:: max(1, len(sel) // 4)][:4]
                    found.setdefault(((lo, hi), side), []).extend(cand[pick])
    return found


@functools.lru_cache(maxsize=None)
def adversarial_set(seed=2024):
    """every kind's windows as one [N, 17] float32 array (the frames of the GPU test are built from it)"""
    out = []
    for i, kind in enumerate(KINDS):
        for ws in adversarial_windows(kind, seed + i).values():
            out.extend(ws)
    return np.asarray(out, np.float32)


def adversarial_frame(H, W, windows):
    """the windows laid down as columns (rows 1 .. 17: the vertical pass meets them at row 9) and below that, transposed,
    as rows repeated down the frame (a column-constant band passes the vertical blur unchanged: the horizontal pass
    meets them on the rows far enough inside it)"""
    f = np.zeros((H, W), np.float32)
    n = len(windows)
    top = min(17, H - 1)
    for c in range(W):
        f[1: 1 + top, c] = windows[c % n][:top]
    if H > 19:
        row = np.concatenate([windows[i % n] for i in range((W + 16) // 17)])[:W]
        f[19:, :] = row[None, :]
    return f


def adversarial_columns(W, n):
    """a few columns of adversarial_frame, one window each"""
    return np.arange(0, min(W, n), max(1, min(W, n) // 16))


# ---------------------------------------------------------------------------------------------------------------
# frames of the GPU test
# ---------------------------------------------------------------------------------------------------------------
def smooth_u8(H, W, seed=0):
    from oflk_synth import synth_pair

    return synth_pair(H, W, seed)[0]


def dots(H, W):
    f = np.zeros((H, W), np.float32)
    f[5::23, 7::29] = 255.0
    return f


def dot_columns(W):
    return np.arange(7, W, 29)


def frames(H, W):
    """name -> (float32 frame, is 8-bit valued)"""
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    normal = (rng.standard_normal((H, W)) * 100.0).astype(np.float32)
    smooth = smooth_u8(H, W)
    return {
        "smooth": (smooth, True),
        "noise": (rng.integers(0, 256, (H, W)).astype(np.float32), True),
        "checker": ((((yy // 24 + xx // 24) & 1) * 255).astype(np.float32), True),
        "dots": (dots(H, W), True),
        "zeros": (np.zeros((H, W), np.float32), True),
        "normal100": (normal, False),
        "tiny": ((smooth * np.float32(2.0 ** -120)).astype(np.float32), False),
        "huge": ((normal * np.float32(2.0 ** 100)).astype(np.float32), False),
        "adversarial": (adversarial_frame(H, W, adversarial_set()), False),
    }
