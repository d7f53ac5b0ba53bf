"""CPU statement of the fp16 single-scale mode (k_lk16d in csrc/oflk_kernels.hpp, host setup in
oflk_plan_single_scale_fp16 in csrc/oflk.hip).

TEST INFRASTRUCTURE ONLY (tests/, tools/); nothing in the product imports it.  It restates the kernel's arithmetic
operation by operation, so that the kernel's flow equals it up to the one operation that is not correctly rounded, the
v_rcp_f32 of the solve (tests/test_gpu_fp16.py holds the kernel to 2 ulp of it and to its exact zero set):

  * range scaling: k is the smallest integer >= 0 with taps * (pixel_max/2 * 2^-k)^2 <= 60000 (the host's loop);
    s_g = 2^-k, s_t = s_g / 2, det_thr = float32(1e-4 * 2^-4k)
  * avg = (p + q) * (0.5 s_g) and It = (p - q) * s_t in float32, rows and columns clamped at the frame edges
  * Sobel/8 in float32, with the kernel's association: sm = (a0 + a2) + 2 a1, df = a0 - a2 over the rows above and
    below, Ix = (sm[x-1] - sm[x+1]) * 0.125, Iy = ((df[x-1] + df[x+1]) + 2 df[x]) * 0.125
  * fp16 conversion of Ix, Iy, It: round to nearest even, subnormals kept.  The library is built without denormal
    flushing: `make asm` shows `.amdhsa_float_denorm_mode_16_64 3` (fp16/fp64 denormals preserved on input and output)
    for every k_lk16d instance, and `.amdhsa_float_denorm_mode_32 3` as well
  * the five products and every fp16 add: computed in float64 (exact for fp16 operands) and rounded once to fp16, so
    each is the correctly rounded fp16 operation (the library builds with -ffp-contract=off: no fused operations)
  * vertical sums over blocks of S = 2HW+1 gradient rows aligned to absolute rows (block boundaries at rows = 0 mod S):
    the window ending at gradient row g is  suffix(previous block, from g-2HW) + prefix(current block, up to g), or the
    prefix alone when the window is the block; the prefix is a left fold, the suffix a right fold
  * horizontal sums over column pairs (even, odd) with the kernel's grouping for odd and even HW (see _horizontal)
  * solve in float32: det = Sxx Syy - Sxy Sxy, numerators unfused, solved where |det| > det_thr and the window lies in
    the frame (borders exactly 0), u = num * ((1/det) * 2) with an IEEE reciprocal where the kernel uses v_rcp_f32.

`variant` switches in deliberate deviations (tests/test_fp16_model.py shows the GPU tolerance sees each of them):
  "suffix_left_fold"  the previous block's suffix folded left to right
  "align1"            blocks aligned to rows = 1 mod S
  "seam_tap"          one tap column dropped in the first output column of every strip
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

F32 = np.float32
VARIANTS = ("suffix_left_fold", "align1", "seam_tap")
FP16_MAX = 65504.0


def range_scale(window_size: int, pixel_max: float) -> Tuple[int, float, float, np.float32]:
    """(k, s_g, s_t, det_thr) as oflk_plan_single_scale_fp16 sets them"""
    hw = window_size // 2
    taps = (2 * hw + 1) ** 2
    k = 0
    while taps * (0.5 * float(F32(pixel_max)) * 2.0 ** -k) ** 2 > 60000.0:
        k += 1
    s_g = float(F32(2.0 ** -k))
    return k, s_g, float(F32(0.5) * F32(s_g)), F32(1e-4 * 2.0 ** (-4 * k))


def strip_width(window_size: int) -> int:
    """output columns per wave (OUTW): 2 (64 - 2 ceil((HW+1)/2))"""
    hw = window_size // 2
    return 2 * (64 - 2 * ((hw + 2) // 2))


def segment_rows(B: int, H: int, W: int, window_size: int) -> int:
    """Hs, the rows per segment of the launch, as oflk_plan_single_scale_fp16 sizes it"""
    import math

    hw = window_size // 2
    strips = (W + strip_width(window_size) - 1) // strip_width(window_size) * B
    slots = 8192 if hw <= 2 else 6144 if hw == 3 else 5120 if hw == 4 else 4096
    segs = (H + 63) // 64
    rounds = strips * segs / slots
    if rounds > 0.75:
        segs = max(1, int(math.ceil(rounds - 0.25)) * slots // strips)
    else:
        segs = max(segs, min(slots // max(strips, 1), max(1, H // 40)))
    segs = min(segs, max(1, H // 8))
    return (H + segs - 1) // segs


class _Fp16:
    """correctly rounded fp16 results of float64 values (exact for one add or multiply of fp16 operands), tracking the
    largest finite-or-infinite magnitude produced"""

    def __init__(self, rounding: bool = True):
        self.rounding = rounding
        self.peak = 0.0

    def __call__(self, x: np.ndarray) -> np.ndarray:
        if self.rounding:
            with np.errstate(over="ignore", invalid="ignore"):
                x = np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
        with np.errstate(invalid="ignore"):
            m = np.nanmax(np.abs(x)) if x.size and not np.isnan(x).all() else 0.0
        self.peak = max(self.peak, float(m))
        return x


def _gradients(p: np.ndarray, q: np.ndarray, s_g: float, s_t: float, g_rows: np.ndarray):
    """float32 Ix, Iy, It of gradient rows g_rows (clamped into the frame), all columns"""
    H, W = p.shape
    ha, st = F32(0.5) * F32(s_g), F32(s_t)
    rows = lambda d: np.clip(g_rows + d, 0, H - 1)   # noqa: E731
    avg = lambda r: (p[r] + q[r]) * ha               # noqa: E731
    a0, a1, a2 = avg(rows(-1)), avg(rows(0)), avg(rows(1))
    it = (p[rows(0)] - q[rows(0)]) * st
    sm = (a0 + a2) + F32(2.0) * a1
    df = a0 - a2
    cl, cr = np.clip(np.arange(W) - 1, 0, W - 1), np.clip(np.arange(W) + 1, 0, W - 1)
    ix = (sm[:, cl] - sm[:, cr]) * F32(0.125)
    iy = ((df[:, cl] + df[:, cr]) + F32(2.0) * df) * F32(0.125)
    return ix, iy, it


def _vertical(c: np.ndarray, hw: int, r16: _Fp16, suffix_left_fold: bool = False) -> np.ndarray:
    """window sums over gradient rows g-2HW .. g for every row g of c ([5, nblocks*S, W], row 0 a block start).  Rows
    of the first block whose window reaches into the block before are NaN."""
    S = 2 * hw + 1
    n5, G, W = c.shape
    nb = G // S
    cb = c.reshape(n5, nb, S, W)
    pre = np.empty_like(cb)   # left fold over the block: fw = j == 0 ? c : fw + c
    pre[:, :, 0] = cb[:, :, 0]
    for j in range(1, S):
        pre[:, :, j] = r16(pre[:, :, j - 1] + cb[:, :, j])
    suf = np.full_like(cb, np.nan)   # ring[k] after the block: sum of slots k .. S-1
    if suffix_left_fold:
        for k in range(1, S):
            acc = cb[:, :, k]
            for j in range(k + 1, S):
                acc = r16(acc + cb[:, :, j])
            suf[:, :, k] = acc
    else:   # ring[k] = ring[k] + ring[k+1], k = S-2 .. 1
        suf[:, :, S - 1] = cb[:, :, S - 1]
        for k in range(S - 2, 0, -1):
            suf[:, :, k] = r16(cb[:, :, k] + suf[:, :, k + 1])
    prev_suf = np.concatenate([np.full_like(suf[:, :1], np.nan), suf[:, :-1]], axis=1)
    out = np.empty_like(cb)
    out[:, :, S - 1] = pre[:, :, S - 1]
    for j in range(S - 1):   # vs = ring[(j+1) % S] + fw
        out[:, :, j] = r16(prev_suf[:, :, j + 1] + pre[:, :, j])
    return out.reshape(n5, G, W)


def _horizontal(v: np.ndarray, hw: int, r16: _Fp16, seam_tap: int = 0) -> np.ndarray:
    """window sums over columns x-HW .. x+HW of the vertical sums v ([..., W]); columns whose window leaves the frame are
    NaN.  A lane holds the column pair (2l, 2l+1) as {lo, hi}; `seam_tap` = OUTW drops the last tap of every column x = 0
    mod OUTW (a deliberate coverage error)."""
    W = v.shape[-1]
    Wp = W + (W & 1)
    K = (hw - 1) // 2 if hw % 2 else hw // 2
    pad = K + 1
    vp = np.full(v.shape[:-1] + (Wp + 4 * pad,), np.nan)
    vp[..., 2 * pad:2 * pad + W] = v
    lo, hi = vp[..., 0::2], vp[..., 1::2]   # lane l + pad
    nl = Wp // 2
    sh = lambda a, d: a[..., pad + d:pad + d + nl]   # noqa: E731  (lane l + d)
    mlo, mhi = sh(lo, 0), sh(hi, 0)
    if hw % 2:   # odd HW: lanes l-K .. l+K both columns, lane l-K-1 its high, lane l+K+1 its low column
        for d in range(1, K + 1):   # m = m + (l + rr)
            mlo = r16(mlo + r16(sh(lo, -d) + sh(lo, d)))
            mhi = r16(mhi + r16(sh(hi, -d) + sh(hi, d)))
        s = r16(mlo + mhi)   # m + swap(m)
        out_lo, out_hi = sh(hi, -K - 1), sh(lo, K + 1)   # hi_lo(l, rr)
        o_lo, o_hi = r16(s + out_lo), r16(s + out_hi)
        part_lo = s
    else:        # even HW: lanes l-K+1 .. l+K-1 both columns; lane l-K both to lo, its high to hi; lane l+K ...
        for d in range(1, K):
            mlo = r16(mlo + r16(sh(lo, -d) + sh(lo, d)))
            mhi = r16(mhi + r16(sh(hi, -d) + sh(hi, d)))
        s = r16(mlo + mhi)                       # m + swap(m)
        e = r16(sh(hi, -K) + sh(lo, K))          # e1 + swap(e1), e1 = {l.hi, rr.lo}
        se = r16(s + e)
        o_lo, o_hi = r16(se + sh(lo, -K)), r16(se + sh(hi, K))   # + e2, e2 = {l.lo, rr.hi}
        part_lo = se
    out = np.empty(v.shape[:-1] + (Wp,))
    out[..., 0::2], out[..., 1::2] = o_lo, o_hi
    if seam_tap:
        xs = np.arange(0, Wp, seam_tap)
        out[..., xs] = part_lo[..., xs // 2]
    x = np.arange(Wp)
    out[..., (x < hw) | (x >= W - hw)] = np.nan
    return out[..., :W]


def _gradient_rows(y0: int, y1: int, hw: int, variant: Optional[str]) -> Tuple[int, int]:
    """gradient rows [g0, g1) for output rows [y0, y1): whole blocks from the one holding row y0 - HW (the first window
    row) to the one holding row y1 - 1 + HW"""
    S, align = 2 * hw + 1, 1 if variant == "align1" else 0
    return (y0 - hw - align) // S * S + align, -(-(y1 + hw - align) // S) * S + align


def _sums(c: np.ndarray, g0: int, y0: int, y1: int, H: int, hw: int, r16: _Fp16, variant: Optional[str]) -> np.ndarray:
    """the five window sums of output rows [y0, y1) from the product planes c of gradient rows g0 .. (block aligned);
    NaN where the window leaves the frame"""
    vsum = _vertical(c, hw, r16, suffix_left_fold=variant == "suffix_left_fold")
    vsum = vsum[:, y0 + hw - g0:y1 + hw - g0]   # the window of output row o ends at gradient row o + HW
    sums = _horizontal(vsum, hw, r16, seam_tap=strip_width(2 * hw + 1) if variant == "seam_tap" else 0)
    o = np.arange(y0, y1)
    sums[:, (o < hw) | (o >= H - hw)] = np.nan   # with _horizontal's columns: NaN exactly where the window leaves the frame
    return sums


def window_sums(c, window_size: int, variant: Optional[str] = None, rounding: bool = True) -> np.ndarray:
    """the model's fp16 window sums of given product planes c [n, H, W] (values exact in fp16), for every pixel; NaN
    where the window leaves the frame.  Rows outside the frame enter as NaN, so a sum that reaches them shows."""
    c = np.asarray(c, np.float64)
    n, H, W = c.shape
    hw = window_size // 2
    g0, g1 = _gradient_rows(0, H, hw, variant)
    cp = np.full((n, g1 - g0, W), np.nan)
    cp[:, -g0:H - g0] = c
    return _sums(cp, g0, 0, H, H, hw, _Fp16(rounding), variant)


def fp16_flow(prev, curr, window_size: int = 5, pixel_max: float = 255.0, rows: Optional[Tuple[int, int]] = None,
              return_sums: bool = False, return_peak: bool = False, variant: Optional[str] = None,
              rounding: bool = True):
    """the kernel's flow for [B,H,W] (or [H,W]) float32 frames: (u, v), plus the five fp16 window-sum planes
    {Sxx, Syy, Sxy, Sxt, Syt} (float64 holding fp16 values; NaN where the window leaves the frame) if `return_sums`, plus
    the largest |value| any fp16 operation produced if `return_peak`.  `rows` = (y0, y1) restricts the output to rows
    y0 .. y1-1 (u, v and the sums then have y1 - y0 rows).  `rounding=False` keeps every fp16 operation in float64."""
    p, q = np.asarray(prev, F32), np.asarray(curr, F32)
    squeeze = p.ndim == 2
    if squeeze:
        p, q = p[None], q[None]
    assert p.shape == q.shape and p.ndim == 3, (p.shape, q.shape)
    assert variant is None or variant in VARIANTS, variant
    B, H, W = p.shape
    y0, y1 = rows if rows is not None else (0, H)
    assert 0 <= y0 < y1 <= H, (y0, y1, H)
    hw = window_size // 2
    assert 1 <= hw <= 5 and window_size == 2 * hw + 1, window_size
    k, s_g, s_t, det_thr = range_scale(window_size, pixel_max)
    g0, g1 = _gradient_rows(y0, y1, hw, variant)
    g_rows = np.arange(g0, g1)
    r16 = _Fp16(rounding)
    us, vs, sums_out = [], [], []
    for b in range(B):
        ix, iy, it = (r16(a.astype(np.float64)) for a in _gradients(p[b], q[b], s_g, s_t, g_rows))
        c = np.stack([r16(ix * ix), r16(iy * iy), r16(ix * iy), r16(ix * it), r16(iy * it)])
        sums = _sums(c, g0, y0, y1, H, hw, r16, variant)
        Sxx, Syy, Sxy, Sxt, Syt = sums.astype(F32)
        with np.errstate(all="ignore"):
            det = Sxx * Syy - Sxy * Sxy
            inv = (F32(1.0) / det) * F32(2.0)
            solve = (np.abs(det) > det_thr) & ~np.isnan(Sxx)   # NaN: the window leaves the frame
            u = np.where(solve, (Sxy * Syt - Syy * Sxt) * inv, F32(0.0)).astype(F32)
            v = np.where(solve, (Sxy * Sxt - Sxx * Syt) * inv, F32(0.0)).astype(F32)
        us.append(u)
        vs.append(v)
        sums_out.append(sums)
    u, v, sums = np.stack(us), np.stack(vs), np.stack(sums_out, axis=1)
    if squeeze:
        u, v, sums = u[0], v[0], sums[:, 0]
    out = (u, v)
    if return_sums:
        out += (sums,)
    if return_peak:
        out += (r16.peak,)
    return out


def ulp_distance(a, b) -> np.ndarray:
    """|a - b| in float32 units in the last place (int64; -0 and +0 are the same point)"""
    def key(x):
        i = np.asarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def compare(u, v, mu, mv):
    """(zero sets equal, largest ulp distance on the rest): the kernel's flow (u, v) against the model's (mu, mv)"""
    zeros = np.array_equal(u == 0, mu == 0) and np.array_equal(v == 0, mv == 0)
    nz = (mu != 0) | (mv != 0)
    d = max(int(ulp_distance(u[nz], mu[nz]).max(initial=0)), int(ulp_distance(v[nz], mv[nz]).max(initial=0)))
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        d = max(d, 1 << 31)
    return zeros, d
