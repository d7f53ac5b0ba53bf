"""Cases for the stage entry points that take a free resampling ratio (test infrastructure):

    upsample_flow(flow_u, flow_v, target_shape)            -> oflk_upsample_flow
    build_gaussian_pyramid(image, num_levels, scale_factor) -> oflk_build_pyramid_w / oflk_build_pyramid

Every list is plain data and every field is seeded, so that tests/test_stages_cpu.py (the oracle against SciPy, and what
the lists cover) and tests/test_gpu_stages.py (the kernels against the oracle) walk the same cases.

Which kernel serves a case is decided on the host from the span of source cells that one output tile samples:

    k_upsample   a block of 256 x 16 outputs stages 136 coarse columns x 10 coarse rows per plane; a target whose blocks all
                 fit runs it (`staged`), any other the gathering kernel k_resample<2> (`fallback`)
    k_pyr_down   a block of 32 x 16 outputs stages 66 blurred columns x 34 blurred rows; a step with a radius-8 Gaussian
                 (scale_factor in (8/17, 8/15]) whose tiles all fit runs it (`fused`), any other k_blur<0>, k_blur<1>,
                 k_resample<1> (`unfused`)

`max_span` below restates the span arithmetic so that a test can NAME the span of a case (at the capacity, one over); the
decision itself is always asked of the library (oflk_upsample_staged, oflk_pyramid_step_fused).  The sizes in the lists
were picked with those two predicates; test_stages_cpu.py asserts that they still do what they were picked for.

The comparison rule (`same_bits`): NaN at the same positions, every other element the same 32 bits.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np

Shape = Tuple[int, int]

# outputs per block and staged source cells per block, (rows, columns): csrc/oflk_kernels.hpp kUTH/kUTW, kUSH/kUSW and
# kPTH/kPTW, kPBH/kPBW
UPSAMPLE_TILE, UPSAMPLE_CAP = (16, 256), (10, 136)
PYRAMID_TILE, PYRAMID_CAP = (16, 32), (34, 66)

B0 = 8.0 / 17.0 + 1e-9   # the lower end of the radius-8 band (int(4 / 0.4705882 + 0.5) is 9)
B1 = 8.0 / 15.0          # its upper end: 4 * 1.875 + 0.5 is exactly 8.0

# ---- upsample_flow: (coarse shape, target shape) ----------------------------------------------------------------------------
UPSAMPLE_CASES: List[Tuple[Shape, Shape]] = [
    # ratio about 2 over several x-tiles and y-tiles
    ((540, 960), (1080, 1920)), ((101, 158), (203, 317)), ((37, 641), (75, 1283)),
    # the predicate's edge in the columns (the rows fit): span 136 of 136, then 137
    ((20, 136), (40, 257)), ((20, 137), (40, 258)), ((20, 137), (40, 257)), ((20, 138), (40, 258)),
    # ... in the rows (the columns fit): span 10 of 10, then 11
    ((10, 80), (17, 160)), ((11, 80), (18, 160)), ((11, 80), (17, 160)), ((12, 80), (18, 160)),
    # both axes at their edge / one over
    ((10, 136), (17, 257)), ((11, 137), (18, 258)), ((11, 137), (17, 257)), ((12, 138), (18, 258)), ((10, 137), (17, 257)),
    ((11, 136), (17, 257)),
    # other ratios: 1.5x, 3x, 1x, 1.004x
    ((240, 320), (360, 480)), ((60, 80), (90, 120)), ((100, 130), (300, 390)), ((240, 320), (240, 320)), ((60, 80), (60, 80)),
    ((300, 700), (301, 701)),
    # shrinking
    ((480, 640), (240, 320)), ((60, 80), (30, 40)), ((500, 520), (171, 173)), ((137, 300), (16, 512)), ((137, 141), (16, 256)),
    # anisotropic
    ((60, 80), (7, 1000)), ((12, 300), (36, 900)),
    # degenerate
    ((1, 1), (40, 50)), ((1, 9), (3, 700)), ((9, 1), (700, 3)), ((2, 2), (33, 1025)), ((37, 53), (1, 1)), ((37, 53), (1, 300)),
]
# indices into UPSAMPLE_CASES of the cases that also run with NaN, +inf and -inf planted (plant_nonfinite)
UPSAMPLE_NONFINITE = [1, 3, 11, 5, 13, 17, 20, 22, 23, 28, 29]

# ---- build_gaussian_pyramid: (shape, levels, scale_factor) --------------------------------------------------------------------
PYRAMID_BAND: List[Tuple[Shape, int, float]] = [
    # 8/17 + 1e-9: columns fit up to 66 only; rows on both sides at every size
    ((47, 66), 2, B0), ((58, 66), 2, B0), ((41, 66), 2, B0), ((47, 67), 2, B0), ((697, 50), 2, B0), ((633, 60), 2, B0),
    ((64, 300), 2, B0), ((480, 640), 3, B0),
    # 0.48
    ((40, 66), 2, 0.48), ((42, 200), 2, 0.48), ((41, 200), 2, 0.48), ((44, 67), 2, 0.48), ((699, 604), 2, 0.48),
    ((81, 604), 2, 0.48), ((46, 69), 2, 0.48), ((480, 640), 3, 0.48),
    # 0.485: widths 66, 89, 91 at the capacity, 67, 69, 71 one over; heights 40, 42, 44 at the capacity, 41, 43, 45 one over
    ((40, 66), 2, 0.485), ((42, 89), 2, 0.485), ((44, 91), 2, 0.485), ((40, 67), 2, 0.485), ((42, 69), 2, 0.485),
    ((44, 71), 2, 0.485), ((41, 66), 2, 0.485), ((43, 89), 2, 0.485), ((45, 91), 2, 0.485), ((694, 699), 2, 0.485),
    ((694, 698), 2, 0.485), ((480, 640), 3, 0.485),
    # 0.49: every height fits (40, 42, 44 ... at the capacity), widths 67, 69 ... 157 do not
    ((40, 66), 2, 0.49), ((42, 68), 2, 0.49), ((44, 70), 2, 0.49), ((40, 67), 2, 0.49), ((48, 157), 2, 0.49),
    ((157, 696), 2, 0.49), ((153, 155), 2, 0.49), ((480, 640), 3, 0.49), ((1080, 1920), 2, 0.49),
    # 0.495, 0.499: everything fits; widths 66, 68 ... and heights 40 ... 48 at the capacity
    ((40, 66), 2, 0.495), ((44, 311), 2, 0.495), ((48, 309), 2, 0.495), ((203, 317), 2, 0.495), ((480, 640), 3, 0.495),
    ((40, 66), 2, 0.499), ((46, 96), 2, 0.499), ((48, 94), 2, 0.499), ((203, 317), 2, 0.499), ((480, 640), 3, 0.499),
    # above 0.5: everything fits, nothing reaches the capacity
    ((203, 317), 2, 0.51), ((33, 67), 2, 0.51), ((480, 640), 3, 0.51), ((1080, 1920), 2, 0.51),
    ((203, 317), 2, 0.52), ((75, 1283), 2, 0.52), ((480, 640), 3, 0.52),
    ((203, 317), 2, B1), ((130, 332), 2, B1), ((480, 640), 3, B1),
]
PYRAMID_UNFUSED: List[Tuple[Shape, int, float]] = [
    # the unfused chain at size
    ((480, 640), 3, 0.6), ((480, 640), 3, 0.4), ((480, 640), 3, 0.75), ((480, 640), 3, 0.3), ((480, 640), 3, 0.25),
    ((480, 640), 3, 0.9), ((480, 640), 3, 1.0),
    ((1080, 1920), 2, 0.75), ((1080, 1920), 2, 0.3),
    # block seams of k_resample at 256 outputs; output widths with Wo % 4 != 0 and == 0
    ((203, 317), 2, 0.6), ((203, 317), 2, 0.4), ((130, 332), 2, 0.6), ((130, 332), 2, 0.4), ((75, 1283), 2, 0.6),
    ((75, 1283), 2, 0.4), ((64, 4100), 2, 0.6), ((64, 4100), 2, 0.4),
    # radius 64, the largest accepted
    ((300, 400), 2, 1.0 / 16.0), ((20, 33), 2, 1.0 / 16.0),
    # levels shorter than the radius: the reflection folds more than once
    ((9, 7), 2, 0.25), ((3, 3), 2, 0.4), ((5, 40), 2, 0.3), ((40, 5), 2, 0.3), ((2, 2), 2, 0.5),
]
PYRAMID_CASES = PYRAMID_BAND + PYRAMID_UNFUSED
BAND_FACTORS = (B0, 0.48, 0.485, 0.49, 0.495, 0.499, 0.51, 0.52, B1)
# where a sweep of the predicate over sizes 40 .. 699 finds steps on both sides (rows, columns); elsewhere in the band every
# size is fused
BAND_BOTH_SIDES = {B0: (True, True), 0.48: (True, True), 0.485: (True, True), 0.49: (False, True), 0.495: (False, False),
                   0.499: (False, False), 0.51: (False, False), 0.52: (False, False), B1: (False, False)}
# refused today and still: (shape, levels, scale_factor, "invalid" | "unsupported")
PYRAMID_REFUSALS = [((1, 700), 2, 0.3, "invalid"),            # the second level would be 0 x 210
                    ((300, 400), 2, 0.062, "unsupported")]    # radius int(4 / 0.062 + 0.5) = 65


def gauss_radius(scale_factor: float) -> int:
    """radius of scipy.ndimage.gaussian_filter's kernel for sigma = 1 / scale_factor (truncate = 4)"""
    return int(4.0 * (1.0 / float(scale_factor)) + 0.5)


def level_shapes(shape: Shape, levels: int, scale_factor: float) -> List[Shape]:
    """fine to coarse: int(h * scale_factor) per step"""
    out = [(int(shape[0]), int(shape[1]))]
    for _ in range(levels - 1):
        h, w = out[-1]
        out.append((int(h * scale_factor), int(w * scale_factor)))
    return out


def pyramid_steps(shape: Shape, levels: int, scale_factor: float) -> List[Tuple[Shape, Shape]]:
    """(source shape, output shape) of every step of a case, finest first"""
    s = level_shapes(shape, levels, scale_factor)
    return list(zip(s[:-1], s[1:]))


def max_span(S: int, T: int, tile: int) -> int:
    """The most source cells along one axis that a tile of `tile` outputs touches when T outputs sample S cells on
    np.linspace(0, S - 1, T): from floor of the first coordinate to floor of the last plus one (capped at S - 1); the last
    tile starts no later than S - 2, since a sample exactly on the last cell is formed from the cell before it."""
    step = (S - 1) / (T - 1) if T > 1 else 0.0

    def at(i):
        return 0.0 if T <= 1 else (float(S - 1) if i == T - 1 else i * step)

    worst = 0
    for t0 in range(0, T, tile):
        last = min(t0 + tile, T) - 1
        lo = math.floor(at(t0))
        if t0 + tile >= T:
            lo = min(lo, max(S - 2, 0))
        hi = min(math.floor(at(last)) + 1, S - 1)
        worst = max(worst, hi - lo + 1)
    return worst


def upsample_spans(cshape: Shape, tshape: Shape) -> Shape:
    """(rows, columns) of the largest coarse span of a k_upsample block"""
    return max_span(cshape[0], tshape[0], UPSAMPLE_TILE[0]), max_span(cshape[1], tshape[1], UPSAMPLE_TILE[1])


def pyramid_spans(src: Shape, dst: Shape) -> Shape:
    """(rows, columns) of the largest blurred span of a k_pyr_down tile"""
    return max_span(src[0], dst[0], PYRAMID_TILE[0]), max_span(src[1], dst[1], PYRAMID_TILE[1])


def upsample_kernel(L, cshape: Shape, tshape: Shape) -> str:
    """the kernel liboflk (L) runs for this case"""
    return "k_upsample" if L.oflk_upsample_staged(cshape[0], cshape[1], tshape[0], tshape[1]) else "k_resample<2>"


def pyramid_kernels(L, shape: Shape, levels: int, scale_factor: float) -> List[str]:
    """the kernel liboflk (L) runs for each step of this case, finest first"""
    r = gauss_radius(scale_factor)
    return ["k_pyr_down" if L.oflk_pyramid_step_fused(s[0], s[1], d[0], d[1], r) else "k_blur+k_resample<1>"
            for s, d in pyramid_steps(shape, levels, scale_factor)]


def flow_fields(cshape: Shape, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """finite coarse flows: seeded normal fields, 3 px standard deviation"""
    rng = np.random.default_rng(1000 + seed)
    return rng.normal(0, 3, cshape).astype(np.float32), rng.normal(0, 3, cshape).astype(np.float32)


def plant_nonfinite(u: np.ndarray, v: np.ndarray, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """NaN, +inf and -inf at random cells, on the last row, on the last column and in both corners of the last row"""
    rng = np.random.default_rng(2000 + seed)
    u, v = u.copy(), v.copy()
    H, W = u.shape
    vals = (np.nan, np.inf, -np.inf)
    for k in range(max(3, u.size // 400)):
        a = u if k % 2 == 0 else v
        a[rng.integers(0, H), rng.integers(0, W)] = vals[k % 3]
    for k in range(3):
        u[H - 1, rng.integers(0, W)] = vals[k]
        v[rng.integers(0, H), W - 1] = vals[(k + 1) % 3]
    u[H - 1, W - 1] = np.inf
    v[H - 1, 0] = np.nan
    u[0, W - 1] = -np.inf
    return u, v


def image_field(shape: Shape, seed: int) -> np.ndarray:
    """a finite frame: a seeded normal field around mid-grey"""
    rng = np.random.default_rng(3000 + seed)
    return rng.normal(120, 40, shape).astype(np.float32)


def diff_report(got: np.ndarray, exp: np.ndarray) -> Optional[str]:
    """None when `got` equals `exp` under the rule above; else the count of differing elements and the first differing index
    with both values"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != np.float32 or exp.dtype != np.float32:
        return f"shape/dtype {got.shape} {got.dtype} against {exp.shape} {exp.dtype}"
    gn, en = np.isnan(got), np.isnan(exp)
    bad = (gn != en) | (~gn & ~en & (got.view(np.uint32) != exp.view(np.uint32)))
    n = int(bad.sum())
    if n == 0:
        return None
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    rows, cols = np.unique(np.argwhere(bad)[:, 0]), np.unique(np.argwhere(bad)[:, 1])
    return (f"{n} of {got.size} elements differ; first at {idx}: got {got[idx]!r} ({int(got.view(np.uint32)[idx]):#010x}), "
            f"expected {exp[idx]!r} ({int(exp.view(np.uint32)[idx]):#010x}); rows {rows[:8].tolist()}{'...' if rows.size > 8 else ''} "
            f"columns {cols[:8].tolist()}{'...' if cols.size > 8 else ''}")


def same_bits(got, exp, what: str) -> None:
    msg = diff_report(got, exp)
    assert msg is None, f"{what}: {msg}"
