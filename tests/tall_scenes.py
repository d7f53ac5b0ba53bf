"""Frames at the tallest and widest shapes the entry checks accept (test infrastructure; the product never imports this
module): the shapes, the builders and the thresholds of tests/test_tall_cpu.py and tests/test_gpu_tall.py.

A tall frame can be narrow, so these shapes are cheap: what they reach is the launch arithmetic.  Ten launch sites put rows
(the NV12 interpolation: columns) on grid.y with no cap, launch_lk chains, unchains and tables its tile rows by the height,
and every kernel forms row offsets with the signed 24-bit __mul24.  The heights below sit just past each threshold.

Frames are an analytic texture: two sinusoids of different orientation whose phases wander with an integer hash of the row
band (so no two stretches of rows repeat), moved by a small smooth flow that is non-zero at both ends of the frame.  From
row `plant_from` on a third sinusoid is added: content that only the blocks past the 65 535th reach.  Nothing here is random.

The comparison rule of the GPU file is stage_scenes.same_bits / test_gpu_fb._same: NaN at the same positions, every other
value the same bits.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import numpy as np

# ---- the constants of the code under test, restated -------------------------------------------------------------------------------
MAX_DIM = 1 << 23          # csrc/oflk.hip kMaxDim: H, W >= 2^23 are refused (signed 24-bit row products)
MAX_PIXELS = 1 << 30       # check_hw: H W < 2^30
MAX_PLAN_PIXELS = 1 << 29  # check_frame_bounds (plans, trackers): H W < 2^29
GRID_CAP = 65535           # the y / z extent that the capped launches (corner, warp, metrics, alignment, fits) loop at
ROWS_2D = 4                # grid2d, grid_resample, k_lk_generic's grid: 4 rows x 64 (256) columns per block
COLS_2D, COLS_RESAMPLE = 64, 256
ROWS_16 = 16               # csrc/oflk_kernels.hpp kPTH (k_pyr_down) and kUTH (k_upsample): 16 output rows per block
COLS_NV12 = 64             # interp_launch, NV12: ceil(W / 64) column blocks on grid.y
K5TX, K5TY = 64, 24        # csrc/oflk_kernels.hpp k5TX, k5TY: k_lkw's tile
MAX_SEGS = 40              # kMaxSegs: launch_lk's segment table; seg_row is unsigned short
CAP_ENV, RESIDENT = 8, 1024  # launch_lk: tiles per chained block at most; 256 CUs x 4 blocks

# ---- the base heights -------------------------------------------------------------------------------------------------------------
T4 = 262152                # grid.y = 65 538 at 4 rows per block: past both 65 535 and 65 536
T16 = 1048600              # 65 538 blocks of 16 output rows
C = 1572840                # exactly 65 535 tile rows of 24: the longest chain, seg_row at its last value
C1 = 1572888               # 65 537 tile rows: the cap = 1 branch
TOP = MAX_DIM - 1          # the bound
NV12_W = 4194368           # 65 537 column blocks of 64: block index 65 536 exists

PREFILL_F32, PREFILL_U8, PREFILL_STATUS = -7.5, 77, 9   # what the device forms' outputs hold before the call


def blocks(n: int, per_block: int) -> int:
    return (n + per_block - 1) // per_block


# ---- launch_lk's chain arithmetic, restated ---------------------------------------------------------------------------------------
def lk_cap(B: int, H: int, W: int, hw: int = 2, chained_mode: bool = True) -> int:
    """tile rows per chained block of k_lkw for B pairs of H x W (1: one tile per block, the table unused)"""
    tiles_x, tiles_y = blocks(W, K5TX), blocks(H, K5TY)
    per_slot = B * tiles_x * tiles_y // RESIDENT
    cap = min(max(1, CAP_ENV), per_slot // 5) if chained_mode else 1
    cap = max(cap, (tiles_y + MAX_SEGS // 2 - 1) // (MAX_SEGS // 2))
    if not chained_mode or hw > 2 or per_slot < 10 or tiles_y > 65535:
        cap = 1
    return cap


def lk_segments(H: int, cap: int) -> List[int]:
    """seg_row of launch_lk for cap > 1: the first tile row of every segment, then tiles_y"""
    tiles_y = blocks(H, K5TY)
    rows, row = [], 0
    while row < tiles_y:
        rest = tiles_y - row
        length = min(cap, max(1, rest // 2))
        if len(rows) == MAX_SEGS - 1:
            length = rest
        rows.append(row)
        row += length
    return rows + [tiles_y]


def level_shapes(shape, levels: int):
    """finest first: int(h * 0.5) per step"""
    out = [(int(shape[0]), int(shape[1]))]
    for _ in range(levels - 1):
        out.append((int(out[-1][0] * 0.5), int(out[-1][1] * 0.5)))
    return out


# ---- the texture ------------------------------------------------------------------------------------------------------------------
def _hash01(k: np.ndarray, salt: int) -> np.ndarray:
    """an integer hash of k (int64) into [0, 1): Knuth's multiplicative hash, xor-folded"""
    x = (k.astype(np.uint64) * np.uint64(2) + np.uint64(salt)) * np.uint64(2654435761)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    return (x & np.uint64(0xffff)).astype(np.float64) / 65536.0


def _phase(yr: np.ndarray, salt: int) -> np.ndarray:
    """a continuous phase in [0, pi) that wanders from one band of 64 rows to the next by the hash of the band"""
    k = np.floor(yr / 64.0)
    f = yr / 64.0 - k
    a, b = _hash01(k.astype(np.int64) + 4, salt), _hash01(k.astype(np.int64) + 5, salt)
    return np.pi * (a + (b - a) * f)


def motion(y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """the scene's motion per frame step at row y, px: (dx, dy), smooth in y and non-zero everywhere"""
    return 0.35 + 0.2 * np.sin(y * 7e-4), -0.3 + 0.15 * np.cos(y * 5e-4)


def _wave(amp, kx: float, x: np.ndarray, phi: np.ndarray) -> np.ndarray:
    """amp * sin(kx * x + phi) for a row of columns x and a column of per-row phases phi, by the addition theorem: no
    transcendental per pixel"""
    return (amp * np.cos(phi)) * np.sin(kx * x) + (amp * np.sin(phi)) * np.cos(kx * x)


def _tall(H: int, W: int, t: int, plant_from: int, rows=None) -> np.ndarray:
    """rows = (first, last + 1): only those rows of the H x W frame"""
    r0, r1 = rows or (0, H)
    out = np.empty((r1 - r0, W), np.float32)
    x = np.arange(W, dtype=np.float64)[None, :]
    for y0 in range(r0, r1, 1 << 20):
        y = np.arange(y0, min(y0 + (1 << 20), r1), dtype=np.float64)[:, None]
        dx, dy = motion(y)
        sx, yr = t * dx, y - t * dy     # the texture at (x - sx, yr)
        f = 120.0 + _wave(45.0, 0.8, x, 0.35 * yr + _phase(yr, 0) - 0.8 * sx) + _wave(35.0, -0.45, x, 0.7 * yr + _phase(yr, 1) + 0.45 * sx)
        if plant_from < H:
            f += _wave(30.0 * np.clip((yr - plant_from) / 32.0, 0.0, 1.0), 0.61, x, 0.43 * yr - 0.61 * sx)
        out[y0 - r0:y0 - r0 + y.shape[0]] = f
    return out


def frames(shape, T: int = 2, plant_from: int = None, u8: bool = False, rows=None) -> np.ndarray:
    """(T, H, W) float32 in [10, 230] (uint8: rounded): the texture at times 0 .. T-1.  The longer axis is the one the
    texture's bands and the planted content run along; plant_from defaults to 65 535 blocks of 4 along it.  rows = (first,
    last + 1): a crop of those lines of the long axis."""
    H, W = shape
    wide = W > H
    n_long, n_short = (W, H) if wide else (H, W)
    if plant_from is None:
        plant_from = GRID_CAP * ROWS_2D
    fr = [_tall(n_long, n_short, t, plant_from, rows) for t in range(T)]
    out = np.stack([np.ascontiguousarray(f.T) if wide else f for f in fr])
    assert 10.0 <= out.min() and out.max() <= 230.0
    return np.rint(out).astype(np.uint8) if u8 else out


def flow_fields(shape, salt: int = 0, amp: float = 3.0) -> Tuple[np.ndarray, np.ndarray]:
    """(u, v) float32 of `shape`: smooth fields of up to `amp` px, hashed along the rows like the texture; on a frame of 8
    columns many points leave the frame"""
    H, W = shape
    u, v = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
    x = np.arange(W, dtype=np.float64)[None, :]
    for y0 in range(0, H, 1 << 20):
        y = np.arange(y0, min(y0 + (1 << 20), H), dtype=np.float64)[:, None]
        u[y0:y0 + y.shape[0]] = _wave(amp, 0.9, x, 0.37 * y + 2.0 * _phase(y, 2 + salt))
        v[y0:y0 + y.shape[0]] = _wave(amp, 0.5, x, -0.21 * y + 2.0 * _phase(y, 3 + salt) + 0.5 * np.pi)
    return u, v


BAD = (np.nan, np.inf, -np.inf, 1e30, -1e30)


def interp_flows(B: int, H: int, W: int, long_axis: int = 0) -> List[np.ndarray]:
    """[uf, vf, ub, vb], each (B, H, W) float32: slowly varying flows of up to 1.5 px with the backward field close to minus
    the forward one (most pixels pass the forward-backward test); every 53rd line along the long axis and the fourth line
    from the end are wild (their points leave the frame); NaN, +-inf and +-1e30 are planted in every plane in the first
    lines, in the middle and in the last eight lines, which only the blocks past the 65 535th reach.  An axis of one pixel
    has no flow along it."""
    n, m = (W, H) if long_axis == 1 else (H, W)
    ax, ay = min(1.5, (m - 1) / 3.0), 1.5
    x = np.arange(m, dtype=np.float64)[None, :]
    w = [np.empty((n, m), np.float32) for _ in range(4)]
    for y0 in range(0, n, 1 << 20):
        y = np.arange(y0, min(y0 + (1 << 20), n), dtype=np.float64)[:, None]
        for k, (kx, ky) in enumerate(((0.15, 0.02), (-0.11, 0.031), (0.9, 0.37), (0.5, -0.21))):
            w[k][y0:y0 + y.shape[0]] = _wave(1.0, kx, x, ky * y + 2.0 * _phase(y, 10 + k))
    planes = [ax * w[0], ay * w[1], -ax * w[0] + 0.05 * ax * w[2], -ay * w[1] + 0.05 * w[3]]
    wild = np.arange(n) % 53 == 17
    wild[n - 4] = True
    for p, q in zip(planes, (w[2], w[3], w[3], w[2])):
        p[wild] = q[wild] * (2.0 * m + 4.0)
    lines = [1, 5, n // 2, n // 2 + 3, n - 8, n - 6, n - 5, n - 3, n - 2, n - 1]
    for k, p in enumerate(planes):
        for j, line in enumerate(lines):
            p[line, (3 * j + k) % m] = BAD[(j + k) % len(BAD)]
    if long_axis == 1:   # the long axis is x: exchange the roles of u and v with the axes
        planes = [planes[1].T, planes[0].T, planes[3].T, planes[2].T]
    return [np.ascontiguousarray(np.broadcast_to(p, (B,) + p.shape), np.float32) for p in planes]


# ---- far-end conditions -----------------------------------------------------------------------------------------------------------
def _differ(a: np.ndarray, b) -> float:
    """the share of elements of a that are not equal to b (NaN equals nothing)"""
    return float(np.mean(a != b))


def far_end(exp: np.ndarray, per_block: int, prefill, what: str, axis: int = 0, alias: bool = True, trim: int = 0) -> int:
    """Asserts the far-end conditions on an expected output whose `axis` lies on a grid axis at `per_block` lines a block:
    the lines that only blocks past the 65 535th write differ, in most elements, from the caller's prefill, from zero, and
    (alias) from the lines 65 536 blocks earlier -- what a block index cut to 16 bits would write.  trim: that many last lines
    have no full window (they are 0 by definition) and are left out.  Returns how many blocks lie past the 65 535th."""
    e = np.moveaxis(np.asarray(exp), axis, 0)
    n = e.shape[0]
    over = blocks(n, per_block) - GRID_CAP
    assert over >= 1, f"{what}: {blocks(n, per_block)} blocks do not pass {GRID_CAP}"
    far = e[GRID_CAP * per_block:n - trim]
    assert far.shape[0] >= 1, what
    assert _differ(far, prefill) > 0.5, f"{what}: the far end equals the prefill"
    assert _differ(far, 0) > 0.5, f"{what}: the far end is zero"
    if alias:
        a0 = (GRID_CAP + 1) * per_block
        assert n > a0, f"{what}: no line past block 65 536"
        assert _differ(e[a0:n - trim], e[:n - trim - a0]) > 0.5, f"{what}: the far end equals the lines {a0} earlier"
    return over


# ---- the cells --------------------------------------------------------------------------------------------------------------------
# name: (call, shape, settings): what tests/test_gpu_tall.py runs; `site` names the launch whose block count passes 65 535
# with (extent on that axis, lines per block), None where the cell is there for its row products or its chain alone
CELLS: Dict[str, dict] = {
    "grad-T4x8": dict(shape=(T4, 8), site=("k_gradients grid.y", T4, ROWS_2D)),
    "grad-1xTOP": dict(shape=(1, TOP), site=None),
    "grad-TOPx1": dict(shape=(TOP, 1), site=("k_gradients grid.y", TOP, ROWS_2D)),
    "warp-T4x8": dict(shape=(T4, 8), site=("k_warp grid.y", T4, ROWS_2D)),
    "warp-TOPx2": dict(shape=(TOP, 2), site=("k_warp grid.y", TOP, ROWS_2D)),
    "single5-T4x8": dict(shape=(T4, 8), window=5, site=None),
    "single5-C1x8": dict(shape=(C1, 8), window=5, site=None),
    "single13-T4x16": dict(shape=(T4, 16), window=13, site=("k_lk_generic grid.y", T4, ROWS_2D)),
    "pyr0.5-2T16x8": dict(shape=(2 * T16, 8), levels=2, sf=0.5, plant=2 * GRID_CAP * ROWS_16, site=("k_pyr_down grid.y", T16, ROWS_16)),
    "pyr0.5-TOPx4": dict(shape=(TOP, 4), levels=2, sf=0.5, plant=2 * GRID_CAP * ROWS_16, site=("k_pyr_down grid.y", TOP // 2, ROWS_16)),
    "pyr0.7-T4x8": dict(shape=(T4, 8), levels=2, sf=0.7, site=("k_blur grid.y", T4, ROWS_2D)),
    "up-T16x8": dict(coarse=(T16 // 2, 4), shape=(T16, 8), site=("k_upsample grid.y", T16, ROWS_16)),
    "up-T4x8": dict(coarse=(T4 * 2 // 3, 6), shape=(T4, 8), site=("k_resample<2> grid.y", T4, ROWS_2D)),
    "pyrlk-Cx24": dict(shape=(C, 24), L=3, K=1, site=("k_upsample grid.y", C, ROWS_16)),
    "pyrlk-Cx24-u8": dict(shape=(C, 24), L=3, K=1, u8=True, site=("k_upsample grid.y", C, ROWS_16)),
    "pyrlk-C1x24": dict(shape=(C1, 24), L=3, K=2, site=("k_upsample grid.y", C1, ROWS_16)),
    "pyrlk-T4x8": dict(shape=(T4, 8), L=3, K=3, site=None),
    "pyrlk-TOPx12": dict(shape=(TOP, 12), L=2, K=1, site=("k_upsample grid.y", TOP, ROWS_16)),
    "pyrlk-8xTOP": dict(shape=(8, TOP), L=2, K=1, site=None),
    "seq-Cx24": dict(shape=(C, 24), T=3, L=3, K=1, site=("k_upsample grid.y", C, ROWS_16)),
    "tolerant-C1x24": dict(shape=(C1, 24), L=3, K=2, site=None),   # the upsampling is fused into k_lks there
    "fb-T4x8": dict(shape=(T4, 8), T=2, L=3, K=3, site=("k_fb_check grid.y", T4, ROWS_2D)),
    "interp-T4x8": dict(shape=(T4, 8), site=("k_interp grid.y", T4, ROWS_2D)),
    "interp-T4x1": dict(shape=(T4, 1), site=("k_interp<NARROW> grid.y", T4, ROWS_2D)),
    "interp-packed-T4x8": dict(shape=(T4, 8), site=("k_interp_packed grid.y", T4, ROWS_2D)),
    "interp-nv12-4xNV12_W": dict(shape=(4, NV12_W), site=("k_interp_nv12 grid.y", NV12_W, COLS_NV12)),
}
SHARED = {"pyrlk-Cx24": "seq-Cx24", "tolerant-C1x24": "pyrlk-C1x24"}
INTERP = dict(taus=[1.0 / 3.0], refine=2, status=True)   # test_gpu_interp.py's first config at another tau
INTERP_NV12 = dict(taus=[1.0 / 3.0], refine=1, status=True)   # 16.8 M luma pixels through the NumPy statement: one refinement


@functools.lru_cache(maxsize=None)
def scene(name: str) -> np.ndarray:
    """the frames of a cell, built once: (T, H, W) float32 (uint8 where the cell says so)"""
    c = CELLS[name]
    H, W = c["shape"]
    if name in SHARED:   # the same frames as another cell's: one array, and one oracle run, serve both
        return scene(SHARED[name])[:c.get("T", 2)]
    # plant: the finer level's rows that the far output tile rows of k_pyr_down sample
    f = frames((H, W), T=c.get("T", 2), plant_from=c.get("plant"), u8=c.get("u8", False))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def pyramidal_flows(name: str):
    """the oracle's (u, v) of every consecutive pair of a pyramidal cell's frames, window 5: (T-1, H, W) each"""
    import oflk_oracle as O

    c = CELLS[name]
    if name == "pyrlk-Cx24":
        assert all(CELLS["seq-Cx24"][k] == c[k] for k in ("shape", "L", "K"))
        return tuple(a[:1] for a in pyramidal_flows("seq-Cx24"))
    f = scene(name).astype(np.float32)
    uv = [O.lucas_kanade_pyramidal(f[t], f[t + 1], c["L"], 5, c["K"]) for t in range(len(f) - 1)]
    u, v = np.stack([a for a, _ in uv]), np.stack([b for _, b in uv])
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def backward_flows(name: str):
    import oflk_oracle as O

    c = CELLS[name]
    f = scene(name).astype(np.float32)
    uv = [O.lucas_kanade_pyramidal(f[t + 1], f[t], c["L"], 5, c["K"]) for t in range(len(f) - 1)]
    return np.stack([a for a, _ in uv]), np.stack([b for _, b in uv])


def packed_frames(B: int, H: int, W: int, C_: int) -> np.ndarray:
    """(B+1, H, W, C) uint8: channel c is the texture under another planting row and another map of its values, so that no
    two channels are equal anywhere"""
    ch = [frames((H, W), T=B + 1, plant_from=GRID_CAP * ROWS_2D - 40 * c, u8=True) for c in range(C_)]
    maps = (lambda a: a, lambda a: 255 - a, lambda a: a // 2 + 60, lambda a: 255 - a // 2)
    return np.ascontiguousarray(np.stack([maps[c](a) for c, a in enumerate(ch)], axis=-1))


def nv12_frames(B: int, H: int, W: int) -> np.ndarray:
    """(B+1, 3H/2, W) uint8: the Y plane the wide texture, the interleaved chroma plane the same texture at half height"""
    y = frames((H, W), T=B + 1, plant_from=GRID_CAP * COLS_NV12, u8=True)
    uv = 255 - frames((H // 2, W), T=B + 1, plant_from=GRID_CAP * COLS_NV12 - 100, u8=True)
    return np.ascontiguousarray(np.concatenate([y, uv], axis=1))


# ---- inputs and expected outputs, built once a process and shared by both test files ------------------------------------------
def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """the arrays a cell's call takes besides its settings"""
    c = CELLS[name]
    kind = name.split("-")[0]
    if kind == "warp":
        # flows of up to 1.2 px (2 columns: 0.4) that lean inwards: most points stay inside, about a third of the border's leave
        W = c["shape"][1]
        amp = min(1.2, 0.4 * (W - 1))
        u, v = flow_fields(c["shape"], 1, amp=amp)
        u = (0.7 * u + 0.3 * amp * np.cos(np.pi * np.arange(W) / (W - 1))[None, :]).astype(np.float32)
        return _frozen(scene(name)[0], u, v)
    if kind == "up":
        return _frozen(*flow_fields(c["coarse"], 2))
    if kind == "interp":
        H, W = c["shape"]
        if "nv12" in name:
            return _frozen(nv12_frames(1, H, W), *interp_flows(1, H, W, long_axis=1))
        if "packed" in name:
            return _frozen(packed_frames(1, H, W, 4), *interp_flows(1, H, W))
        return _frozen(scene(name), *interp_flows(1, H, W))
    return scene(name)


@functools.lru_cache(maxsize=None)
def expected(name: str, variant=None):
    """the oracle's (or the NumPy statement's) outputs of a cell, as a tuple of arrays.  variant: "u8" (interp-T4x8: uint8
    frames), 3 or 4 (interp-packed: the channel count), "left" / "center" (interp-nv12: the siting)"""
    import oflk_oracle as O

    c = CELLS[name]
    kind = name.split("-")[0]
    x = inputs(name)
    if kind == "grad":
        return _frozen(*O.compute_gradients(x[0], x[1]))
    if kind == "warp":
        return (_frozen(O.warp_image(*x)),)
    if kind in ("single5", "single13"):
        return _frozen(*O.lucas_kanade_single_scale(x[0], x[1], c["window"]))
    if kind in ("pyr0.5", "pyr0.7"):
        return _frozen(*O.build_gaussian_pyramid(x[0], c["levels"], c["sf"]))
    if kind == "up":
        return _frozen(*O.upsample_flow(x[0], x[1], c["shape"]))
    if kind in ("pyrlk", "seq"):
        return pyramidal_flows(name)
    if kind == "tolerant":
        import oflk_tolerant_model as TM

        f = scene(name)
        u, v, _, runs = TM.pyramidal(f[0], f[1], TM.tolerant_spec(c["L"], c["K"], c["shape"]), 5)
        return _frozen(u, v) + (tuple(int(r) for r in runs),)
    if kind == "fb":
        import fb_model as FM

        uf, vf = pyramidal_flows(name)
        ub, vb = backward_flows(name)
        return (uf, vf, ub, vb) + tuple(FM.fb_check(uf, vf, ub, vb))
    if kind == "interp":
        import interp_colour_model as CM
        import interp_model as M

        fr, flows = x[0], x[1:]
        if "nv12" in name:   # interp_colour_model.interpolate_nv12, with the Y plane (the same for both sitings) solved once
            import nv12_model as NM

            taus, refine = INTERP_NV12["taus"], INTERP_NV12["refine"]
            y, uv = NM.planes(fr)
            new_y, status = expected(name, "luma") if variant != "luma" else M.interpolate(np.ascontiguousarray(y), *flows, taus, refine=refine)
            if variant == "luma":
                return new_y, status
            new_uv = np.stack([CM.chroma_pair(uv[0], uv[1], *(f[0] for f in flows), tau, variant, refine=refine) for tau in taus])
            return NM.from_planes(new_y[0], new_uv)[None], status
        if "packed" in name:
            new, st = expected(name, 4) if variant == 3 else CM.interpolate_packed(fr, *flows, INTERP["taus"], refine=INTERP["refine"])
            return (np.ascontiguousarray(new[..., :3]), st) if variant == 3 else (new, st)
        if variant == "u8":
            fr = np.rint(fr).astype(np.uint8)
        return M.interpolate(fr, *flows, INTERP["taus"], refine=INTERP["refine"])
    raise KeyError(name)


# ---- the conditions on the expected outputs ------------------------------------------------------------------------------------
# Cells whose reference takes tens of seconds on a CPU host.  tests/test_tall_cpu.py asserts the conditions below on every
# other cell, and on crops of these; tests/test_gpu_tall.py asserts them on these cells' full expected outputs, which it has
# to compute anyway, before it compares the device with them.
HEAVY = frozenset({"pyrlk-Cx24", "pyrlk-Cx24-u8", "pyrlk-C1x24", "pyrlk-TOPx12", "pyrlk-8xTOP", "seq-Cx24", "tolerant-C1x24",
                   "interp-nv12-4xNV12_W"})


def full_windows(flow: np.ndarray, wide: bool, hw: int = 2) -> np.ndarray:
    """a flow plane with its long axis first and without the `hw` lines at either side that have no full window (they are 0)"""
    f = flow.T if wide else flow
    return f[:, hw:f.shape[1] - hw]


def check_solves(u: np.ndarray, v: np.ndarray, what: str, last: int = 2000) -> None:
    """u, v from full_windows: finite, and non-zero in most pixels, over the whole plane and in its last lines"""
    for e in (u, v, u[-last:], v[-last:]):
        ok = np.isfinite(e) & (e != 0)
        assert ok.mean() > 0.9, (what, float(ok.mean()))
    assert float(np.abs(u).mean()) > 0.05 and float(np.abs(v).mean()) > 0.05, what


def check_pyramidal(name: str) -> None:
    """the pyramidal scenes solve, the far end of their flows is their own, and at the bound the upper half of the lines does
    not repeat the lower half (what row products formed modulo 2^22 would give)"""
    c = CELLS[name]
    wide = c["shape"][1] > c["shape"][0]
    u, v = expected(name)[:2]
    for t in range(u.shape[0]):
        cu, cv = full_windows(u[t], wide), full_windows(v[t], wide)
        check_solves(cu, cv, f"{name} pair {t}")
        if c["site"]:
            far_end(cu, c["site"][2], PREFILL_F32, f"{name} pair {t} u")
            far_end(cv, c["site"][2], PREFILL_F32, f"{name} pair {t} v")
        if "TOP" in name:
            half = 1 << 22
            for e in (cu, cv):
                assert np.mean(e[half:] != e[:e.shape[0] - half]) > 0.9, name


def check_interp(name: str, variant=None) -> None:
    """frames and status differ at the far end from prefill, zero and (frames) the lines 65 536 blocks earlier; the flows are
    not trivial there: points leave the frame (status 0) and pass (status 3), and NaN, +-inf and 1e30 are planted"""
    x = inputs(name)
    new, status = expected(name, variant)
    axis, per = (3, COLS_NV12) if "nv12" in name else (2, ROWS_2D)
    far_end(new, per, PREFILL_U8, f"{name} {variant}: frames", axis=axis)
    far = np.moveaxis(status, axis, 0)[GRID_CAP * per:]
    assert _differ(far, PREFILL_STATUS) == 1.0 and {0, 3} <= set(np.unique(far).tolist()), np.unique(far)
    assert set(np.unique(status).tolist()) == {0, 1, 2, 3} or x[0].shape[-1] == 1
    # not a comparison of fallbacks: most pixels pass on both sides.  On the border lines of the short axis a side passes
    # only where the flow is tangent to the border (its start p = x - s F and its target p + F lie on opposite sides of the
    # line), so both fail there; a frame of 4 rows has half its pixels on such lines and is asked for its inner lines
    share3 = float((status == 3).mean())
    if 2 < min(status.shape[2:]) <= 4:
        inner = np.moveaxis(status, 5 - axis, 0)[1:-1]
        assert float((inner == 3).mean()) > 0.5, (share3, float((inner == 3).mean()))
    else:
        assert share3 > 0.5, share3
    check_planted(x[1:], axis - 1, per)


def check_planted(flows, axis: int, per: int) -> None:
    for f in flows:
        tail = np.moveaxis(f, axis, 0)[GRID_CAP * per:]
        assert np.isnan(tail).any() and np.isposinf(tail).any() and np.isneginf(tail).any() and (np.abs(tail) == np.float32(1e30)).any()
        assert (np.abs(tail[np.isfinite(tail)]) > max(f.shape[1:])).any() or (np.abs(tail[np.isfinite(tail)]) > 4).any()   # wild


def check_tolerant(name: str = "tolerant-C1x24") -> None:
    """the model's flows solve and are not the oracle's: the comparison sees the tolerant arithmetic"""
    assert SHARED[name] == "pyrlk-C1x24" and all(CELLS[name][k] == CELLS["pyrlk-C1x24"][k] for k in ("shape", "L", "K"))
    mu, mv, runs = expected(name)
    ou, _ = expected("pyrlk-C1x24")
    check_solves(full_windows(mu, False), full_windows(mv, False), name)
    assert np.mean(mu != ou[0]) > 0.1 and len(runs) == CELLS[name]["L"]
