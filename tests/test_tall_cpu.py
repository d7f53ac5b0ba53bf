"""CPU tests of the tall and wide cells (tests/tall_scenes.py): no GPU is used.

1. The threshold arithmetic of every cell: which launch site's block count passes 65 535, and by how much; launch_lk's
   cap and segment table for every level of the chained cells.
2. The far-end conditions: in the expected output of every cell whose site passes 65 535 blocks, the lines that only those
   blocks write differ from the caller's prefill, from zero and from the lines 65 536 blocks earlier.
3. Every shape passes the library's own entry checks (never-dereferenced pointers; asked only where no device is usable,
   as tests/test_stages_cpu.py does), and the next size up, 2^23, is refused.
4. The pyramidal scenes solve: the far-end flow is non-zero and finite in most pixels; at the bound the oracle's flows in
   the upper half of the rows (columns) differ from those 2^22 earlier.

The references of the cells in tall_scenes.HEAVY (the C, C1 and bound passes, the NV12 statement) take tens of seconds each on
a CPU host.  For those, 2 and 4 are asserted here on crops of the far end and of the lines it could be confused with, and
on the full expected outputs in tests/test_gpu_tall.py, which computes them anyway (tall_scenes.check_pyramidal,
check_interp, check_tolerant).  Every other oracle run of this file is the one tests/test_gpu_tall.py compares with:
tall_scenes caches them for the process.
"""
import ctypes

import numpy as np
import pytest

import tall_scenes as S


@pytest.fixture(scope="module")
def L():
    import _oflk

    return _oflk.lib()


# ---- 1. thresholds -------------------------------------------------------------------------------------------------------------
def test_base_heights_sit_where_the_issue_puts_them():
    assert S.blocks(S.T4, S.ROWS_2D) == 65538 and S.blocks(S.T16, S.ROWS_16) == 65538
    assert S.C == 65535 * S.K5TY and S.blocks(S.C, S.K5TY) == 65535 and S.blocks(S.C1, S.K5TY) == 65537
    assert S.TOP == (1 << 23) - 1 and S.blocks(S.NV12_W, S.COLS_NV12) == 65537
    assert S.blocks(4320, S.K5TY) == 180 and S.lk_cap(64, 4320, 7680) == 9   # the tallest frame of the older tests
    for name, c in S.CELLS.items():
        H, W = c["shape"]
        assert 1 <= H < S.MAX_DIM and 1 <= W < S.MAX_DIM and H * W < S.MAX_PIXELS, name
        if name.split("-")[0] in ("single5", "single13", "pyrlk", "seq", "tolerant"):   # plans
            assert H * W < S.MAX_PLAN_PIXELS, name


# blocks on the site's axis of every cell that has one
SITE_BLOCKS = {
    "grad-T4x8": 65538, "grad-TOPx1": 2097152, "warp-T4x8": 65538, "warp-TOPx2": 2097152, "single13-T4x16": 65538,
    "pyr0.5-2T16x8": 65538, "pyr0.5-TOPx4": 262144, "pyr0.7-T4x8": 65538, "up-T16x8": 65538, "up-T4x8": 65538,
    "pyrlk-Cx24": 98303, "pyrlk-Cx24-u8": 98303, "pyrlk-C1x24": 98306, "pyrlk-TOPx12": 524288, "seq-Cx24": 98303,
    "fb-T4x8": 65538, "interp-T4x8": 65538, "interp-T4x1": 65538, "interp-packed-T4x8": 65538, "interp-nv12-4xNV12_W": 65537,
}


def test_every_site_passes_the_grid_cap_by_the_stated_count():
    assert set(SITE_BLOCKS) == {n for n, c in S.CELLS.items() if c["site"]}
    for name, n in SITE_BLOCKS.items():
        _, extent, per = S.CELLS[name]["site"]
        assert S.blocks(extent, per) == n > S.GRID_CAP, (name, S.blocks(extent, per))
    # every level of the bound cell's pass: k_pyr_down and k_upsample at 16 rows, the 4-row launches of the exact redo
    assert S.level_shapes((S.TOP, 12), 2) == [(8388607, 12), (4194303, 6)]
    # the degenerate levels of the T4 x 8 pass (W <= 4: no full window): one block per 256 pixels on grid.x
    assert [S.blocks(h * w, 256) for h, w in S.level_shapes((S.T4, 8), 3)[1:]] == [2049, 513]


def test_upsample_cells_reach_their_kernels(L):
    c = S.CELLS["up-T16x8"]
    assert L.oflk_upsample_staged(*c["coarse"], *c["shape"]) == 1
    c = S.CELLS["up-T4x8"]
    assert c["coarse"] == (174768, 6) and L.oflk_upsample_staged(*c["coarse"], *c["shape"]) == 0
    assert L.oflk_pyramid_step_fused(2 * S.T16, 8, S.T16, 4, 8) == 1 and L.oflk_pyramid_step_fused(S.TOP, 4, S.TOP // 2, 2, 8) == 1
    assert L.oflk_pyramid_step_fused(S.T4, 8, int(S.T4 * 0.7), 5, 6) == 0


# launch_lk's cap per level, finest first
CAPS = {"pyrlk-Cx24": [3277, 1639, 820], "pyrlk-C1x24": [1, 1639, 820], "seq-Cx24": [3277, 1639, 820]}


@pytest.mark.parametrize("name", sorted(CAPS))
def test_chained_cells_run_k_lkw_at_every_level_with_the_stated_caps(name):
    c = S.CELLS[name]
    B = c.get("T", 2) - 1
    shapes = S.level_shapes(c["shape"], c["L"])
    assert all(w > 4 and h > 4 for h, w in shapes), shapes   # wider than 2 hw: no degenerate level
    assert [S.lk_cap(B, h, w) for h, w in shapes] == CAPS[name]
    for (h, w), cap in zip(shapes, CAPS[name]):
        if cap > 1:
            seg = S.lk_segments(h, cap)
            assert seg[-1] == S.blocks(h, S.K5TY) <= 65535 and len(seg) - 1 <= S.MAX_SEGS
            assert all(b - a <= cap for a, b in zip(seg, seg[1:])) and seg[1] - seg[0] == cap > 1024 * (h >= S.C // 2)


def test_the_longest_chain_and_the_segment_table():
    """at C the table's last entry is 65 535, the last value an unsigned short holds; one tile row more unchains.  The
    cap keeps the table to 20 full segments and a halving tail of at most log2(2 cap) more, so the `n == kMaxSegs - 1`
    tail of launch_lk is not reached at any height the table is used for."""
    seg = S.lk_segments(S.C, S.lk_cap(1, S.C, 24))
    assert seg[-1] == 65535 and len(seg) - 1 == 32
    assert S.lk_cap(1, S.C + 1, 24) == 1 and S.lk_cap(1, S.C1, 24) == 1
    longest = max(len(S.lk_segments(ty * 24, cap)) - 1 for ty in range(1, 65536, 7) for cap in [S.lk_cap(1, ty * 24, 24)] if cap > 1)
    assert longest == 32 < S.MAX_SEGS - 1, longest
    assert S.lk_cap(1, S.T4, 8) == 547 and S.lk_cap(1, S.C1, 8) == 1   # the single-scale cells


# ---- 2. far-end conditions --------------------------------------------------------------------------------------------------------
def _site(name):
    return S.CELLS[name]["site"][2]


@pytest.mark.parametrize("name", ["grad-T4x8", "grad-TOPx1", "warp-T4x8", "warp-TOPx2", "single13-T4x16", "up-T16x8", "up-T4x8"])
def test_far_end_of_the_per_pixel_cells(name):
    exp = S.expected(name)
    if name == "grad-TOPx1":
        exp = exp[1:]     # one column has no x gradient
    if name == "single13-T4x16":
        exp = [S.full_windows(e, False, 6) for e in exp]
    for k, e in enumerate(exp):
        S.far_end(e, _site(name), S.PREFILL_F32, f"{name} output {k}", trim=6 if name == "single13-T4x16" else 0)


@pytest.mark.parametrize("name", ["pyr0.5-2T16x8", "pyr0.5-TOPx4"])
def test_far_end_of_the_fused_pyramid_cells(name):
    exp = S.expected(name)
    assert exp[0].shape[0] == S.CELLS[name]["site"][1] and exp[1].shape == S.CELLS[name]["shape"]
    S.far_end(exp[0], S.ROWS_16, S.PREFILL_F32, name)


def test_far_end_of_the_unfused_pyramid_cell():
    """k_blur's far blocks write blurred rows from 262 140 on; the output rows that sample them are the last five"""
    coarse = S.expected("pyr0.7-T4x8")[0]
    ho = coarse.shape[0]
    assert ho == int(S.T4 * 0.7) and (ho - 5) * (S.T4 - 1) / (ho - 1) + 1 >= S.GRID_CAP * S.ROWS_2D
    assert (coarse[-5:] != 0).all() and not np.array_equal(coarse[-5:], coarse[:5])


@pytest.mark.parametrize("name", ["pyrlk-T4x8"])
def test_pyramidal_scenes_solve(name):
    assert name not in S.HEAVY
    S.check_pyramidal(name)


@pytest.mark.parametrize("name", sorted(n for n in S.HEAVY if n.split("-")[0] in ("pyrlk", "seq", "tolerant")))
def test_heavy_pyramidal_scenes_solve_at_their_far_end(oracle, name):
    """the oracle on the last 3 072 lines of the scene and, where a 16-row launch passes 65 535 blocks, on the 3 072 lines
    65 536 x 16 earlier: the far end solves, and its flow is not the earlier lines' (the full-frame conditions of
    tall_scenes.check_pyramidal run in tests/test_gpu_tall.py, where the full reference is computed anyway)"""
    c = S.CELLS[name]
    wide = c["shape"][1] > c["shape"][0]
    n = max(c["shape"])

    def flows(last):
        f = S.frames(c["shape"], T=2, u8=c.get("u8", False), rows=(last - 3072, last)).astype(np.float32)
        u, v = oracle.lucas_kanade_pyramidal(f[0], f[1], c["L"], 5, c["K"])
        return S.full_windows(u, wide)[1024:], S.full_windows(v, wide)[1024:]   # away from the crop's own upper border

    fu, fv = flows(n)
    S.check_solves(fu, fv, name)
    if c["site"]:
        au, av = flows(n - (S.GRID_CAP + 1) * c["site"][2])
        assert np.mean(fu != au) > 0.9 and np.mean(fv != av) > 0.9
    if "TOP" in name:
        au, av = flows(n - (1 << 22))
        assert np.mean(fu != au) > 0.9 and np.mean(fv != av) > 0.9


def test_far_end_of_the_fb_cell():
    want = S.expected("fb-T4x8")
    for k in range(6):
        S.far_end(S.full_windows(want[k][0], False), S.ROWS_2D, S.PREFILL_F32, f"fb output {k}")
    for k in (6, 7):   # valid: most vectors pass at both ends, so the far end differs from zero, not from the near end
        S.far_end(want[k][0], S.ROWS_2D, S.PREFILL_STATUS, f"fb output {k}", alias=False)
        assert 0.5 < want[k].mean() < 1.0


@pytest.mark.parametrize("name,variant", [("interp-T4x8", None), ("interp-T4x8", "u8"), ("interp-T4x1", None),
                                          ("interp-packed-T4x8", 4), ("interp-packed-T4x8", 3)])
def test_far_end_of_the_interpolation_cells(name, variant):
    assert name not in S.HEAVY
    S.check_interp(name, variant)


def test_nv12_flows_are_not_trivial_at_the_far_end():
    """(the conditions on the NV12 cell's expected frames run in tests/test_gpu_tall.py: its NumPy statement takes tens of
    seconds)"""
    H, W = S.CELLS["interp-nv12-4xNV12_W"]["shape"]
    S.check_planted(S.interp_flows(1, H, W, long_axis=1), 2, S.COLS_NV12)


# ---- 3. the entry checks ----------------------------------------------------------------------------------------------------------
def test_every_shape_passes_the_entry_checks_and_2_to_the_23_does_not(L):
    import _oflk

    f32p, UNS, NODEV = ctypes.POINTER(ctypes.c_float), _oflk.OFLK_ERR_UNSUPPORTED, _oflk.OFLK_ERR_NO_DEVICE
    buf = ctypes.cast(ctypes.c_void_p(1 << 20), f32p)   # never dereferenced: each call below ends in its checks
    vbuf = ctypes.c_void_p(1 << 20)
    out, vout = ctypes.cast(ctypes.c_void_p(1 << 44), f32p), ctypes.c_void_p(1 << 44)   # far from buf: not an overlap
    taus = (ctypes.c_double * 1)(0.5)
    levels = (f32p * 2)(buf, buf)

    def call(name, H, W):
        c = S.CELLS[name]
        kind = name.split("-")[0]
        if kind == "grad":
            return L.oflk_compute_gradients(buf, buf, H, W, buf, buf, buf)
        if kind == "warp":
            return L.oflk_warp(buf, buf, buf, H, W, buf)
        if kind in ("single5", "single13"):
            return L.oflk_single_scale(buf, buf, H, W, c["window"], buf, buf)
        if kind in ("pyr0.5", "pyr0.7"):
            return L.oflk_build_pyramid(buf, H, W, 2, c["sf"], levels)
        if kind == "up":
            return L.oflk_upsample_flow(buf, buf, max(H * c["coarse"][0] // c["shape"][0], 1), max(W * c["coarse"][1] // c["shape"][1], 1),
                                        H, W, buf, buf)
        if kind in ("pyrlk", "tolerant", "seq"):
            h = ctypes.c_void_p()
            rc = L.oflk_plan_create(ctypes.byref(h), 0, c.get("T", 2) - 1, H, W, c["L"], 5, c["K"])
            assert not h.value
            return rc
        if kind == "fb":
            return L.oflk_pyramidal_sequence_fb(buf, 2, H, W, c["L"], 5, c["K"], 0.01, 0.5, *([buf] * 6), vbuf, vbuf)
        if "nv12" in name:
            return L.oflk_interpolate_frames_nv12_host(vbuf, 1, H, W, 0, buf, buf, buf, buf, 0.01, 0.5, 2, taus, 1, vout, vbuf)
        if "packed" in name:
            return L.oflk_interpolate_frames_packed_host(vbuf, 1, H, W, 4, buf, buf, buf, buf, 0.01, 0.5, 2, taus, 1, vout, vbuf)
        return L.oflk_interpolate_frames_host(buf, 1, H, W, buf, buf, buf, buf, 0.01, 0.5, 2, taus, 1, out, vbuf)

    for name, c in S.CELLS.items():
        H, W = c["shape"]
        # the next size up along the long axis is refused, with or without a device, before any pointer is read
        big = (H, 1 << 23) if W > H else (1 << 23, W)
        rc = call(name, *big)
        assert rc == UNS, (name, big, rc, L.oflk_last_error())
        # the shape itself passes every check.  Only where no device is usable is that safe to ask: the call then ends in
        # OFLK_ERR_NO_DEVICE before it reads a pointer
        if _oflk.device_count() == 0:
            rc = call(name, H, W)
            assert rc == NODEV, (name, (H, W), rc, L.oflk_last_error())
