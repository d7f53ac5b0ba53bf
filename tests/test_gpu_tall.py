"""The frame calls at the tallest and widest shapes they accept, against the oracle or the call's NumPy statement, every
element: NaN at the same positions, every other value the same bits (run on an MI355X:
python -m pytest tests/test_gpu_tall.py -m gpu -q).

tests/tall_scenes.py holds the shapes and what each reaches; tests/test_tall_cpu.py asserts the thresholds, that the rows
(columns) which only the blocks past the 65 535th write differ from the prefill, from zero and from the rows 65 536 blocks
earlier, and that the pyramidal scenes solve.  For the cells of tall_scenes.HEAVY, whose reference takes tens of seconds, it
does so on crops, and the same conditions on the full expected outputs are asserted here (tall_scenes.check_*), where those
outputs are computed anyway.  The cheap per-pixel cells come first in this file, the pyramidal passes last.  Device forms
run on outputs prefilled with a sentinel.

Measured on an MI355X host (the CPU reference is most of every figure): DESIGN.md, "Frames at the accepted bound".
"""
import numpy as np
import pytest

import stage_scenes as SS
import tall_scenes as S
from test_gpu_fb import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import lucas_kanade_pyramidal

    return lucas_kanade_pyramidal


@pytest.fixture(scope="module")
def K():
    import lucas_kanade_core

    return lucas_kanade_core


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))   # a copy: the cells' arrays are read-only


def _prefilled(shape):
    import torch

    return torch.full(shape, S.PREFILL_F32, dtype=torch.float32, device=torch.device("cuda", 0))


def _plan_flows(frames, L, window, K_, single=False, kernels=None, arith=None, sequence=False):
    """(u, v), each (B, H, W), of a plan's device form on prefilled outputs; a pyramidal pass is followed by the redo of the
    pairs whose exit decisions were flagged, as the host forms do"""
    import torch

    import _oflk

    T, H, W = frames.shape
    B = T - 1
    u8 = frames.dtype == np.uint8
    st = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, B, H, W, L, window, K_)
    try:
        if kernels is not None:
            plan.set_kernels(kernels)
        if arith is not None:
            plan.set_arithmetic(arith)
        d_f = _dev(frames)
        step = H * W * frames.dtype.itemsize
        u, v = _prefilled((B, H, W)), _prefilled((B, H, W))
        if single:
            (plan.single_scale_u8 if u8 else plan.single_scale)(d_f.data_ptr(), d_f.data_ptr() + step, u.data_ptr(), v.data_ptr(), st)
        elif sequence:
            plan.pyramidal_sequence(d_f.data_ptr(), u.data_ptr(), v.data_ptr(), st, u8=u8)
        else:
            (plan.pyramidal_u8 if u8 else plan.pyramidal)(d_f.data_ptr(), d_f.data_ptr() + step, u.data_ptr(), v.data_ptr(), st)
        if not single and arith is None:
            plan.resolve_uncertain(d_f.data_ptr(), d_f.data_ptr() + step, u.data_ptr(), v.data_ptr(), st, u8=u8)
        runs = None if single else plan.read_log(st)[1]
        torch.cuda.synchronize()
        return u.cpu().numpy(), v.cpu().numpy(), runs
    finally:
        plan.close()


# ---- cells 1, 2: gradients and the warp --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grad-T4x8", "grad-1xTOP", "grad-TOPx1"])
def test_compute_gradients(K, name):
    p, c = S.inputs(name)
    for g, e, what in zip(K.compute_gradients(p, c), S.expected(name), ("Ix", "Iy", "It")):
        SS.same_bits(g, e, f"{name}: {what}")


@pytest.mark.parametrize("name", ["warp-T4x8", "warp-TOPx2"])
def test_warp_image(P, name):
    img, u, v = S.inputs(name)
    SS.same_bits(P.warp_image(img, u, v), S.expected(name)[0], name)


# ---- cells 5 to 8: the pyramid and the flow upsampling ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pyr0.5-2T16x8", "pyr0.5-TOPx4", "pyr0.7-T4x8"])
def test_build_gaussian_pyramid(P, name):
    c = S.CELLS[name]
    got, exp = P.build_gaussian_pyramid(S.inputs(name)[0], c["levels"], c["sf"]), S.expected(name)
    assert len(got) == len(exp)
    for l, (g, e) in enumerate(zip(got, exp)):
        SS.same_bits(g, e, f"{name}: level {l} {e.shape}")


@pytest.mark.parametrize("name", ["up-T16x8", "up-T4x8"])
def test_upsample_flow(P, name):
    u, v = S.inputs(name)
    gu, gv = P.upsample_flow(u, v, S.CELLS[name]["shape"])
    eu, ev = S.expected(name)
    SS.same_bits(gu, eu, f"{name}: u")
    SS.same_bits(gv, ev, f"{name}: v")


# ---- cells 16 to 19: frame interpolation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, "u8"], ids=["f32", "u8"])
def test_interpolate_frames(variant):
    from test_gpu_interp import _device

    name = "interp-T4x8"
    x = S.inputs(name)
    fr = np.rint(x[0]).astype(np.uint8) if variant == "u8" else x[0]
    want = S.expected(name, variant)
    got = _device(np.array(fr), [np.array(f) for f in x[1:]], S.INTERP["taus"], refine=S.INTERP["refine"])
    _same(got[0], want[0], f"{name} {variant}: frames")
    _same(got[1], want[1], f"{name} {variant}: status")


def test_interpolate_frames_narrow():
    from test_gpu_interp import _device

    name = "interp-T4x1"
    x = S.inputs(name)
    want = S.expected(name)
    got = _device(np.array(x[0]), [np.array(f) for f in x[1:]], S.INTERP["taus"], refine=S.INTERP["refine"])
    _same(got[0], want[0], f"{name}: frames")
    _same(got[1], want[1], f"{name}: status")


@pytest.mark.parametrize("channels", [3, 4])
def test_interpolate_frames_packed(channels):
    from test_gpu_interp_colour import _device_layout

    name = "interp-packed-T4x8"
    x = S.inputs(name)
    fr = np.array(x[0][..., :channels], order="C")
    want = S.expected(name, channels)
    got = _device_layout("packed", channels, fr, [np.array(f) for f in x[1:]], S.INTERP["taus"], refine=S.INTERP["refine"])
    _same(got[0], want[0], f"{name} C={channels}: frames")
    _same(got[1], want[1], f"{name} C={channels}: status")


@pytest.mark.parametrize("siting", ["left", "center"])
def test_interpolate_frames_nv12(siting):
    import nv12_model as NM
    from test_gpu_interp_colour import _device_layout

    name = "interp-nv12-4xNV12_W"
    x = S.inputs(name)
    want = S.expected(name, siting)
    S.check_interp(name, siting)
    got = _device_layout("nv12", NM.SITING_CODES[siting], np.array(x[0]), [np.array(f) for f in x[1:]], S.INTERP_NV12["taus"], refine=S.INTERP_NV12["refine"])
    _same(got[0], want[0], f"{name} {siting}: frames")
    _same(got[1], want[1], f"{name} {siting}: status")


# ---- cells 3, 4: single-scale ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single5-T4x8", "single5-C1x8", "single13-T4x16"])
def test_single_scale(name):
    """window 5 through both of a plan's kernel choices: the tile kernel k_lkw throughout (T4: chains of 547 tile rows; C1:
    65 537 tile rows, one tile a block), and the automatic choice, which at these heights streams (k_lks) and redoes the
    doubtful tiles with k_lkw"""
    c = S.CELLS[name]
    eu, ev = S.expected(name)
    choices = (1, 0) if c["window"] == 5 else (0,)   # OFLK_KERNELS_TILE, OFLK_KERNELS_AUTO
    for choice in choices:
        u, v, _ = _plan_flows(S.inputs(name), 1, c["window"], 0, single=True, kernels=choice)
        SS.same_bits(u[0], eu, f"{name}, kernels {choice}: u")
        SS.same_bits(v[0], ev, f"{name}, kernels {choice}: v")


# ---- cell 15: both directions and their consistency ------------------------------------------------------------------------------
def test_sequence_fb(P):
    name = "fb-T4x8"
    c = S.CELLS[name]
    r = P.lucas_kanade_pyramidal_sequence_fb(S.inputs(name), c["L"], 5, c["K"])
    want = S.expected(name)
    for g, e, what in zip(r[:6], want[:6], ("u_fwd", "v_fwd", "u_bwd", "v_bwd", "err_fwd", "err_bwd")):
        SS.same_bits(g, e, f"{name}: {what}")
    _same(r.valid_fwd.astype(np.uint8), want[6], f"{name}: valid_fwd")
    _same(r.valid_bwd.astype(np.uint8), want[7], f"{name}: valid_bwd")


# ---- cells 9 to 13: the pyramidal pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pyrlk-T4x8", "pyrlk-Cx24", "pyrlk-Cx24-u8", "pyrlk-C1x24", "pyrlk-TOPx12", "pyrlk-8xTOP"])
def test_pyramidal(name):
    c = S.CELLS[name]
    eu, ev = S.expected(name)
    S.check_pyramidal(name)
    u, v, _ = _plan_flows(S.inputs(name), c["L"], 5, c["K"])
    SS.same_bits(u[0], eu[0], f"{name}: u")
    SS.same_bits(v[0], ev[0], f"{name}: v")


def test_pyramidal_sequence():
    name = "seq-Cx24"
    c = S.CELLS[name]
    eu, ev = S.expected(name)
    S.check_pyramidal(name)
    u, v, _ = _plan_flows(S.inputs(name), c["L"], 5, c["K"], sequence=True)
    SS.same_bits(u, eu, f"{name}: u")
    SS.same_bits(v, ev, f"{name}: v")


# ---- cell 14: the tolerant arithmetic --------------------------------------------------------------------------------------------
def test_tolerant_arithmetic(P):
    """a tolerant plan (prefilled outputs, no redo) equals its CPU model; the host form under oflk_set_host_arithmetic(2)
    equals the model too unless it redid the pair exactly (oflk_last_resolved), when it equals the oracle"""
    import _oflk

    name = "tolerant-C1x24"
    c = S.CELLS[name]
    f = S.inputs(name)
    mu, mv, mruns = S.expected(name)
    S.check_tolerant(name)
    u, v, runs = _plan_flows(f, c["L"], 5, c["K"], arith=2)
    assert tuple(int(r) for r in runs[0]) == mruns, (runs, mruns)
    SS.same_bits(u[0], mu, f"{name}: plan u")
    SS.same_bits(v[0], mv, f"{name}: plan v")
    _oflk.check(_oflk.lib().oflk_set_host_arithmetic(2))
    try:
        hu, hv = P.lucas_kanade_pyramidal(f[0], f[1], c["L"], 5, c["K"])
        redone = int(_oflk.lib().oflk_last_resolved())
    finally:
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
    if redone:
        import oflk_oracle as O

        mu, mv = O.lucas_kanade_pyramidal(f[0], f[1], c["L"], 5, c["K"])
    SS.same_bits(hu, mu, f"{name}: host u (redone exactly: {redone})")
    SS.same_bits(hv, mv, f"{name}: host v (redone exactly: {redone})")
