"""k_pyr_down's two tile geometries: the tight one (a 32 x 16 output tile blurs the 32 x 64 values a
half-scale step samples) and the general one (34 x 66: odd sizes, tiny levels).  Which one a step takes is asked of the
library (oflk_pyramid_step_form); whichever it is, the pyramid equals the CPU oracle's value for value, through
oflk_build_pyramid and through a plan, on float32 and uint8 frames, on frames that send most waves to the certificate's
exact redo (isolated dots) and on an all-black frame (the M == 0 exit).

Shapes: 64 x 96 (rows: two full tiles; columns: one full and a half tile) and 70 x 100 (a partial last tile row and
column) are tight, every border tile is staged with one mirror step; 64 x 67 and 33 x 64 need 33 values on one axis and
must run the general form; 64 x 96 at a scale factor of 0.4 lies away from the half-scale ratio and keeps the unfused
chain."""
import numpy as np
import pytest

import pyr_cert_model as C

pytestmark = pytest.mark.gpu

UNFUSED, GENERAL, TIGHT = 0, 1, 2
TIGHT_SHAPES = [(64, 96), (70, 100)]
GENERAL_SHAPES = [(64, 67), (33, 64)]
_frames = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = C.frames(*shape)
    return _frames[shape]


def step_forms(shape, levels, sf=0.5):
    """the form of every step of a pyramid, finest first"""
    import _oflk

    L = _oflk.lib()
    forms, (h, w) = [], shape
    for _ in range(levels - 1):
        ho, wo = int(h * sf), int(w * sf)
        forms.append(L.oflk_pyramid_step_form(h, w, ho, wo, 8))
        h, w = ho, wo
    return forms


def assert_pyramid_equals_oracle(oracle, f, levels, sf, what):
    import lucas_kanade_pyramidal as P

    got = P.build_gaussian_pyramid(f, levels, sf)
    exp = oracle.build_gaussian_pyramid(f, levels, sf)
    assert len(got) == len(exp) == levels
    for lvl, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and g.dtype == e.dtype == np.float32
        same = (g + np.float32(0.0)).tobytes() == (e + np.float32(0.0)).tobytes()
        assert same, (what, lvl, int(np.count_nonzero(g != e)))


def plan_flows(prev, curr, arith=0, u8=False):
    import torch

    import _oflk

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    p, c = np.stack(prev), np.stack(curr)
    B, H, W = p.shape
    if u8:
        p, c = p.astype(np.uint8), c.astype(np.uint8)
    tp, tc = torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev)
    u = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    v = torch.empty_like(u)
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    try:
        plan.set_arithmetic(arith)
        (plan.pyramidal_u8 if u8 else plan.pyramidal)(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
        plan.resolve_uncertain(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st, u8=u8)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return u.cpu().numpy(), v.cpu().numpy()


def test_the_shapes_take_the_forms_they_are_here_for():
    assert step_forms((64, 96), 3) == [TIGHT, TIGHT]
    assert step_forms((70, 100), 3)[0] == TIGHT and UNFUSED not in step_forms((70, 100), 3)
    for shape in GENERAL_SHAPES:
        assert step_forms(shape, 3)[0] == GENERAL and UNFUSED not in step_forms(shape, 3), shape
    assert step_forms((64, 96), 2, 0.4) == [UNFUSED]


@pytest.mark.parametrize("shape", TIGHT_SHAPES + GENERAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_equals_the_oracle(oracle, shape):
    """every frame kind of the certificate's test, the dots (redo in most waves) and the all-black frame among them"""
    fr = frames(shape)
    assert {"dots", "zeros", "adversarial", "huge", "tiny"} <= set(fr)
    assert set(np.unique(fr["dots"][0])) == {0.0, 255.0} and not fr["zeros"][0].any()
    for name, (f, _) in fr.items():
        assert_pyramid_equals_oracle(oracle, f, 3, 0.5, (name, shape))


def test_unfused_shape_still_equals_the_oracle(oracle):
    for name in ("smooth", "dots", "normal100"):
        assert_pyramid_equals_oracle(oracle, frames((64, 96))[name][0], 2, 0.4, name)


@pytest.fixture(scope="module")
def batch():
    """three pairs of 8-bit frames per tight shape, and the oracle's flows for them"""
    out = {}
    for shape in TIGHT_SHAPES:
        fr = frames(shape)
        prev = [fr[n][0] for n in ("smooth", "noise", "dots")]
        curr = [np.roll(f, (1, 2), axis=(0, 1)) for f in prev]
        out[shape] = (prev, curr)
    return out


@pytest.fixture(scope="module")
def oracle_flows(oracle, batch):
    return {shape: [oracle.lucas_kanade_pyramidal_ex(p, c, 3, 5, 3)[:2] for p, c in zip(prev, curr)]
            for shape, (prev, curr) in batch.items()}


@pytest.mark.parametrize("u8", [False, True], ids=["float32", "uint8"])
@pytest.mark.parametrize("shape", TIGHT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_batch_of_three_gives_the_oracle_flow(batch, oracle_flows, shape, u8):
    """a plan call of 3 pairs: its first pyramid launch reads two caller buffers (in2 / nsplit) and carries the call's
    zeroing, in the tight form; the flow built on that pyramid is the oracle's"""
    prev, curr = batch[shape]
    u, v = plan_flows(prev, curr, u8=u8)
    for i, (ou, ov) in enumerate(oracle_flows[shape]):
        assert np.array_equal(u[i], ou) and np.array_equal(v[i], ov), (shape, i, int(np.count_nonzero(u[i] != ou)))


def test_black_and_dot_frames_as_uint8_give_the_float32_flow():
    fr = frames((70, 100))
    prev = [fr[n][0] for n in ("zeros", "dots", "checker")]
    curr = [np.roll(f, (1, 2), axis=(0, 1)) for f in prev]
    uf, vf = plan_flows(prev, curr)
    u8, v8 = plan_flows(prev, curr, u8=True)
    assert uf.tobytes() == u8.tobytes() and vf.tobytes() == v8.tobytes()


def test_contracted_arithmetic_leaves_zero_values_differing(batch):
    """the opt-in contracted pyramid in the tight form against the exact one: 0 flow values differ on these frames (it
    moves about one pyramid value in 10^7)"""
    prev, curr = batch[(64, 96)]
    u0, v0 = plan_flows(prev, curr, 0)
    u1, v1 = plan_flows(prev, curr, 1)
    differing = int(np.count_nonzero(u0 != u1) + np.count_nonzero(v0 != v1))
    print(f"flow values differing, contracted against exact: {differing} of {2 * u0.size}")
    assert differing == 0
