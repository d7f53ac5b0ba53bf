"""k_pyr_down's half-scale instantiation: where oflk_pyramid_step_half holds, stage A stages fixed
rows per thread and stage D reads its taps at compile-time offsets; the values are the tight tile's.  The pyramid is held
to the CPU oracle's value for value, as in tests/test_gpu_pyr_tight.py, on the smallest shapes that reach every path:

  96 x 200, 3 levels  interior tiles (tile row i0 = 16: source rows 24 .. 71; tile columns j0 = 32, 64: source columns
                      56 .. 135 and 120 .. 199), border tiles on every side, a partial last tile column (4 of 32 outputs);
                      96 -> 48 -> 24 and 200 -> 100 -> 50 are both half scale
  64 x 96, 3 levels   every tile a border tile, one partial tile per step
  34 x 36, 2 levels   the smallest tight size: one partial tile, which holds the first and the last row and column
  33 x 33, 65 x 65 at scale factor 0.52 (-> 17, 33 per axis): S = 2 T - 1, a linspace step of exactly 2, the last point at
                      2 (T - 1); at 65 the last tile row and column hold that one output alone
  a tight step off the half-scale ratio (pyr_half_scenes.tight_but_not_half) keeps the tight tile's code

Frames: seeded float32 noise with negative values, a 1e6 : 1 dynamic range inside every tile (the certificate's redo), all
zeros, isolated dots; 8-bit frames as float32 and as uint8 through a plan with a batch of three (two caller buffers in the
first launch, blockIdx.z), for the exact, the contracted and the tolerant plan arithmetic."""
import numpy as np
import pytest

import pyr_cert_model as C
import pyr_half_scenes as S

pytestmark = pytest.mark.gpu

HALF_SHAPES = [((96, 200), 3), ((64, 96), 3), ((34, 36), 2)]
_ids = lambda sl: f"{sl[0][0]}x{sl[0][1]}"


def lib():
    import _oflk

    return _oflk.lib()


def pyramid_frames(shape):
    H, W = shape
    rng = np.random.default_rng(H * 4096 + W)
    wide = rng.uniform(1.0, 2.0, shape).astype(np.float32)
    wide[3::7, 2::11] *= np.float32(1e6)   # within every window of 17: values 1e6 times their neighbours
    return {
        "random": (rng.standard_normal(shape) * 100.0).astype(np.float32),
        "range1e6": wide,
        "zeros": np.zeros(shape, np.float32),
        "dots": C.dots(H, W),
        "noise8": rng.integers(0, 256, shape).astype(np.float32),
    }


def assert_pyramid_equals_oracle(oracle, f, levels, sf, what):
    import lucas_kanade_pyramidal as P

    got = P.build_gaussian_pyramid(f, levels, sf)
    exp = oracle.build_gaussian_pyramid(f, levels, sf)
    assert len(got) == len(exp) == levels
    for lvl, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and g.dtype == e.dtype == np.float32
        g, e = g + np.float32(0.0), e + np.float32(0.0)
        assert g[-1].tobytes() == e[-1].tobytes(), ("last output row", what, lvl, int(np.count_nonzero(g[-1] != e[-1])))
        assert g[:, -1].tobytes() == e[:, -1].tobytes(), ("last output column", what, lvl, int(np.count_nonzero(g[:, -1] != e[:, -1])))
        assert g.tobytes() == e.tobytes(), (what, lvl, int(np.count_nonzero(g != e)))


def test_the_shapes_take_the_paths_they_are_here_for():
    L = lib()
    for shape, levels in HALF_SHAPES:
        st = S.steps(L, shape, levels)
        assert all(L.oflk_pyramid_step_half(*s, 8) == 1 for s in st), (shape, st)
    # 96 x 200: tile (1, 1) and (1, 2) of the first step stage source rows 24 .. 71 and columns 56 .. 135, 120 .. 199
    assert 2 * 16 - 8 >= 0 and 2 * 16 + 40 <= 96 and 2 * 32 - 8 >= 0 and 2 * 64 + 72 <= 200
    for n, t in ((33, 17), (65, 33)):
        assert int(n * 0.52) == t and L.oflk_pyramid_step_half(n, n, t, t, 8) == 1
    (h, w), sf = S.tight_but_not_half(L)
    assert L.oflk_pyramid_step_form(h, w, int(h * sf), int(w * sf), 8) == S.TIGHT
    assert L.oflk_pyramid_step_half(h, w, int(h * sf), int(w * sf), 8) == 0


@pytest.mark.parametrize("sl", HALF_SHAPES, ids=_ids)
def test_pyramid_equals_the_oracle(oracle, sl):
    shape, levels = sl
    for name, f in pyramid_frames(shape).items():
        assert_pyramid_equals_oracle(oracle, f, levels, 0.5, (name, shape))


@pytest.mark.parametrize("n", [33, 65])
def test_a_linspace_step_of_exactly_two_equals_the_oracle(oracle, n):
    """S = 2 T - 1: half scale by the predicate, with the last point on the even cell 2 (T - 1) and its second tap below it"""
    for name, f in pyramid_frames((n, n)).items():
        assert_pyramid_equals_oracle(oracle, f, 2, 0.52, (name, n))


def test_a_tight_step_off_the_half_scale_ratio_still_equals_the_oracle(oracle):
    shape, sf = S.tight_but_not_half(lib())
    for name, f in pyramid_frames(shape).items():
        assert_pyramid_equals_oracle(oracle, f, 2, sf, (name, shape, sf))


def plan_flows(prev, curr, levels, arith, u8):
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
    plan = _oflk.Plan(0, B, H, W, levels, 5, 3)
    try:
        plan.set_arithmetic(arith)
        (plan.pyramidal_u8 if u8 else plan.pyramidal)(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st)
        if arith != 2:   # the exact flow: the pixels the device left undecided, from the host
            plan.resolve_uncertain(tp.data_ptr(), tc.data_ptr(), u.data_ptr(), v.data_ptr(), st, u8=u8)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return u.cpu().numpy(), v.cpu().numpy()


@pytest.fixture(scope="module")
def batch():
    """three pairs of 8-bit frames per shape"""
    out = {}
    for shape, _ in HALF_SHAPES:
        fr = C.frames(*shape)
        prev = [fr[n][0] for n in ("smooth", "noise", "dots")]
        out[shape] = (prev, [np.roll(f, (1, 2), axis=(0, 1)) for f in prev])
    return out


@pytest.fixture(scope="module")
def reference_flows(oracle, batch):
    """per shape: the oracle's flows for the exact arithmetic; for the contracted and the tolerant one their CPU statement
    (oracle/oflk_tolerant_model.c), which says what the device computes in those modes operation for operation"""
    import oflk_tolerant_model as M

    out = {}
    for shape, levels in HALF_SHAPES:
        prev, curr = batch[shape]
        exact = [oracle.lucas_kanade_pyramidal_ex(p, c, levels, 5, 3)[:2] for p, c in zip(prev, curr)]
        contracted = [M.pyramidal(p, c, M.contracted_spec(levels, 3), 5)[:2] for p, c in zip(prev, curr)]
        tolerant = [M.pyramidal(p, c, M.tolerant_spec(levels, 3, shape), 5)[:2] for p, c in zip(prev, curr)]
        out[shape] = {0: exact, 1: contracted, 2: tolerant}
    return out


def test_contracted_flows_equal_the_exact_ones_where_that_is_documented(batch, reference_flows):
    """the contracted pyramid moves about one pyramid value in 10^7 and no flow value on the frames
    measured there.  The two 3-level shapes here (tests/test_gpu_pyr_tight.py asserts the same of its own 64 x 96 batch) keep
    that property, so their contracted flows are held to the oracle's as well; the 8-bit noise frame of 34 x 36 does
    not have it (the contracted CPU statement and the device agree on 575 u values that differ from the exact flow)."""
    for shape in ((96, 200), (64, 96)):
        prev, curr = batch[shape]
        u, v = plan_flows(prev, curr, 3, 1, False)
        for i, (ou, ov) in enumerate(reference_flows[shape][0]):
            assert np.array_equal(u[i], ou) and np.array_equal(v[i], ov), (shape, i, int(np.count_nonzero(u[i] != ou)))


@pytest.mark.parametrize("u8", [False, True], ids=["float32", "uint8"])
@pytest.mark.parametrize("arith", [0, 1, 2], ids=["exact", "contracted", "tolerant"])
@pytest.mark.parametrize("sl", HALF_SHAPES, ids=_ids)
def test_plan_batch_of_three_gives_the_reference_flow(batch, reference_flows, sl, arith, u8):
    shape, levels = sl
    prev, curr = batch[shape]
    u, v = plan_flows(prev, curr, levels, arith, u8)
    for i, (ru, rv) in enumerate(reference_flows[shape][arith]):
        assert np.array_equal(u[i], ru) and np.array_equal(v[i], rv), (shape, arith, u8, i, int(np.count_nonzero(u[i] != ru)))
