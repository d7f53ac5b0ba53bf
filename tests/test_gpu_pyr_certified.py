"""The exact pyramid runs fused multiply-adds behind a rounding certificate (k_pyr_down<PIX, PYR_CERTIFIED>; DESIGN.md
section 2): its results must stay the oracle's byte for byte, on frames that keep every wave on the fast path and on
frames that send waves to the exact redo (which tests/pyr_cert_model.py shows beforehand), as float32 and as uint8; and
the opt-in modes must stay what the parent of this change computed (tests/golden/pyr_certified_digests.json)."""
import hashlib
import json

import numpy as np
import pytest

import pyr_cert_model as C

pytestmark = pytest.mark.gpu

SHAPES = [(200, 328),   # interior tiles, pair staging, one-mirror border tiles
          (67, 131),    # odd: every tile on the border
          (20, 24)]     # the reflection wraps more than once
_frames = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = C.frames(*shape)
    return _frames[shape]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def plan_flows(frames_prev, frames_curr, arith=0, u8=False):
    import torch

    import _oflk

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    p, c = np.stack(frames_prev), np.stack(frames_curr)
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


def plan_case():
    """the 2-pair 200 x 328 call of the arithmetic-mode test (also what the golden digests were recorded from)"""
    from oflk_synth import synth_pair

    pairs = [synth_pair(200, 328, i) for i in range(2)]
    return [p for p, _ in pairs], [c for _, c in pairs]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_equals_the_oracle(oracle, shape):
    import lucas_kanade_pyramidal as P

    H, W = shape
    fr = frames(shape)
    # the redo path is exercised: the CPU statement of the guard flags values of the first vertical pass
    flagged, _ = C.flag_vertical(fr["dots"][0], C.dot_columns(W))
    assert flagged.any(), "no value of the dot frame is flagged"
    # (rows 0 .. 19 hold everything the threads of rows 0 .. 11 read)
    flagged, _ = C.flag_vertical(fr["adversarial"][0][:20], C.adversarial_columns(W, len(C.adversarial_set())))
    assert flagged[9].all(), "an adversarial window is not flagged where the vertical pass meets it"
    for name, (f, _) in fr.items():
        got = P.build_gaussian_pyramid(f, 3, 0.5)
        exp = oracle.build_gaussian_pyramid(f, 3, 0.5)
        assert len(got) == len(exp) == 3
        for lvl, (g, e) in enumerate(zip(got, exp)):
            assert g.shape == e.shape and g.dtype == e.dtype == np.float32
            same = (g + np.float32(0.0)).tobytes() == (e + np.float32(0.0)).tobytes()
            assert same, (name, shape, lvl, int(np.count_nonzero(g != e)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_uint8_frames_give_the_float32_flow(shape):
    fr = frames(shape)
    names = [n for n, (_, eight_bit) in fr.items() if eight_bit]
    assert {"smooth", "noise", "checker", "dots", "zeros"} <= set(names)
    prev = [fr[n][0] for n in names]
    curr = [np.roll(f, (1, 2), axis=(0, 1)) for f in prev]
    uf, vf = plan_flows(prev, curr)
    u8, v8 = plan_flows(prev, curr, u8=True)
    for i, n in enumerate(names):
        assert uf[i].tobytes() == u8[i].tobytes() and vf[i].tobytes() == v8[i].tobytes(), (n, shape)


def test_arithmetic_modes(oracle, golden_dir):
    """exact: the oracle's flow.  Contracted and tolerant: the digests recorded from the parent of this change."""
    prev, curr = plan_case()
    u, v = plan_flows(prev, curr, 0)
    for i in range(2):
        ou, ov, _, _ = oracle.lucas_kanade_pyramidal_ex(prev[i], curr[i], 3, 5, 3)
        assert np.array_equal(u[i], ou) and np.array_equal(v[i], ov), i
    want = json.loads((golden_dir / "pyr_certified_digests.json").read_text())
    for mode, key in ((1, "contracted"), (2, "tolerant")):
        u, v = plan_flows(prev, curr, mode)
        assert digest(u, v) == want[key], key
