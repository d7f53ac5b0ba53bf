"""CPU tests of the alignment statement (tests/align_model.py): what the refinement reaches against a planted map, the bytes
of every refusal and freeze, the summation order, and the library's host-only refusals (make align-host-check)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import align_model as AM
import homography_model as HM

ROOT = Path(__file__).resolve().parents[1]
H, W, L, N = 96, 128, 3, 5
KINDS = [AM.HOMOGRAPHY, AM.AFFINE]
# measured with this file's scenes (seed 1): the largest corner error after refinement, px; the bound is twice that, because
# the resampling of B sets a floor that varies with the texture
MEASURED = {(AM.HOMOGRAPHY, "identity"): 0.00607, (AM.HOMOGRAPHY, "pushed"): 0.00607,
            (AM.AFFINE, "identity"): 0.00197, (AM.AFFINE, "pushed"): 0.00197}


@pytest.fixture(scope="module")
def scenes(oracle):
    out = {}
    for kind in KINDS:
        A, B, planted = AM.planted_pair(H, W, 1, kind)
        out[kind] = (AM.pyramids(A, L), AM.pyramids(B, L), planted, A, B)
    return out


@pytest.mark.parametrize("start", ["identity", "pushed"])
@pytest.mark.parametrize("kind", KINDS)
def test_refinement_reaches_the_planted_map(scenes, kind, start):
    """A 96 x 128 band-limited texture, B resampled from it under a planted map that moves the corners by up to 3 px; L = 3,
    n = 5.  Measured largest corner error, before -> after refinement: homography 2.90580 -> 0.00607 px from the identity and
    1.06278 -> 0.00607 px from the planted map with its corners pushed by 1 px; affine 2.90580 -> 0.00197 px and 1.06117 ->
    0.00197 px.  Both starts reach the same model to the digits shown.  The bound is twice the measured value: 0.01214 px
    (homography) and 0.00394 px (affine)."""
    pa, pb, planted, _, _ = scenes[kind]
    m0 = AM.IDENTITY[kind] if start == "identity" else AM.pushed(planted, H, W, kind)
    out, status, stats = AM.refine_pyramids(pa, pb, m0, 1, kind, N)
    e0, e1 = AM.corner_error(m0, planted, H, W), AM.corner_error(out, planted, H, W)
    print(f"kind {kind} start {start}: corner error {e0:.5f} -> {e1:.5f} px, status {status}, stats {stats}")
    assert status == 1 and stats[3] == L * N and stats[1] < stats[0]
    assert e1 < e0
    assert e1 <= 2.0 * MEASURED[(kind, start)]


@pytest.mark.parametrize("kind", KINDS)
def test_equal_frames_under_the_identity_give_the_identity_back(scenes, kind):
    pa = scenes[kind][0]
    out, status, stats = AM.refine_pyramids(pa, pa, AM.IDENTITY[kind], 1, kind, N)
    assert status == 1 and out.tobytes() == AM.IDENTITY[kind].tobytes()
    assert stats.tolist() == [0.0, 0.0, 1.0, float(L * N)]


@pytest.mark.parametrize("kind", KINDS)
def test_refused_and_frozen_steps_return_the_input_bytes(scenes, kind):
    pa, pb, planted, A, _ = scenes[kind]
    nc = len(AM.IDENTITY[kind])
    m0 = AM.pushed(planted, H, W, kind)
    # input status 0, and a model that is not finite
    out, status, stats = AM.refine_pyramids(pa, pb, m0, 0, kind, N)
    assert status == 0 and out.tobytes() == m0.tobytes() and not stats.any()
    for bad in (np.nan, np.inf):
        mb = m0.copy()
        mb[nc - 2] = bad
        out, status, stats = AM.refine_pyramids(pa, pb, mb, 1, kind, N)
        assert status == 0 and out.tobytes() == mb.tobytes() and not stats.any()
    # a flat template: every pivot is zero
    flat = AM.pyramids(np.full((H, W), 7.0, np.float32), L)
    out, status, stats = AM.refine_pyramids(flat, pb, m0, 1, kind, N)
    assert status == 0 and out.tobytes() == m0.tobytes() and stats[3] == 0 and stats[2] > 0.9
    # a model that throws B out of the frame: nothing is counted
    off = AM.IDENTITY[kind].copy()
    off[2] = 4.0 * W
    out, status, stats = AM.refine_pyramids(pa, pb, off, 1, kind, N)
    assert status == 0 and out.tobytes() == off.tobytes() and stats[2] == 0 and stats[3] == 0 and np.isnan(stats[0])
    # a step made worse: rejected
    ca, cb = AM.checker_pair(40, 56)
    out, status, stats = AM.refine_pyramids(AM.pyramids(ca, 1), AM.pyramids(cb, 1), AM.IDENTITY[kind], 1, kind, 1)
    assert status == 2 and out.tobytes() == AM.IDENTITY[kind].tobytes() and stats[0] == 1.0 and stats[1] > 1000.0 and stats[3] == 1


def test_uint8_frames_are_their_float_values(scenes):
    _, _, planted, A, B = scenes[AM.HOMOGRAPHY]
    a8, b8 = np.rint(A).astype(np.uint8), np.rint(B).astype(np.uint8)
    m0 = AM.pushed(planted, H, W, AM.HOMOGRAPHY)[None]
    AM.same(AM.refine(a8[None], b8[None], m0, levels=2, iterations=2),
            AM.refine(a8[None].astype(np.float32), b8[None].astype(np.float32), m0, levels=2, iterations=2), "uint8")


def test_batches_and_sequences_are_their_steps(scenes):
    """the result does not depend on how the steps are batched: a batch is its steps one by one, and the sequence form is the
    pair form on consecutive frames"""
    _, _, planted, A, B = scenes[AM.HOMOGRAPHY]
    frames = np.stack([A, B, A, np.full_like(A, 3.0)])[:, :40, :56]
    model = np.stack([AM.IDENTITY[AM.HOMOGRAPHY]] * 3)
    model[1, 2] = 0.5
    status = np.array([1, 1, 0], np.int32)
    seq = AM.sequence(frames, model, status, levels=2, iterations=2)
    AM.same(AM.refine(frames[:-1], frames[1:], model, status, levels=2, iterations=2), seq, "pair form")
    for s in range(3):
        one = AM.refine(frames[s:s + 1], frames[s + 1:s + 2], model[s:s + 1], status[s:s + 1], levels=2, iterations=2)
        AM.same(one, tuple(x[s:s + 1] for x in seq), f"step {s}")
    assert seq[1].tolist()[2] == 0


@pytest.mark.parametrize("shape", [(33, 47), (64, 64), (70, 257), (32, 129), (1, 65)])
def test_the_summation_order_at_sizes_off_the_tile(shape):
    """ordered_sum against the order written out pixel by pixel: tiles of 64 x 32 in raster order, a column top to bottom, the
    64 columns by the tree, at heights and widths that are no multiples of the tile"""
    Hh, Ww = shape
    rng = np.random.default_rng(Hh * 1000 + Ww)
    terms = rng.standard_normal((2, Hh, Ww)) * 10.0 ** rng.integers(-6, 7, (2, Hh, Ww))
    counted = rng.random((Hh, Ww)) < 0.8
    got = AM.ordered_sum(terms, counted)
    want = np.zeros(2)
    for k in range(2):
        total = 0.0
        for ty in range(0, Hh, AM.TILE_H):
            for tx in range(0, Ww, AM.TILE_W):
                part = [0.0] * AM.TILE_W
                for c in range(AM.TILE_W):
                    for y in range(ty, min(ty + AM.TILE_H, Hh)):
                        if tx + c < Ww and counted[y, tx + c]:
                            part[c] = part[c] + float(terms[k, y, tx + c])
                st = AM.TILE_W // 2
                while st >= 1:
                    for c in range(st):
                        part[c] = part[c] + part[c + st]
                    st //= 2
                total = total + part[0]
        want[k] = total
    assert got.tobytes() == want.tobytes()
    assert np.allclose(got, np.where(counted, terms, 0.0).sum((1, 2)), rtol=1e-9, atol=1e-6)


def test_the_six_parameter_elimination_is_solve8s(oracle):
    """solve on NP = 6 rows against solve8 on the same system padded by two identity rows, and against numpy"""
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((40, 6))
    G = np.concatenate([Q.T @ Q, rng.standard_normal((6, 1))], 1)
    h, ok = AM.solve(G, 6)
    G8 = np.zeros((8, 9))
    G8[:6, :6], G8[:6, 8], G8[6, 6], G8[7, 7] = G[:, :6], G[:, 6], 1.0, 1.0
    h8, ok8 = HM.solve8(G8)
    assert ok and ok8 and h.tobytes() == h8[:6].tobytes()
    assert np.allclose(h, np.linalg.solve(G[:, :6], G[:, 6]), rtol=1e-9)
    G[2, 2] = np.nan
    assert not AM.solve(G, 6)[1]


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="no hipcc to build the host check")
def test_make_align_host_check_passes():
    """the workspace sizing and every refusal that needs no device, under host ASan/UBSan (tools/align_host_check.hip)"""
    r = subprocess.run(["make", "-C", str(ROOT / "optical-flow-fpga_amd" / "csrc"), "align-host-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "align host check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
