"""The float32 calls beyond the dense flow paths on frames outside the 8-bit value range (tests/range_feature_scenes.py):
sparse LK, the sparse tracks and the online tracker, the affine and perspective warps, frame interpolation, the mosaic and its
exposure form, the three direct-alignment families and alignment_weights, and compute_gradients on subnormal frames off the
2^9-ulp grid.  Every (call, scene) cell is held to the call's statement under range_scenes' rule: NaN at the same positions,
every other value equal as a value; integer outputs exactly.  tests/test_ranges_features_cpu.py shows on the statements alone
which cells solve and which refuse, so that none of these comparisons is NaN against NaN or 0 against 0 throughout.
(run on an MI355X: python -m pytest tests/test_gpu_ranges_features.py -m gpu -q)"""
import numpy as np
import pytest

import range_feature_scenes as F

pytestmark = pytest.mark.gpu
same = F.assert_same


@pytest.fixture(autouse=True)
def _quiet_fp():
    """these scenes overflow, underflow and make NaN on purpose: NumPy's warnings off for this module's tests only"""
    with np.errstate(all="ignore"):
        yield


# ---------------------------------------------------------------------------------------------------------------------
# sparse LK, the tracks, the online tracker
# ---------------------------------------------------------------------------------------------------------------------
SPARSE = [((24, 32), 2, 5, 3), ((33, 47), 3, 7, 2)]


@pytest.mark.parametrize("name", F.SCENES)
@pytest.mark.parametrize("shape,L,w,K", SPARSE, ids=lambda v: str(v))
def test_sparse_lk(oracle, shape, L, w, K, name):
    import lucas_kanade_pyramidal as P
    import sparse_model as M

    fr = F.frames_of(name, F.sparse_frames(*shape))
    pts = F.sparse_points(fr[0], w, 60 if shape[0] < 30 else 100)
    want = M.sparse_lk(fr[0], fr[1], pts, L, w, K)
    got = P.lucas_kanade_sparse(fr[0], fr[1], pts, L, w, K)
    what = f"{name} {shape} L={L} w={w} K={K}"
    same(got[0], want[0], what + ": next points")
    same(got[1], want[1].astype(bool), what + ": status")
    same(got[2], want[2], what + ": residual")


@pytest.mark.parametrize("name", F.SCENES)
def test_sparse_tracks(oracle, name):
    """T = 3: the forward-backward and the residual tests meet NaN and inf residuals and displacements"""
    import lucas_kanade_pyramidal as P
    import sparse_model as M

    fr = F.frames_of(name, F.sparse_frames(24, 32, 3))
    pts = F.sparse_points(fr[0], 5)
    want = M.track(fr, None, pts, 2, 5, 3)
    got = P.lucas_kanade_pyramidal_sequence_sparse_tracks(fr, pts, 2, 5, 3)
    same(got.tracks, want[0], f"{name}: tracks")
    same(got.visible, want[1].astype(bool), f"{name}: visible")


@pytest.mark.parametrize("name", ["holes", "huge"])
def test_online_tracker(oracle, name):
    import sparse_replenish_model as RM
    import tracker_model as TM
    from test_gpu_tracker import _push_all, _tracker

    fr = F.frames_of(name, F.sparse_frames(40, 52, 4))
    want, wbirth = TM.pushes(fr, 30, 2, quality_level=0.05, min_distance=4.0)
    tr = _tracker(fr, 30, 2, q=0.05, md=4.0)
    try:
        got, birth = _push_all(tr, fr)
    finally:
        tr.close()
    for g, w, nm in zip(got, want, RM.NAMES):
        same(g, w, f"{name}: {nm}")   # shape and dtype included, as sparse_replenish_model.same
    v = got[1] != 0
    assert np.array_equal(birth[v], wbirth[v])


def test_single_scale_on_tinyfrac_equals_the_oracle(oracle):
    """the fused flow kernels keep their Sobel: products of two subnormal gradients are 0, so nothing is solved either way"""
    import lucas_kanade_core as K

    for name in F.GRADIENT_SCENES:
        p, c = F.gradient_pair(name)
        for win in (5, 13):
            u, v = K.lucas_kanade_single_scale(p, c, win)
            ou, ov = oracle.lucas_kanade_single_scale(p, c, win)
            same(u, ou, f"{name} {win}: u")
            same(v, ov, f"{name} {win}: v")


# ---------------------------------------------------------------------------------------------------------------------
# the warps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SCENES)
@pytest.mark.parametrize("shape", [(5, 7), (37, 53)], ids=str)
@pytest.mark.parametrize("perspective", [False, True], ids=["affine", "perspective"])
def test_warps(perspective, shape, name):
    import homography_model as HM
    import lucas_kanade_core as K
    import stabilize_model as SM

    frames = F.warp_frames(name, *shape)
    call, model = (K.warp_perspective, HM.warp) if perspective else (K.warp_affine, SM.warp)
    for key, m in F.warp_maps(*shape, perspective).items():
        maps = np.stack([m, m])
        want = model(frames, maps)
        out, inside = call(frames, maps, return_inside=True)
        same(out, want[0], f"{name} {shape} {key}: frames")
        same(inside, want[1].astype(bool), f"{name} {shape} {key}: inside")


# ---------------------------------------------------------------------------------------------------------------------
# interpolation
# ---------------------------------------------------------------------------------------------------------------------
INTERP_TAUS = [0.5, 1 / 3, 1 - 2.0 ** -20]


@pytest.mark.parametrize("name", F.SCENES)
@pytest.mark.parametrize("shape", [(24, 32), (37, 53)], ids=str)
def test_interpolate_frames(shape, name):
    """test_gpu_interp._check_all_forms without its assertion that the statement is finite"""
    import interp_model as M
    import lucas_kanade_pyramidal as P
    from test_gpu_interp import _device, _planted_flows, _wild_flows

    B, (H, W) = 2, shape
    frames = F.interp_frames(name, B, H, W)
    # zero flows: every sample sits on a pixel, so its weight-0 taps fall on the next column and row -- on a hole, or past
    # the last column and row, where the kernel's taps come from the other side than SciPy's
    for kind, make in (("planted", _planted_flows), ("wild", _wild_flows), ("zero", None)):
        flows = make(B, H, W, seed=H * 7 + W) if make else [np.zeros((B, H, W), np.float32) for _ in range(4)]
        want = M.interpolate(frames, *flows, INTERP_TAUS, 0.01, 0.5, 2)
        got = _device(frames, flows, INTERP_TAUS, 0.01, 0.5, 2, True)
        host = P.interpolate_frames(frames, *flows, taus=INTERP_TAUS, refine=2, return_status=True)
        for form, g in (("device", got), ("host", host)):
            same(g[0], want[0], f"{name} {shape} {kind} {form}: frames")
            same(g[1], want[1], f"{name} {shape} {kind} {form}: status")


# ---------------------------------------------------------------------------------------------------------------------
# the mosaic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SCENES)
@pytest.mark.parametrize("projective,behind", [(False, False), (True, False), (True, True)],
                         ids=["translation", "homography", "behind"])
def test_mosaic_composite(projective, behind, name):
    """behind: frame 1 lands inside its frame with a negative divisor, so it is outside and its holes stay off the canvas"""
    import lucas_kanade_core as K
    import mosaic_model as MM

    frames, maps, origin, shape = F.mosaic_scene(name, projective, behind)
    for blend, code in MM.BLENDS.items():
        want = MM.composite(frames, maps, None, *origin, *shape, code)
        got = K.mosaic_composite(frames, maps.reshape(-1, 3, 3), shape, origin, blend=blend, return_count=True)
        same(got[0], want[0], f"{name} {blend}: canvas")
        same(got[1], want[1], f"{name} {blend}: count")


@pytest.mark.parametrize("name", ["signed", "huge", "holes"])
def test_mosaic_composite_with_exposure(name):
    import lucas_kanade_core as K
    import mosaic_exposure_model as EM
    import mosaic_model as MM

    for behind in (False, True):
        frames, maps, origin, shape = F.mosaic_scene(name, True, behind)
        for blend, code in MM.BLENDS.items():
            want = EM.composite(frames, maps, None, F.EXPOSURES, *origin, *shape, code)
            got = K.mosaic_composite(frames, maps.reshape(-1, 3, 3), shape, origin, blend=blend, return_count=True,
                                     exposure=F.EXPOSURES)
            same(got[0], want[0], f"{name} {blend} behind={behind}: canvas")
            same(got[1], want[1], f"{name} {blend} behind={behind}: count")


# ---------------------------------------------------------------------------------------------------------------------
# direct alignment
# ---------------------------------------------------------------------------------------------------------------------
ALIGN = [((33, 47), 2, 3), ((64, 64), 1, 1)]
FAMILIES = ["plain", "photometric", "robust"]
DELTA = 4.0


def _refine(family, a, b, model, kind, L, n):
    """(got, want): the call's and the statement's (model (S, nc), status, stats[, photo (S, 2)])"""
    import align_model as AM
    import align_photo_model as APM
    import align_robust_model as ARM
    import lucas_kanade_core as K

    name = {v: k for k, v in AM.KINDS.items()}[kind]
    S = len(a)
    shaped = model.reshape((S, 3, 3) if kind == AM.HOMOGRAPHY else (S, 2, 3))
    if family == "plain":
        r = K.refine_alignment(a, b, shaped, None, name, L, n)
        return (r.model.reshape(S, -1), r.status, r.stats), AM.refine(a, b, model, None, kind, L, n)
    if family == "photometric":
        r = K.refine_alignment(a, b, shaped, None, name, L, n, photometric=True)
        want = APM.refine(a, b, model, None, kind, L, n)
    else:
        r = K.refine_alignment(a, b, shaped, None, name, L, n, robust_delta=DELTA)
        want = ARM.refine(a, b, model, DELTA, None, kind, L, n)
    return (r.model.reshape(S, -1), r.status, r.stats, np.stack([r.gain, r.bias], 1)), want


def _same_alignment(got, want, what):
    for g, w, nm in zip(got, want, ("model", "status", "stats", "photo")):
        same(g, w, f"{what}: {nm}")


@pytest.mark.parametrize("name", F.SCENES)
@pytest.mark.parametrize("shape,L,n", ALIGN, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["affine", "homography"])
@pytest.mark.parametrize("family", FAMILIES)
def test_refine_alignment(oracle, family, kind, shape, L, n, name):
    """S = 2 steps: the scene's pair and the same pair the other way round (b as the template, the inverse push)"""
    import align_model as AM

    code = AM.KINDS[kind]
    a, b, m = F.align_pair(name, *shape, code)
    a2, b2, m2 = F.align_pair(name, *shape, code, seed=sum(shape) + 1)
    a, b, m = np.concatenate([a, b2]), np.concatenate([b, a2]), np.concatenate([m, AM.IDENTITY[code][None]])
    got, want = _refine(family, a, b, m, code, L, n)
    _same_alignment(got, want, f"{family} {kind} {name} {shape} L={L} n={n}")


@pytest.mark.parametrize("kind", ["affine", "homography"])
@pytest.mark.parametrize("family", FAMILIES)
def test_refine_alignment_with_holes_that_no_counted_pixel_reads(oracle, family, kind):
    import align_model as AM

    code = AM.KINDS[kind]
    for shape in ((33, 47), (64, 64)):
        got, want = _refine(family, *F.holes_unsampled(*shape, code), code, 1, 3)
        _same_alignment(got, want, f"{family} {kind} {shape} holes_unsampled")
        assert got[1][0] == 1
        clean, _ = _refine(family, *F.holes_unsampled(*shape, code, holes=False), code, 1, 3)
        for g, w in zip(got, clean):
            assert np.asarray(g).tobytes() == np.asarray(w).tobytes()


@pytest.mark.parametrize("name", ["signed", "huge", "holes"])
@pytest.mark.parametrize("kind", ["affine", "homography"])
def test_alignment_weights(oracle, kind, name):
    import align_model as AM
    import align_robust_model as ARM
    import lucas_kanade_core as K

    code = AM.KINDS[kind]
    for shape in ((33, 47), (64, 64)):
        a, b, m = F.align_pair(name, *shape, code)
        shaped = m.reshape((1, 3, 3) if code == AM.HOMOGRAPHY else (1, 2, 3))
        for gain, bias in ((None, None), (1.1, -3.0), (0.9, 1e30)):
            want = ARM.weights(a[0], b[0], m[0], code, DELTA, gain, bias)
            got = K.alignment_weights(a, b, shaped, kind, DELTA, gain, bias)
            same(got[0], want, f"{kind} {name} {shape} gain {gain} bias {bias}")


# ---------------------------------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.GRADIENT_SCENES)
def test_compute_gradients_on_subnormal_frames_equals_the_reference(golden_dir, name):
    """tinyulp is the cell that an fma Sobel fails (test_ranges_features_cpu: 1089 / 1117 of 2745 pixels)"""
    import lucas_kanade_core as K

    z = np.load(golden_dir / "reference_gradients_tinyfrac.npz")
    p, c = F.gradient_pair(name)
    for nm, a in zip(("Ix", "Iy", "It"), K.compute_gradients(p, c)):
        same(a, z[f"{name}/{nm}"], f"{name}: {nm}")
        assert np.count_nonzero(a) > 2000
