"""The scenes of tests/range_feature_scenes.py on the statements alone (no GPU): every scene does what it promises, so that no
comparison of tests/test_gpu_ranges_features.py is NaN against NaN throughout or 0 against 0 throughout.  The counts in the
comments are the statements' own on these shapes and seeds."""
import numpy as np
import pytest

import range_feature_scenes as F
import range_scenes as S


@pytest.fixture(autouse=True)
def _quiet_fp():
    """these scenes overflow, underflow and make NaN on purpose: NumPy's warnings off for this module's tests only"""
    with np.errstate(all="ignore"):
        yield


def test_the_added_scenes_are_what_they_say():
    x = F.sparse_frames(24, 32)[0]
    assert np.array_equal(F.transform("u16", x, True), (x.astype(np.float64) * 257.0).astype(np.float32))
    tiny = np.finfo(np.float32).tiny
    for name in F.SUBNORMAL:
        t = F.transform(name, x, True)
        assert (t > 0).all() and (t < tiny).all()
        ulps = t.view(np.uint32).astype(np.int64)          # a positive subnormal's bits are its multiple of the ulp
        assert np.count_nonzero(ulps % 512) > 0.9 * t.size, name    # off range_scenes' 2^9-ulp grid
    assert not np.isfinite(F.transform("holes", x, True)).all() and np.isfinite(F.transform("huge", x, True)).all()


def test_ring_points_put_the_hole_on_the_patch_ring_only():
    H, W, w = 24, 32, 5
    h = w // 2
    pts = F.ring_points([(10, 12)], H, W, w)
    d = np.abs(pts - np.array([10, 12], np.float32))
    cheb = d.max(axis=1)
    assert (cheb == h + 1).sum() == 3 and (cheb <= h).sum() == 1 and (cheb > w + 2).sum() == 1
    for want in ((0, h + 1), (h + 1, 0), (h + 1, h + 1)):
        assert (d == np.array(want, np.float32)).all(axis=1).sum() == 1
    # at the frame's edge only the positions inside are kept
    edge = F.ring_points([(W - 1, H - 1), (W - 2, 3)], H, W, w)
    assert edge.tolist() == [[W - 2, 3 + h + 1], [W - 1, 3]]


# ---- sparse LK -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SCENES)
def test_sparse_scenes_solve_or_refuse_as_stated(oracle, name):
    import sparse_model as M

    fr = F.frames_of(name, F.sparse_frames(24, 32))
    pts = F.sparse_points(fr[0], 5)
    assert len(pts) == 60
    nxt, status, res = M.sparse_lk(fr[0], fr[1], pts, 2, 5, 3)
    if name in ("signed", "u16"):
        assert status.sum() >= len(pts) // 2                       # 60 of 60
        assert np.isfinite(res).all()
    elif name == "holes":
        assert np.isnan(res).any() and status.sum() >= len(pts) // 3
        assert len(F.hole_positions(fr[0])) == 5
    elif name in ("big", "huge", "tiny", "tinyfrac"):
        assert not status.any()                                    # products overflow / underflow: status 0 is the statement
        assert np.isfinite(nxt).any() or name in ("big", "huge")
    else:   # small: normal pixels, products underflow
        assert not status.any()


def test_sparse_tracks_statement_evaluates_nan_residuals(oracle):
    import sparse_model as M

    fr = F.frames_of("holes", F.sparse_frames(24, 32, 3))
    pts = F.sparse_points(fr[0], 5)
    tr, vis = M.track(fr, None, pts, 2, 5, 3)
    assert vis[0].all() and 0 < vis[2].sum() < vis[0].sum()       # some tracks end on the holes, some live on


def test_online_tracker_statement_tracks_and_ends_on_the_scenes(oracle):
    """the two tracker cells of the GPU file are real comparisons"""
    import tracker_model as TM

    for name in ("holes", "huge"):
        fr = F.frames_of(name, F.sparse_frames(40, 52, 4))
        (xy, vis, born, det, res), _ = TM.pushes(fr, 30, 2, quality_level=0.05, min_distance=4.0)
        if name == "holes":   # tracks end on the holes and are replaced at the next detection; NaN residuals are logged
            assert vis.sum(axis=1).tolist() == [30, 16, 30, 18] and det.tolist() == [30, 0, 16, 0]
            assert np.isnan(res).sum() == 54 and np.isfinite(res).sum() > 30
        else:                 # window products overflow: 30 slots are born at every detection and none survives a step
            assert vis.sum(axis=1).tolist() == [30, 0, 30, 0] and det.tolist() == [30, 0, 30, 0]


# ---- interpolation ---------------------------------------------------------------------------------------------------
def test_interpolation_holes_reach_few_pixels_and_status_ignores_the_scene():
    import interp_model as M

    H, W = 24, 32
    flows = F.unit_flows(1, H, W)
    base = None
    for name in ("signed", "holes", "huge"):
        new, status = M.interpolate(F.interp_frames(name, 1, H, W), *flows, [0.5])
        hist = np.bincount(status.ravel(), minlength=4)
        base = hist if base is None else base
        assert np.array_equal(hist, base), name                    # the status is a function of the flows
        if name == "holes":
            assert 0 < np.isnan(new).sum() < new.size // 10
    assert base[3] > 0.5 * H * W


# ---- warps -----------------------------------------------------------------------------------------------------------
def test_warp_holes_make_nan_pixels_and_the_inside_count_is_the_8_bit_scenes():
    import homography_model as HM
    import stabilize_model as SM

    H, W = 37, 53
    plain = F.sparse_frames(H, W)
    holes = F.warp_frames("holes", H, W)
    for persp, warp in ((False, SM.warp), (True, HM.warp)):
        maps = F.warp_maps(H, W, persp)
        for key, m in maps.items():
            mm = np.stack([m, m])
            out, inside = warp(holes, mm)
            _, inside8 = warp(plain, mm)
            if key == "behind":   # every divisor negative: nothing is sampled, though every position is inside the frame
                assert not inside.any() and not out.any()
                continue
            assert np.isnan(out).sum() > 0, key
            assert inside.sum() == inside8.sum() > 0, key
    # the identity: a sample at integer positions reads the next pixel with weight 0, and 0 * inf is NaN
    out, _ = SM.warp(holes, np.stack([F.warp_maps(H, W, False)["identity"]] * 2))
    assert np.isnan(out).sum() > np.isnan(holes).sum()


# ---- mosaic ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("projective", [False, True])
def test_mosaic_scene_covers_its_canvas_and_holes_reach_it(projective):
    import mosaic_model as MM

    frames, maps, (x0, y0), (Hc, Wc) = F.mosaic_scene("holes", projective)
    for blend in MM.BLENDS.values():
        out, count = MM.composite(frames, maps, None, x0, y0, Hc, Wc, blend)
        assert count.max() == 3 and (count == 0).any()
        assert 0 < np.isnan(out).sum() < out.size // 4
    # behind: frame 1 covers nothing, and the canvas is that of frames 0 and 2 alone
    frames, maps, (x0, y0), (Hc, Wc) = F.mosaic_scene("holes", projective, behind=True)
    for blend in MM.BLENDS.values():
        out, count = MM.composite(frames, maps, None, x0, y0, Hc, Wc, blend)
        two = MM.composite(frames[[0, 2]], maps[[0, 2]], None, x0, y0, Hc, Wc, blend)
        assert count.max() == 2 and S.same(out, two[0]) and np.array_equal(count, two[1])


# ---- alignment -------------------------------------------------------------------------------------------------------
def _families():
    import align_model as AM
    import align_photo_model as APM
    import align_robust_model as ARM

    return {"plain": lambda a, b, m, k, L, n: AM.refine(a, b, m, None, k, L, n),
            "photo": lambda a, b, m, k, L, n: APM.refine(a, b, m, None, k, L, n),
            "robust": lambda a, b, m, k, L, n: ARM.refine(a, b, m, 4.0, None, k, L, n)}


@pytest.mark.parametrize("family", ["plain", "photo", "robust"])
def test_alignment_solves_on_the_finite_scenes_and_refuses_holes(oracle, family):
    import align_model as AM

    refine = _families()[family]
    for name in ("signed", "big", "huge", "tiny", "small"):
        a, b, m = F.align_pair(name, 33, 47, AM.AFFINE)
        r = refine(a, b, m, AM.AFFINE, 2, 3)
        assert r[1][0] == 1, (name, r[1], r[2])
        if name == "tiny":   # the sums are fp64, so subnormal gradients count: about 1e-84, not 0
            assert 0 < r[2][0, 0] < 1e-80 and 0 < r[2][0, 1] < 1e-80, r[2]
    a, b, m = F.align_pair("holes", 33, 47, AM.AFFINE)
    r = refine(a, b, m, AM.AFFINE, 2, 3)
    assert r[1][0] == 0 and np.isnan(r[2][0, :2]).all()


@pytest.mark.parametrize("family", ["plain", "photo", "robust"])
def test_alignment_ignores_holes_that_no_counted_pixel_reads(oracle, family):
    import align_model as AM

    refine = _families()[family]
    for kind in (AM.AFFINE, AM.HOMOGRAPHY):
        with_holes = refine(*F.holes_unsampled(33, 47, kind), kind, 1, 3)
        without = refine(*F.holes_unsampled(33, 47, kind, holes=False), kind, 1, 3)
        assert with_holes[1][0] == 1
        for g, w in zip(with_holes, without):
            assert np.asarray(g).tobytes() == np.asarray(w).tobytes()
    a, b, _ = F.holes_unsampled(33, 47, AM.AFFINE)
    assert np.isnan(a).sum() == 1 and (~np.isfinite(b)).sum() == 4


# ---- gradients -------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """one rounding: the float32 nearest to a * b + c; exact in float64 here, since b is a power of two and a, c are
    multiples of 2^-149 below 2^-125 in size"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _fma_sobel(avg):
    """the fused-multiply-add order the kernels had: the first product rounded, then five fmas, on the `symm` border"""
    p = np.pad(avg, 1, mode="symmetric").astype(np.float64)
    H, W = avg.shape

    def at(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    def chain(taps):
        (dy, dx, k), rest = taps[0], taps[1:]
        acc = (at(dy, dx) * k).astype(np.float32)
        for dy, dx, k in rest:
            acc = (at(dy, dx) * k + acc.astype(np.float64)).astype(np.float32)
        return acc

    ix = chain([(1, 1, -0.125), (1, -1, 0.125), (0, 1, -0.25), (0, -1, 0.25), (-1, 1, -0.125), (-1, -1, 0.125)])
    iy = chain([(1, 1, -0.125), (1, 0, -0.25), (1, -1, -0.125), (-1, 1, 0.125), (-1, 0, 0.25), (-1, -1, 0.125)])
    return ix, iy


def _convolve2d_sobel(avg):
    from scipy.signal import convolve2d

    sx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float32) / np.float32(8.0)
    sy = np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], np.float32) / np.float32(8.0)
    rx, ry = convolve2d(avg, sx, "same", "symm"), convolve2d(avg, sy, "same", "symm")
    assert rx.dtype == ry.dtype == np.float32
    return rx, ry


@pytest.mark.parametrize("name", F.GRADIENT_SCENES)
def test_subnormal_gradients_are_convolve2d_byte_for_byte(oracle, name):
    p, c = F.gradient_pair(name)
    Ix, Iy, _ = oracle.compute_gradients(p, c)
    rx, ry = _convolve2d_sobel((p + c) / np.float32(2.0))
    assert Ix.tobytes() == rx.tobytes() and Iy.tobytes() == ry.tobytes()
    assert np.count_nonzero(Ix) > 2000 and np.count_nonzero(Iy) > 2000


@pytest.mark.parametrize("name", F.GRADIENT_SCENES)
def test_oracle_gradients_equal_the_reference_fixture(oracle, golden_dir, name):
    z = np.load(golden_dir / "reference_gradients_tinyfrac.npz")
    for nm, a in zip(("Ix", "Iy", "It"), oracle.compute_gradients(*F.gradient_pair(name))):
        ref = z[f"{name}/{nm}"]
        assert ref.dtype == np.float32 and a.tobytes() == ref.tobytes(), (name, nm)


def test_the_fma_order_differs_where_products_tie_and_only_there(oracle):
    """what separates the kernels' earlier order (one rounding per fma) from convolve2d's (product rounded, then added)"""
    differ = {}
    for name in ("tiny", "tinyfrac", "tinyulp"):
        p, c = S.scene("tiny", "odd") if name == "tiny" else F.gradient_pair(name)
        Ix, Iy, _ = oracle.compute_gradients(p, c)
        fx, fy = _fma_sobel((p + c) / np.float32(2.0))
        differ[name] = (int(np.count_nonzero(fx != Ix)), int(np.count_nonzero(fy != Iy)))
    # integer crops: range_scenes' `tiny` sits on the 2^9-ulp grid and `tinyfrac` at 3 mod 8 ulps, so no product ties;
    # `tinyulp` is the scene that discriminates there (1089 and 1117 of 2745 pixels)
    assert differ["tiny"] == (0, 0) and differ["tinyfrac"] == (0, 0)
    assert min(differ["tinyulp"]) > 500
    # the builders' non-integer frames under `tiny` and `tinyfrac`, as alignment's template sees them (its average is of
    # the template with itself), at both levels of the (33, 47) cell: 100 to 520 pixels each
    import align_model as AM

    for name in F.SUBNORMAL:
        a, _, _ = F.align_pair(name, 33, 47, AM.AFFINE)
        for lv in AM.pyramids(a[0], 2):
            Ix, Iy, _ = oracle.compute_gradients(lv, lv)
            rx, ry = _convolve2d_sobel((lv + lv) / np.float32(2.0))
            assert Ix.tobytes() == rx.tobytes() and Iy.tobytes() == ry.tobytes()
            fx, fy = _fma_sobel((lv + lv) / np.float32(2.0))
            assert np.count_nonzero(fx != Ix) > 50 and np.count_nonzero(fy != Iy) > 50, (name, lv.shape)
