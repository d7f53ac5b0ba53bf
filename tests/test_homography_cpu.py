"""CPU tests of the homography fit and the perspective warp: the statement (tests/homography_model.py) against independent
restatements and references, and what the library and the Python wrappers refuse without a device.  No GPU is used."""
import ctypes

import numpy as np
import pytest

import homography_model as HM
import motion_model as MM
import stabilize_model as SM

# Measured with the committed model (the figures are in DESIGN.md section 2); each gate is four times the measured worst.
QUAD_REPROJECTION_PX = 2.72      # worst of 1000 random quads onto random quads in 1919 x 1079, float32 model, float64 evaluation
REFIT_AGAINST_LSTSQ = 1.09e-7    # worst coefficient difference to float64 lstsq over the 12 planted runs


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 5, 64, 1000])
def test_four_picks_are_distinct_in_range_and_independent_of_the_number_of_hypotheses(M):
    pos = HM.sample(7, 3, 500, 4, M)
    assert pos.shape == (500, 4) and pos.min() >= 0 and pos.max() < M
    assert all(len(set(r)) == 4 for r in pos.tolist())
    assert np.array_equal(HM.sample(7, 3, 37, 4, M), pos[:37])
    if M == 4:
        assert (np.sort(pos, 1) == np.arange(4)).all()
    else:
        assert len({tuple(r) for r in pos.tolist()}) > 100, "the samples vary"


@pytest.mark.parametrize("M", [4, 5, 64, 1000])
def test_four_picks_equal_popping_the_rth_of_the_remaining(M):
    pos = HM.sample(11, 2 ** 32 - 1, 200, 4, M)
    for h in range(200):
        left, want = list(range(M)), []
        for j in range(4):
            want.append(left.pop(int(HM.draw(11, 2 ** 32 - 1, h, j)) % (M - j)))
        assert pos[h].tolist() == want, h


@pytest.mark.parametrize("m", [1, 2, 3])
def test_smaller_samples_are_the_motion_fit_s(m):
    for M in (m, 5, 64, 1000):
        assert np.array_equal(HM.sample(5, 9, 300, m, M), MM.sample(5, 9, 300, m, M))
        assert np.array_equal(HM.sample(5, 9, 300, 4, max(M, 4))[:, :m], MM.sample(5, 9, 300, m, max(M, 4))), "a prefix of four picks"


# ---------------------------------------------------------------------------------------------------------------------
# the minimal solve
# ---------------------------------------------------------------------------------------------------------------------
def _solve(p, q):
    c, bad = HM.minimal(np.asarray(p, np.float64)[None], np.asarray(q, np.float64)[None])
    return c[0], bool(bad[0])


def test_exact_quads_come_back_equal():
    unit = [(0, 0), (1, 0), (1, 1), (0, 1)]
    c, bad = _solve(unit, [(5, -7), (8, -7), (8, -4), (5, -4)])          # scale 3, translation (5, -7)
    assert not bad and (c == np.float32([3, 0, 5, 0, 3, -7, 0, 0, 1])).all()
    # [2 0 1; 0 2 3; 1/2 0 1] on the square of side 2: w = 1, 2, 2, 1, every image dyadic
    sq = [(0, 0), (2, 0), (2, 2), (0, 2)]
    h = np.array([2, 0, 1, 0, 2, 3, 0.5, 0, 1])
    img = HM.apply(h, sq)
    assert img.tolist() == [[1, 3], [2.5, 1.5], [2.5, 3.5], [1, 7]]
    c, bad = _solve(sq, img)
    assert not bad and (c == h.astype(np.float32)).all() and c[8] == 1.0
    for roll in range(1, 4):   # the pick order does not matter to an exact case
        c2, bad = _solve(np.roll(sq, roll, 0), np.roll(img, roll, 0))
        assert not bad and (c2 == c).all()


def test_random_quads_map_onto_their_targets():
    """the worst reprojection of the four points, in pixels: the float32 model evaluated in float64"""
    rng = np.random.default_rng(0)
    p = (rng.random((1000, 4, 2)) * [1919.0, 1079.0]).astype(np.float32).astype(np.float64)
    q = (rng.random((1000, 4, 2)) * [1919.0, 1079.0]).astype(np.float32).astype(np.float64)
    c, bad = HM.minimal(p, q)
    assert not bad.any() and (c[:, 8] == 1.0).all()
    err = np.array([np.abs(HM.apply(c[i], p[i]) - q[i]).max() for i in range(1000)])
    print(f"random quads: worst {err.max():.4g} px, median {np.median(err):.3g} px, 99th percentile {np.percentile(err, 99):.3g} px")
    assert err.max() <= 4 * QUAD_REPROJECTION_PX
    # quads under the planted homography, as a sample of a real scene is: the rounding of the model to float32 is all there is
    qp = HM.apply(HM.planted_homography(), p).astype(np.float32).astype(np.float64)
    c, bad = HM.minimal(p, qp)
    errp = np.array([np.abs(HM.apply(c[i], p[i]) - qp[i]).max() for i in range(1000)])
    print(f"planted quads: worst {errp.max():.4g} px")
    assert not bad.any() and errp.max() <= 4 * QUAD_REPROJECTION_PX


def test_degenerate_samples():
    sq = np.array([(0, 0), (2, 0), (2, 2), (0, 2)], np.float64)
    assert _solve(sq, sq)[1] is False
    same = np.tile([[3.0, 4.0]], (4, 1))
    assert _solve(same, sq)[1] and _solve(sq, same)[1]
    # Three collinear points of four.  When they are picks 1, 2 and 3 the denominator is zero; in another order the
    # square-to-quad matrix is singular without a zero denominator, and the hypothesis is then either degenerate or a
    # rank-deficient model that does not even map its own four points: it scores, and cannot win against a good sample
    line3 = np.array([(0, 5), (0, 0), (1, 1), (2, 2)], np.float64)
    assert _solve(line3, sq)[1] and _solve(sq, line3)[1]
    for roll in range(1, 4):
        for p, q in ((np.roll(line3, roll, 0), np.roll(sq, roll, 0)), (np.roll(sq, roll, 0), np.roll(line3, roll, 0))):
            c, bad = _solve(p, q)
            with np.errstate(all="ignore"):
                assert bad or not (np.abs(HM.apply(c, p) - q).max() < 1.0), roll
    assert _solve(sq * 1e200, sq)[1], "not finite after the rounding"


# ---------------------------------------------------------------------------------------------------------------------
# planted scenes and the refit
# ---------------------------------------------------------------------------------------------------------------------
_planted = {}


def _planted_run(N, share, hyps, seed):
    """one run of the committed model per (scene, seed), shared by the tests"""
    key = (N, seed)
    if key not in _planted:
        src, dst, inl = HM.planted_scene(N, share, seed)
        d = {}
        _planted[key] = (src, dst, inl, HM.estimate(src, dst, None, hyps, 1.0, 0, 0, d), d)
    return _planted[key]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("N,share,hyps", HM.PLANTED)
def test_planted_scenes_recover_the_planted_set_and_the_lstsq_coefficients(N, share, hyps, seed):
    src, dst, planted, (model, mask, counts), d = _planted_run(N, share, hyps, seed)
    assert counts.tolist() == [int(planted.sum()), N, 1] and model[8] == 1.0
    assert np.array_equal(mask.astype(bool), planted), "the returned mask is the planted inlier set"
    ref = HM.lstsq_fit(src[:, 0], src[:, 1], dst[:, 0], dst[:, 1], d["best_inliers"])
    diff = np.abs(model.astype(np.float64) - ref).max()
    cond = np.linalg.cond(d["G"][:, :8])
    print(f"N={N} seed={seed}: refit - lstsq {diff:.3g}, to the planted coefficients {np.abs(model - HM.planted_homography()).max():.3g}, "
          f"condition of the normal matrix {cond:.3g}")
    assert diff <= 4 * REFIT_AGAINST_LSTSQ
    assert cond < 100, "the normalisation keeps the normal matrix well conditioned"


def test_the_normal_equations_are_those_of_the_design_matrix():
    src, dst, planted, _, d = _planted_run(*HM.PLANTED[1], 0)
    x, y, u, v = (a[d["best_inliers"]] for a in d["xyuv"])
    k = len(x)
    A = np.zeros((2 * k, 8))
    A[:k, 0], A[:k, 1], A[:k, 2], A[:k, 6], A[:k, 7] = x, y, 1.0, -x * u, -y * u
    A[k:, 3], A[k:, 4], A[k:, 5], A[k:, 6], A[k:, 7] = x, y, 1.0, -x * v, -y * v
    b = np.concatenate([u, v])
    G = d["G"]
    assert np.allclose(G[:, :8], A.T @ A, rtol=1e-12, atol=1e-12) and np.allclose(G[:, 8], A.T @ b, rtol=1e-12, atol=1e-12)
    assert np.array_equal(G[:, :8], G[:, :8].T)
    h, ok = HM.solve8(G)
    assert ok and np.allclose(h, np.linalg.solve(G[:, :8], G[:, 8]), rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def _edge(name):
    e = [c for c in HM.edge_cases() if c[0] == name]
    assert len(e) == 1, name
    return e[0]


def _run(e, seed=1, index=3, detail=None):
    _, src, dst, valid, hyps, thr = e
    return HM.estimate(src, dst, valid, hyps, thr, seed, index, detail)


def _failed(r, N, M):
    return np.isnan(r[0]).all() and r[0].shape == (9,) and not r[1].any() and r[1].shape == (N,) and r[2].tolist() == [0, M, 0]


def test_fewer_than_four_valid_correspondences():
    for M in range(4):
        assert _failed(_run(_edge(f"M={M}<4")), 5, M), M


def test_every_hypothesis_degenerate():
    for name, N in (("identical points", 9), ("collinear points", 10)):
        d = {}
        assert _failed(_run(_edge(name), detail=d), N, N), name
        assert (d["score"] == -1).all()


def test_collinear_triples_in_some_samples_do_not_stop_the_good_ones():
    d = {}
    model, mask, counts = _run(_edge("collinear triples in the samples"), detail=d)
    assert (d["score"] == -1).any() and (d["score"] == 30).any() and counts.tolist() == [30, 30, 1]
    assert np.abs(model - np.float32([1, 0, 2, 0, 1, 1, 0, 0, 1])).max() < 1e-6


def test_an_exact_scene_ties_the_good_scores_and_the_lowest_hypothesis_wins():
    d = {}
    model, mask, counts = _run(_edge("exact integer scene"), detail=d)
    assert counts.tolist() == [40, 40, 1] and mask.all()
    assert d["best"] == int(np.flatnonzero(d["score"] == d["score"].max())[0])
    assert np.abs(model - np.float32([2, -1, 3, 1, 2, -4, 0, 0, 1])).max() < 1e-5 and model[8] == 1.0


def test_a_residual_exactly_on_the_threshold_is_an_inlier():
    e = _edge("residual on the threshold")
    d = {}
    model, mask, counts = _run(e, detail=d)
    exact = np.float32([1, 0, 2, 0, 1, 1, 0, 0, 1])
    _, src, dst, _, _, thr = e
    on = HM.inlier_test(exact, src[:, 0], src[:, 1], dst[:, 0], dst[:, 1], np.float32(thr) * np.float32(thr))
    assert on.all(), "(3, 4) off at threshold 5: r2 == 25 <= 25"
    assert not HM.inlier_test(exact, src[7, 0], src[7, 1], dst[7, 0], dst[7, 1], np.float32(24.999998))
    assert d["score"].max() == 30 and counts[2] == 1


def test_nan_and_inf_coordinates_are_invalid_without_a_mask():
    e = _edge("NaN and inf coordinates")
    model, mask, counts = _run(e)
    bad = [3, 11, 4, 20, 21]
    assert counts.tolist() == [25, 25, 1] and not mask[bad].any() and mask.sum() == 25 and np.isfinite(model).all()


def test_points_behind_the_camera_are_no_inliers():
    e = _edge("w <= 0 at valid points")
    _, src, dst, _, _, thr = e
    model, mask, counts = _run(e)
    front = src[:, 0] < 16
    assert counts.tolist() == [int(front.sum()), len(src), 1] and np.array_equal(mask.astype(bool), front)
    w = (model[6] * src[:, 0] + model[7] * src[:, 1]) + model[8]
    assert (w[~front] < 0).all() and (w[front] > 0).all()
    # the far side reprojects within the threshold all the same: only the sign of w keeps it out
    assert (np.abs(HM.apply(model, src[~front]) - dst[~front]).max(-1) < thr).all()


def test_tracks_are_the_steps_of_consecutive_rows():
    rng = np.random.default_rng(3)
    tr = np.stack([HM.planted_scene(30, 0.2, 40 + t)[0] for t in range(4)])
    vis, born = rng.random((4, 30)) < 0.9, rng.random((4, 30)) < 0.1
    got = HM.tracks(tr, vis, born, 16, 1.0, 2, 5)
    for t in range(3):
        want = HM.estimate(tr[t], tr[t + 1], vis[t] & vis[t + 1] & ~born[t + 1], 16, 1.0, 2, 5 + t)
        HM.same(tuple(g[t] for g in got), want, f"step {t}")


# ---------------------------------------------------------------------------------------------------------------------
# the perspective warp
# ---------------------------------------------------------------------------------------------------------------------
def _frames(F, H, W, dtype, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.random((F, H, W)) * 255
    return np.rint(f).astype(np.uint8) if dtype == np.uint8 else f.astype(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_the_warp_under_the_identity_and_under_affine_maps(dtype):
    fr = _frames(3, 9, 14, dtype)
    ident = np.tile(np.eye(3).reshape(9), (3, 1))
    out, ins = HM.warp(fr, ident)
    assert np.array_equal(out, fr) and ins.all() and out.dtype == fr.dtype
    aff = np.array([[1.01, -0.03, 0.6, 0.02, 0.99, -0.4], [1, 0, 2, 0, 1, -1], [0.5, 0.25, 1.125, -0.25, 0.5, 3.0]])
    maps = np.concatenate([aff, np.tile([0.0, 0.0, 1.0], (3, 1))], 1)
    want = SM.warp(fr, aff)
    got = HM.warp(fr, maps)
    SM.same(got[0], want[0], "samples")
    SM.same(got[1], want[1], "inside")
    assert 0 < got[1].sum() < got[1].size


def test_the_warp_where_w_changes_sign_and_under_a_nan():
    fr = _frames(1, 8, 12, np.float32) + 1
    m = np.array([1, 0, 0, 0, 1, 0, -0.2, 0, 1.0])   # w = 1 - x / 5: zero at x = 5, negative beyond
    out, ins = HM.warp(fr, m[None])
    assert not ins[0][:, 5:].any() and (out[0][:, 5:] == 0).all() and ins[0][:, 0].all()
    xs, ys, w = HM.coordinates(m, 8, 12)
    assert (w[:, 6:] < 0).all() and w[0, 5] == 0 and np.array_equal(ins[0], (w > 0) & (xs <= 11) & (ys <= 7))
    m[4] = np.nan
    out, ins = HM.warp(fr, m[None])
    assert not ins.any() and (out == 0).all()
    out, ins = HM.warp(fr, np.array([[2, 0, 0, 0, 2, 0, 0, 0, 2.0]]))   # m8 = 2: the identity again
    assert np.array_equal(out, fr) and ins.all()


# ---------------------------------------------------------------------------------------------------------------------
# the library and the wrappers, without a device
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ["oflk_homography_workspace", "oflk_estimate_homography", "oflk_tracks_homography", "oflk_estimate_homography_host",
           "oflk_warp_perspective", "oflk_warp_perspective_host", "oflk_warp_perspective_host_u8"]


def test_the_library_exports_the_entry_points():
    import _oflk

    L = _oflk.lib()
    for name in SYMBOLS:
        assert name in _oflk.SIGNATURES and hasattr(L, name), name


def test_the_workspace_size_covers_its_pieces():
    import _oflk

    for S, N, Hn in [(1, 1, 1), (3, 65, 257), (1, 10000, 1024), (7, 1000, 64)]:
        need = S * 4 + S * N * 16 + S * Hn * 4 + S * Hn * 36
        got = _oflk.homography_workspace(S, N, Hn)
        assert need <= got <= need + 4 * 256 and got % 256 == 0
        assert got >= _oflk.motion_workspace(S, N, Hn)


def test_refusals_come_before_any_device_call():
    """every refusal is decided on the host: this runs without a GPU, with pointers that are never dereferenced"""
    import _oflk

    L = _oflk.lib()
    P, WS = 0x10000, 0x20000   # 8-byte and 256-byte aligned addresses, never read
    n = ctypes.c_size_t(0)
    big = 1 << 40
    INVALID, UNSUPPORTED = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED

    def est(src=P, dst=P, valid=None, S=2, N=10, step0=0, hyps=16, thr=1.0, seed=0, ws=WS, ws_bytes=big, out=P, inl=P, cnt=P):
        return L.oflk_estimate_homography(src, dst, valid, S, N, step0, hyps, thr, seed, ws, ws_bytes, out, inl, cnt, None)

    def trk(tracks=P, vis=P, born=None, T=3, K=10, t0=0, hyps=16, thr=1.0, seed=0, ws=WS, ws_bytes=big, out=P, inl=P, cnt=P):
        return L.oflk_tracks_homography(tracks, vis, born, T, K, t0, hyps, thr, seed, ws, ws_bytes, out, inl, cnt, None)

    need = _oflk.homography_workspace(2, 10, 16)
    assert need > _oflk.motion_workspace(2, 10, 16)
    bad = [dict(hyps=0), dict(hyps=-1), dict(hyps=HM.MAX_HYPOTHESES + 1), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
           dict(thr=float("inf")), dict(ws=None), dict(ws=WS + 8), dict(ws_bytes=need - 1),
           dict(ws_bytes=_oflk.motion_workspace(2, 10, 16)), dict(out=None), dict(inl=None), dict(cnt=None)]
    for kw in bad + [dict(S=0), dict(N=0), dict(src=None), dict(dst=None), dict(src=P + 4), dict(dst=P + 4)]:
        assert est(**kw) == INVALID, kw
        assert L.oflk_last_error()
    for kw in bad + [dict(T=1), dict(K=0), dict(tracks=None), dict(vis=None), dict(tracks=P + 4)]:
        assert trk(**kw) == INVALID, kw
    f = np.zeros((2, 10, 2), np.float32)
    out, inl, cnt = np.zeros((2, 9), np.float32), np.zeros((2, 10), np.uint8), np.zeros((2, 3), np.int32)

    def host(src=f, S=2, N=10, hyps=16, thr=1.0, out=out, inl=inl, cnt=cnt):
        return L.oflk_estimate_homography_host(None if src is None else _oflk.ptr(src), _oflk.ptr(f), None, S, N, 0, hyps, thr, 0,
                                               None if out is None else _oflk.ptr(out), None if inl is None else inl.ctypes.data,
                                               None if cnt is None else cnt.ctypes.data_as(_oflk._i32p))

    for kw in [dict(src=None), dict(S=0), dict(N=-1), dict(hyps=0), dict(hyps=HM.MAX_HYPOTHESES + 1), dict(thr=0.0),
               dict(thr=float("inf")), dict(out=None), dict(inl=None), dict(cnt=None)]:
        assert host(**kw) == INVALID, kw
    for args in [(0, 10, 16), (2, 0, 16), (2, 10, 0), (2, 10, HM.MAX_HYPOTHESES + 1)]:
        assert L.oflk_homography_workspace(*args, ctypes.byref(n)) == INVALID
    assert L.oflk_homography_workspace(2, 10, 16, None) == INVALID

    def warp(frames=P, u8=0, F=2, H=8, W=8, maps=P, out=WS, inside=None):
        return L.oflk_warp_perspective(frames, u8, F, H, W, maps, out, inside, None)

    for kw in [dict(F=0), dict(H=1), dict(W=1), dict(frames=None), dict(maps=None), dict(out=None), dict(maps=P + 4),
               dict(frames=P + 2), dict(out=WS + 2)]:
        assert warp(**kw) == INVALID, kw
    assert warp(frames=P + 2, out=WS + 2, u8=1, F=0) == INVALID
    assert warp(H=1 << 15, W=1 << 15) == UNSUPPORTED and warp(H=1 << 15, W=1 << 15, u8=1) == UNSUPPORTED
    fr, m = np.zeros((1, 4, 4), np.float32), np.zeros((1, 9))
    fp, mp = _oflk.ptr(fr), m.ctypes.data_as(_oflk._f64p)
    for fn, a in ((L.oflk_warp_perspective_host, fp), (L.oflk_warp_perspective_host_u8, fr.ctypes.data)):
        for args in [(None, 1, 4, 4, mp, a, None), (a, 0, 4, 4, mp, a, None), (a, 1, 1, 4, mp, a, None), (a, 1, 4, 1, mp, a, None),
                     (a, 1, 4, 4, None, a, None), (a, 1, 4, 4, mp, None, None)]:
            assert fn(*args) == INVALID, args
        assert fn(a, 1, 1 << 15, 1 << 15, mp, a, None) == UNSUPPORTED


def test_python_arguments_are_checked_before_the_library_is_asked():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    p = np.zeros((5, 2), np.float32)
    for kw in [dict(hypotheses=0), dict(hypotheses=2.5), dict(hypotheses=True), dict(hypotheses=HM.MAX_HYPOTHESES + 1), dict(threshold=0),
               dict(threshold=float("nan")), dict(seed=-1), dict(seed=2 ** 32), dict(step0=-1), dict(step0=2 ** 31)]:
        with pytest.raises(ValueError):
            K.estimate_homography(p, p, **kw)
    with pytest.raises(TypeError):
        K.estimate_homography(p, p, model="homography")   # the family is the call
    for a, b, v in [(p, p[:4], None), (p[:, :1], p[:, :1], None), (p, p, np.ones(4)), (p[:0], p[:0], None), (p[None, None], p[None, None], None)]:
        with pytest.raises(ValueError):
            K.estimate_homography(a, b, v)
    with pytest.raises(ValueError):
        K.tracks_homography(p[None], np.ones((1, 5)))   # T < 2
    with pytest.raises(ValueError):
        K.tracks_homography(np.zeros((3, 5, 2)), np.ones((3, 4)))
    with pytest.raises(ValueError):
        K.tracks_homography(np.zeros((3, 5, 2)), np.ones((3, 5)), np.ones((2, 5)))
    fr = np.zeros((2, 6, 7), np.float32)
    for frames, maps in [(fr, np.eye(3)), (fr, np.zeros((2, 6))), (fr, np.zeros((3, 3, 3))), (fr, np.zeros((2, 2, 3))), (fr, np.zeros(18)[None, None, None]),
                         (fr[:, :1], np.zeros((2, 3, 3))), (fr[:, :, :1], np.zeros((2, 3, 3))), (fr[0], np.zeros((3, 6)))]:
        with pytest.raises(ValueError):
            K.warp_perspective(frames, maps)
    assert P.estimate_homography is K.estimate_homography and P.tracks_homography is K.tracks_homography
    assert P.warp_perspective is K.warp_perspective and P.Homography is K.Homography
