"""CPU tests of the sparse pyramidal LK statement (tests/sparse_model.py), of the sparse entry points' refusals and of their
Python shims' argument checks.  Nothing here touches a device."""
import numpy as np
import pytest

import fb_model as FM
import sparse_model as S
import track_model as TM


# ---------------------------------------------------------------------------------------------------------------
# the statement is the reference's arithmetic
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [3, 5, 7, 9, 11])
def test_centre_value_is_the_oracles_centre_pixel(oracle, w):
    """the mosaic route and the oracle on each (w+2)^2 patch by itself give the same bytes: random patches, a flat patch
    (det fails: no solution, zero update) and an 8-bit patch"""
    rng = np.random.default_rng(w)
    M = 41
    P = (rng.random((M, w + 2, w + 2)) * 255).astype(np.float32)
    Q = (P + rng.standard_normal(P.shape) * 4).astype(np.float32)
    P[5] = Q[5] = np.float32(93.0)                      # flat
    P[6], Q[6] = np.rint(P[6]), np.rint(Q[6])           # 8-bit values
    P[7] = Q[7]                                         # identical patches: solved, zero update
    du, dv, solved = S.centre_flow(P, Q, w)
    c = w // 2 + 1
    for m in range(M):
        u, v = oracle.lucas_kanade_single_scale(P[m], Q[m], w)
        assert u[c, c].tobytes() == du[m].tobytes() and v[c, c].tobytes() == dv[m].tobytes(), (w, m)
        ou, ov, osolved = S.centre_flow_one(P[m], Q[m], w)
        assert (ou.tobytes(), ov.tobytes(), osolved) == (du[m].tobytes(), dv[m].tobytes(), bool(solved[m])), (w, m)
    assert not solved[5] and du[5] == 0 and dv[5] == 0
    assert solved[7] and du[7] == 0 and dv[7] == 0
    assert solved.sum() >= M - 1 and np.abs(du).max() > 0


def test_row_sums_are_np_sum_of_each_row():
    """the model sums (M, n) arrays along axis 1; that is np.sum of each contiguous row (pairwise, eight accumulators)"""
    rng = np.random.default_rng(2)
    for n in (9, 25, 49, 81, 121):
        a = (rng.standard_normal((64, n)) * 1e3).astype(np.float32)
        rows = np.sum(a, axis=1)
        assert all(rows[i].tobytes() == np.sum(np.ascontiguousarray(a[i])).tobytes() for i in range(64)), n


def _drifting(T, H, W, seed):
    from scipy.ndimage import gaussian_filter, shift

    rng = np.random.default_rng(seed)
    base = gaussian_filter(rng.random((H + 16, W + 16)) * 255.0, 1.5)
    base = (base - base.min()) / (base.max() - base.min()) * 220.0 + 15.0
    return np.stack([shift(base, (0.6 * t, -0.9 * t), order=1, mode="nearest")[8:8 + H, 8:8 + W] +
                     rng.normal(0, 1.0, (H, W)) for t in range(T)]).astype(np.float32)


def test_pieces_equal_one_call():
    """positions are float32 between steps: the model run in pieces cut at every possible pair, each piece carrying the
    previous piece's last row, gives the tracks of one call"""
    T, H, W = 5, 40, 52
    frames = _drifting(T, H, W, 3)
    rng = np.random.default_rng(4)
    N = 120
    qxy = (rng.random((N, 2)) * [W - 1, H - 1]).astype(np.float32)
    qxy[:4] = [[0, 0], [W - 1, H - 1], [-1, 3], [np.nan, 2]]
    qt = rng.integers(0, T, N)
    qt[::2] = 0
    pyr = [S.pyramid(f, 3) for f in frames]
    one = S.track(frames, qt, qxy, 3, 5, 3, pyramids=pyr)
    assert one[1][0].sum() > 40 and one[1][-1].sum() > 40 and one[1][-1].sum() < N
    for cut in range(1, T - 1):
        a = S.track(frames[:cut + 1], qt, qxy, 3, 5, 3, pyramids=pyr[:cut + 1])
        b = S.track(frames[cut:], qt, qxy, 3, 5, 3, t0=cut, prev=(a[0][-1], a[1][-1]), pyramids=pyr[cut:])
        tr, vis = np.concatenate([a[0], b[0][1:]]), np.concatenate([a[1], b[1][1:]])
        assert np.array_equal(vis, one[1]) and np.array_equal(tr.view(np.int32), one[0].view(np.int32)), cut
        # row 0 of the second piece: the first piece's last row, queries of frame `cut` started, later ones NaN
        assert np.array_equal(b[1][0], one[1][cut])


# ---------------------------------------------------------------------------------------------------------------
# meaning
# ---------------------------------------------------------------------------------------------------------------
def test_occluder_scene_meaning():
    T, Sc = 5, TM.SCENE
    frames, corners = FM.occluder_scene(T, Sc["H"], Sc["W"], Sc["size"], Sc["step"])
    pyr = [S.pyramid(f, 3) for f in frames]

    def run(q, max_residual=4.0):
        tr, vis = S.track(frames, q[:, 0].astype(np.int64), q[:, 1:], 3, 5, 3, 0.01, 0.5, max_residual, pyramids=pyr)
        return tr, vis.astype(bool)

    S.check_scene_sparse_tracks(run, T, corners, Sc["H"], Sc["W"], Sc["size"], Sc["step"],
                                run_no_residual=lambda q: run(q, np.inf))


SHIFTS = [(0.4, -0.3), (5.5, -2.25), (9.0, 4.0)]


def subpixel_case(dx, dy):
    """the two 8-bit frames and the 200 points of the motion test"""
    H, W = 96, 128
    rng = np.random.default_rng(100)
    pts = np.stack([rng.uniform(16, W - 17, 200), rng.uniform(16, H - 17, 200)], 1).astype(np.float32)
    return S.sinusoid_texture(H, W, 0, 0), S.sinusoid_texture(H, W, dx, dy), pts


def check_subpixel(nxt, status, pts, dx, dy):
    err = np.hypot(nxt[:, 0] - (pts[:, 0] + np.float32(dx)), nxt[:, 1] - (pts[:, 1] + np.float32(dy)))
    assert status.all()
    assert np.median(err) <= 0.1 and np.percentile(err, 90) <= 0.25, (dx, dy, np.median(err), np.percentile(err, 90))
    return float(np.median(err)), float(np.percentile(err, 90))


@pytest.mark.parametrize("dx,dy", SHIFTS)
def test_subpixel_and_large_motion(dx, dy):
    """a smooth 8-bit texture moved by (dx, dy), 96 x 128, 3/5/3, 200 points at least 16 px inside: median error <= 0.1 px,
    90th percentile <= 0.25 px.  The statement's values (median, 90th percentile): (0.4, -0.3): 0.034, 0.098;
    (5.5, -2.25): 0.041, 0.097; (9, 4): 0.0002, 0.001 -- the 8-bit rounding, not the solver (a whole-pixel shift of the
    analytic texture rounds to the same bytes, so its error is the solver's alone)."""
    a, b, pts = subpixel_case(dx, dy)
    nxt, status, _ = S.sparse_lk(a, b, pts, 3, 5, 3)
    check_subpixel(nxt, status.astype(bool), pts, dx, dy)


def test_constant_frames_solve_nothing():
    """identical frames never move a point (It = 0).  A frame of zeros has no gradient anywhere, so no system is solved:
    status 0 for every point inside.  A constant frame of another value has the gradient of its zero surround at the
    border (cval 0), and none in windows that stay inside"""
    pts = np.array([[3.0, 4.0], [10.5, 7.25], [31.0, 23.0], [0.0, 0.0], [40.0, 2.0]], np.float32)
    for value in (0.0, 80.0):
        f = np.full((24, 32), value, np.float32)
        nxt, status, res = S.sparse_lk(f, f, pts, 3, 5, 3)
        assert np.array_equal(nxt[:4], pts[:4]) and np.isnan(nxt[4]).all() and np.isnan(res[4]) and status[4] == 0
        assert not res[:4].any()
        assert not status[:2].any() and (value != 0.0 or not status.any())


# ---------------------------------------------------------------------------------------------------------------
# refusals, before any device call
# ---------------------------------------------------------------------------------------------------------------
def _c_sequence(T=3, H=24, W=32, L=3, w=5, K=3, alpha=0.01, beta=0.5, mr=4.0, N=2, null=None):
    import _oflk

    frames = np.zeros((max(T, 1), H, W), np.float32)
    qxy, tr, vis = np.zeros((max(N, 1), 2), np.float32), np.zeros((max(T, 1), max(N, 1), 2), np.float32), np.zeros((max(T, 1), max(N, 1)), np.uint8)
    args = dict(frames=_oflk.ptr(frames), qxy=_oflk.ptr(qxy), tracks=_oflk.ptr(tr), visible=vis.ctypes.data)
    if null:
        args[null] = None
    return _oflk.lib().oflk_pyramidal_sequence_sparse_tracks(args["frames"], T, H, W, L, w, K, alpha, beta, mr, None, args["qxy"], N,
                                                             args["tracks"], args["visible"])


def _c_pair(H=24, W=32, L=3, w=5, K=3, N=2, null=None, u8=False):
    import _oflk

    f = np.zeros((H, W), np.uint8 if u8 else np.float32)
    pts, nxt, st, res = np.zeros((max(N, 1), 2), np.float32), np.zeros((max(N, 1), 2), np.float32), np.zeros(max(N, 1), np.uint8), np.zeros(max(N, 1), np.float32)
    args = dict(prev=f.ctypes.data if u8 else _oflk.ptr(f), pts=_oflk.ptr(pts), nxt=_oflk.ptr(nxt), st=st.ctypes.data, res=_oflk.ptr(res))
    if null:
        args[null] = None
    fn = _oflk.lib().oflk_sparse_lk_u8 if u8 else _oflk.lib().oflk_sparse_lk
    return fn(args["prev"], args["prev"], H, W, L, w, K, args["pts"], N, args["nxt"], args["st"], args["res"])


INVALID, UNSUPPORTED = -1, -4


@pytest.mark.parametrize("kw,code", [
    (dict(H=7, W=9), UNSUPPORTED), (dict(H=3, W=3), UNSUPPORTED), (dict(H=1, W=40, L=1), UNSUPPORTED),
    (dict(w=1), UNSUPPORTED), (dict(w=4), UNSUPPORTED), (dict(w=13), UNSUPPORTED), (dict(w=0), UNSUPPORTED), (dict(w=-3), UNSUPPORTED),
    (dict(K=0), INVALID), (dict(K=-1), INVALID), (dict(L=0), INVALID), (dict(N=0), INVALID),
])
def test_c_entry_points_refuse_without_a_device(kw, code):
    assert _c_pair(**kw) == code, kw
    assert _c_pair(u8=True, **kw) == code, kw
    assert _c_sequence(**kw) == code, kw


@pytest.mark.parametrize("kw", [dict(T=1), dict(alpha=-1.0), dict(beta=float("nan")), dict(alpha=float("inf")), dict(mr=-0.5),
                                dict(mr=float("nan")), dict(null="frames"), dict(null="qxy"), dict(null="tracks"),
                                dict(null="visible")])
def test_sequence_entry_point_refuses_bad_arguments(kw):
    assert _c_sequence(**kw) == INVALID, kw


@pytest.mark.parametrize("null", ["prev", "pts", "nxt", "st", "res"])
def test_pair_entry_point_refuses_null_pointers(null):
    assert _c_pair(null=null) == INVALID


def test_plan_entry_point_refuses_a_null_plan():
    import _oflk

    assert _oflk.lib().oflk_plan_sparse_tracks(None, None, 0, 0.01, 0.5, 4.0, 0, None, None, 1, None, None, None) == INVALID


def test_shims_raise_value_error_before_any_device_call():
    import lucas_kanade_pyramidal as P

    f = np.zeros((24, 32), np.float32)
    pts = np.zeros((3, 2), np.float32)
    seq = np.zeros((3, 24, 32), np.float32)
    bad_pair = [dict(num_levels=0), dict(num_iterations=0), dict(window_size=4), dict(window_size=13), dict(window_size=1)]
    for kw in bad_pair:
        with pytest.raises(ValueError):
            P.lucas_kanade_sparse(f, f, pts, **kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_sparse_tracks(seq, pts, **kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_sparse(seq, 10, **kw)
    small = np.zeros((7, 9), np.float32)
    with pytest.raises(ValueError):
        P.lucas_kanade_sparse(small, small, pts)   # 7x9 at 3 levels: a level of width 1
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_sparse_tracks(np.zeros((3, 7, 9), np.float32), pts)
    for kw in (dict(max_residual=-1.0), dict(max_residual=float("nan")), dict(alpha=-0.1), dict(beta=float("inf"))):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_sparse_tracks(seq, pts, **kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_sparse(seq, 10, **kw)
    for bad_pts in (np.zeros((0, 2)), np.zeros((3, 3)), np.zeros(4)):
        with pytest.raises(ValueError):
            P.lucas_kanade_sparse(f, f, bad_pts)
    with pytest.raises(ValueError):
        P.lucas_kanade_sparse(f, np.zeros((24, 33), np.float32), pts)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_sparse_tracks(seq[:1], pts)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_sparse_tracks(seq, np.array([[5, 1.0, 1.0]]))   # query frame outside [0, T-1]
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_klt_sparse(seq, 0)
    with pytest.raises(ValueError):
        S.check_config((7, 9), 3, 5, 3)
