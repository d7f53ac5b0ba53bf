"""CPU tests of the replenished-KLT statement (tests/replenish_model.py), of split_tracks and of the new C ABI surface.
Nothing here touches a device."""
import numpy as np
import pytest

import feature_model as FM
import replenish_model as M
import track_model as TM

MDS = [0.0, 0.5, 1.0, 1.5, 7.0, 10.0, 300.0, 1e9]
SYMBOLS = ["oflk_pyramidal_sequence_klt_replenish", "oflk_pyramidal_sequence_klt_replenish_u8", "oflk_replenish_features",
           "oflk_replenish_features_workspace", "oflk_replenish_features_host", "oflk_replenish_features_host_u8"]


def score_map(H, W, seed, levels=12):
    """a random score map with many ties (few distinct values), zeros included"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (H, W)) * rng.integers(0, 2, (H, W))).astype(np.float32)


def slots(K, H, W, seed, kind):
    """(xy (K, 2) float32, visible (K,) bool) of one kind of slot state"""
    rng = np.random.default_rng(seed)
    xy = (rng.random((K, 2)) * [W - 1, H - 1]).astype(np.float32)
    vis = rng.random(K) < 0.6
    if kind == "none_free":
        vis[:] = True
    elif kind == "all_free":
        vis[:] = False
    elif kind == "stacked":   # more than four seeds in one cell, several on one pixel
        xy[:K // 2] = (W // 2, H // 2)
        xy[K // 2:3 * K // 4] = np.float32([W // 2, H // 2]) + rng.integers(-1, 2, (3 * K // 4 - K // 2, 2))
        vis[:3 * K // 4] = True
    elif kind == "border":
        xy[0::4, 0], xy[1::4, 0], xy[2::4, 1], xy[3::4, 1] = 0, W - 1, 0, H - 1
    elif kind == "half":   # x.5 positions of both parities: rint goes to the even neighbour
        xy = (np.floor(xy) + 0.5).astype(np.float32)
        xy = np.minimum(xy, np.float32([W - 1.5, H - 1.5]))
    xy[~vis] = np.nan
    return xy, vis


KINDS = ["some", "none_free", "all_free", "stacked", "border", "half"]


def brute(S, xy, vis, q, md):
    """the statement without a grid: every candidate against every seed and every accepted point"""
    H, W = S.shape
    free = np.flatnonzero(~vis)
    md32 = float(np.float32(md))
    sx, sy = M.seeds_of(xy, vis, H, W)
    taken = list(zip(sx.tolist(), sy.tolist())) if md32 > 0 else []
    ys, xs, _ = FM.candidates(S, q)
    pts = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        if len(pts) == len(free):
            break
        if any(float((px - x) ** 2 + (py - y) ** 2) < md32 * md32 for px, py in taken):
            continue
        taken.append((x, y))
        pts.append((x, y))
    return free[:len(pts)], np.array(pts, np.float32).reshape(-1, 2)


def delete_then_select(S, xy, vis, q, md):
    """feature_model's candidates (of the unmasked S), those within md of a seed deleted, the plain greedy on the rest"""
    H, W = S.shape
    free = np.flatnonzero(~vis)
    md32 = float(np.float32(md))
    sx, sy = M.seeds_of(xy, vis, H, W)
    ys, xs, _ = FM.candidates(S, q)
    keep = np.ones(len(ys), bool)
    if md32 > 0 and len(sx):
        d2 = (xs[:, None] - sx[None]) ** 2 + (ys[:, None] - sy[None]) ** 2
        keep = ~(d2.astype(np.float64) < md32 * md32).any(1)
    pts = []
    for y, x in zip(ys[keep].tolist(), xs[keep].tolist()):
        if len(pts) == len(free):
            break
        if any(float((px - x) ** 2 + (py - y) ** 2) < md32 * md32 for px, py in pts):
            continue
        pts.append((x, y))
    return free[:len(pts)], np.array(pts, np.float32).reshape(-1, 2)


def _equal(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: slots"
    assert a[1].tobytes() == b[1].tobytes(), f"{what}: points"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("md", MDS, ids=lambda v: f"md{v:g}")
def test_detect_equals_brute_force_and_delete_then_select(md, kind):
    for seed, (H, W, K) in enumerate([(24, 31, 40), (40, 37, 12), (9, 50, 300)]):
        S = score_map(H, W, 100 + seed)
        xy, vis = slots(K, H, W, 7 * seed + KINDS.index(kind), kind)
        for q in (0.0, 0.3):
            got = M.detect(S, xy, vis, q, md)
            _equal(got, brute(S, xy, vis, q, md), f"brute {H}x{W} q={q}")
            _equal(got, delete_then_select(S, xy, vis, q, md), f"delete-then-select {H}x{W} q={q}")
            assert len(got[0]) <= (~vis).sum()
            if kind == "none_free":
                assert len(got[0]) == 0


def test_seeds_round_half_to_even_and_refuse_their_own_pixel():
    """seeds at x.5: 2.5 -> 2 and 3.5 -> 4 (both parities); with 0 < md <= 1 exactly the seed's own pixel is refused, with
    md = 0 nothing is"""
    S = np.zeros((9, 12), np.float32)
    S[4, 2], S[4, 3], S[4, 4], S[6, 8] = 5, 4, 3, 2   # (y, x)
    xy = np.float32([[2.5, 4.0], [3.5, 4.0], [np.nan, np.nan], [np.nan, np.nan], [np.nan, np.nan]])
    vis = np.array([1, 1, 0, 0, 0], bool)
    sx, sy = M.seeds_of(xy, vis, 9, 12)
    assert sx.tolist() == [2, 4] and sy.tolist() == [4, 4]
    S2 = S.copy()
    S2[4, 3] = 0   # (4, 2) and (4, 4) are local maxima now
    for md, want in ((0.0, [(2, 4), (4, 4), (8, 6)]), (0.5, [(8, 6)]), (1.0, [(8, 6)])):
        sl, pts = M.detect(S2, xy, vis, 0.0, md)
        assert pts.tolist() == [list(map(float, p)) for p in want], (md, pts)
        assert sl.tolist() == [2, 3, 4][:len(want)]
    _equal(M.detect(S2, xy, vis, 0.0, 1.5), brute(S2, xy, vis, 0.0, 1.5), "md 1.5")


def test_candidates_and_max_come_from_the_unmasked_map():
    """a seed on the frame's strongest corner: the threshold stays q * M of the whole frame, so zeroing S near the seed
    first (which would lower M and admit the weak corner) is not the statement"""
    S = np.zeros((20, 30), np.float32)
    S[5, 5], S[12, 20], S[15, 8] = 100, 40, 5
    xy, vis = np.float32([[5, 5], [np.nan, np.nan], [np.nan, np.nan]]), np.array([1, 0, 0], bool)
    sl, pts = M.detect(S, xy, vis, 0.1, 3.0)
    assert pts.tolist() == [[20.0, 12.0]] and sl.tolist() == [1]
    masked = S.copy()
    masked[3:8, 3:8] = 0
    assert len(M.detect(masked, xy, vis, 0.1, 3.0)[1]) == 2


@pytest.mark.parametrize("md", MDS, ids=lambda v: f"md{v:g}")
def test_no_seeds_and_all_free_is_the_plain_selection(md):
    S = score_map(33, 41, 5)
    for K in (1, 17, 5000):
        xy, vis = np.full((K, 2), np.nan, np.float32), np.zeros(K, bool)
        sl, pts = M.detect(S, xy, vis, 0.2, md)
        n, wxy, _ = FM.select(S, 0.2, md, K)
        assert sl.tolist() == list(range(n)) and pts.tobytes() == wxy[:n].tobytes()


def test_md_beyond_the_diagonal_one_alive_slot_removes_every_candidate():
    S = score_map(30, 40, 9)
    xy, vis = slots(20, 30, 40, 3, "all_free")
    xy[7], vis[7] = (39.0, 29.0), True
    for md in (51.0, 300.0, 1e9):
        assert len(M.detect(S, xy, vis, 0.0, md)[0]) == 0
    assert len(M.detect(S, xy, vis, 0.0, 10.0)[0]) > 0


def _scores_from(maps):
    return lambda t: maps[t]


def test_sequence_without_replenishing_is_detection_then_tracks():
    T, H, W, K = 7, 40, 50, 60
    flows = TM.smooth_flows(T - 1, H, W, seed=3, scale=4.0)
    maps = [score_map(H, W, 50 + t, levels=200) for t in range(T)]
    for D in (T, T + 5, 10 ** 6):
        tr, vis, born, det = M.sequence(_scores_from(maps), flows, K, D, 0.1, 4.0)
        n, xy, _ = FM.select(maps[0], 0.1, 4.0, K)
        wtr, wvis = TM.track(*flows, None, xy)
        assert np.array_equal(vis, wvis) and np.array_equal(np.isnan(tr), np.isnan(wtr))
        assert np.nan_to_num(tr).tobytes() == np.nan_to_num(wtr).tobytes()
        assert np.array_equal(born[0], vis[0]) and not born[1:].any()
        assert det.tolist() == [n] + [0] * (T - 1) and 0 < n
        assert not vis[-1].all(), "some tracks should end on these flows"


@pytest.mark.parametrize("D", [1, 2, 3, 5])
def test_sequence_equals_itself_cut_in_two_and_keeps_its_invariants(D):
    T, H, W, K, md = 9, 40, 50, 40, 5.0
    flows = TM.smooth_flows(T - 1, H, W, seed=11, scale=5.0)
    maps = [score_map(H, W, 70 + t, levels=200) for t in range(T)]
    whole = M.sequence(_scores_from(maps), flows, K, D, 0.05, md)
    for cut in range(1, T - 1):
        parts = M.sequence_in_two(_scores_from(maps), flows, K, D, cut, quality_level=0.05, min_distance=md)
        for a, b, name in zip(whole, parts, ("tracks", "visible", "born", "detected")):
            assert np.array_equal(a, b, equal_nan=True), (name, cut)
    check_invariants(*whole, D, md)
    tr, vis, born, det = whole
    if D < T - 1:
        assert born[1:].any(), "ended tracks should be replaced"


def check_invariants(tracks, visible, born, detected, D, md):
    """what holds for every output of the statement, read from the outputs alone"""
    vis, born = np.asarray(visible).astype(bool), np.asarray(born).astype(bool)
    T = vis.shape[0]
    assert not (born & ~vis).any(), "born implies visible"
    before = np.vstack([np.zeros((1, vis.shape[1]), bool), vis[:-1]])
    assert not (vis & ~before & ~born).any(), "visible rises only where born is set"
    assert np.array_equal(np.isnan(tracks).any(2), ~vis) and np.array_equal(np.isnan(tracks).all(2), ~vis)
    md32 = float(np.float32(md))
    for t in range(T):
        assert int(detected[t]) == int(born[t].sum())
        if t % D != 0 or t == T - 1:
            assert detected[t] == 0
            continue
        new = tracks[t][born[t]].astype(np.int64)   # born points are integers
        assert np.array_equal(new.astype(np.float32), tracks[t][born[t]])
        old = np.rint(tracks[t][vis[t] & ~born[t]]).astype(np.int64)
        if len(new) and len(old):
            d2 = ((new[:, None] - old[None]) ** 2).sum(2)
            assert (d2.astype(np.float64) >= md32 * md32).all(), ("born point within md of a live track", t)
        if len(new) > 1:
            d2 = ((new[:, None] - new[None]) ** 2).sum(2)
            d2[np.arange(len(new)), np.arange(len(new))] = np.iinfo(np.int64).max
            assert (d2.astype(np.float64) >= md32 * md32).all(), ("two born points within md", t)


def test_split_tracks_on_hand_made_masks():
    import lucas_kanade_core as LK

    V = np.array([[1, 0, 0, 1],
                  [1, 0, 1, 1],
                  [0, 0, 1, 1],
                  [1, 0, 0, 1],
                  [1, 0, 0, 0]], bool)
    B = np.array([[1, 0, 0, 1],
                  [0, 0, 1, 0],
                  [0, 0, 0, 1],    # slot 3: a new track born while the old one was still visible is not possible in the
                  [1, 0, 0, 0],    # call, but the masks allow it and the cut is at the born mark
                  [0, 0, 0, 0]], bool)
    assert LK.split_tracks(V, B) == [(0, 0, 1), (0, 3, 4), (2, 1, 2), (3, 0, 1), (3, 2, 3)]
    assert LK.split_tracks(np.zeros((3, 2), bool), np.zeros((3, 2), bool)) == []
    assert LK.split_tracks(V.astype(np.uint8), B.astype(np.uint8)) == LK.split_tracks(V, B)
    bad = B.copy()
    bad[3, 0] = False   # visible rises without born
    with pytest.raises(ValueError):
        LK.split_tracks(V, bad)
    bad = B.copy()
    bad[2, 0] = True    # born without visible
    with pytest.raises(ValueError):
        LK.split_tracks(V, bad)
    with pytest.raises(ValueError):
        LK.split_tracks(V, B[:3])
    tr, vis, born, det = M.sequence(_scores_from([score_map(30, 30, t, 100) for t in range(6)]),
                                    TM.smooth_flows(5, 30, 30, seed=2, scale=5.0), 25, 2, 0.05, 4.0)
    parts = LK.split_tracks(vis, born)
    assert len(parts) == int(det.sum())
    cover = np.zeros_like(vis, dtype=np.int64)
    for n, a, b in parts:
        assert born[a, n] and vis[a:b + 1, n].all() and not born[a + 1:b + 1, n].any()
        cover[a:b + 1, n] += 1
    assert np.array_equal(cover, vis.astype(np.int64)), "every visible row belongs to exactly one track"


def test_python_arguments_are_checked_before_any_device_call():
    import lucas_kanade_core as LK
    import lucas_kanade_pyramidal as P

    frames = np.zeros((4, 16, 16), np.float32)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_replenish(frames, 10, bad)
    for win in (4, 13):
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt_replenish(frames, 10, 2, window_size=win)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_klt_replenish(frames, 0, 2)
    xy, vis = np.zeros((5, 2), np.float32), np.zeros(5, bool)
    with pytest.raises(ValueError):
        LK.replenish_features(frames, xy, vis)              # not one frame
    with pytest.raises(ValueError):
        LK.replenish_features(frames[0], xy, vis[:4])       # masks of different lengths
    with pytest.raises(ValueError):
        LK.replenish_features(frames[0], xy, vis, t=-1)
    with pytest.raises(ValueError):
        LK.replenish_features(frames[0], xy, vis, max_corners=6)
    with pytest.raises(ValueError):
        LK.replenish_features(frames[0], xy, vis, min_distance=-1.0)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """the C checks run before any device call, so they answer on a machine without a GPU"""
    import _oflk

    L = _oflk.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _oflk.SIGNATURES
    T, H, W, K = 4, 16, 16, 8
    frames = np.zeros((T, H, W), np.float32)
    tr, vis, born = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8), np.empty((T, K), np.uint8)
    det = np.empty(T, np.int32)

    def call(T_=T, win=5, D=2, K_=K, md=3.0, outs=None, u8=False):
        o = outs or (_oflk.ptr(tr), vis.ctypes.data, born.ctypes.data, det.ctypes.data_as(_oflk._i32p))
        fn = L.oflk_pyramidal_sequence_klt_replenish_u8 if u8 else L.oflk_pyramidal_sequence_klt_replenish
        src = frames.astype(np.uint8).ctypes.data if u8 else _oflk.ptr(frames)
        return fn(src, T_, H, W, 3, win, 3, 0.01, 0.5, 0.01, md, K_, D, *o)

    for u8 in (False, True):
        assert call(D=0, u8=u8) == _oflk.OFLK_ERR_INVALID and b"detect_every" in L.oflk_last_error()
        assert call(D=-1, u8=u8) == _oflk.OFLK_ERR_INVALID
        assert call(win=4, u8=u8) == _oflk.OFLK_ERR_UNSUPPORTED
        assert call(win=13, u8=u8) == _oflk.OFLK_ERR_UNSUPPORTED
        assert call(T_=1, u8=u8) == _oflk.OFLK_ERR_INVALID
        assert call(K_=0, u8=u8) == _oflk.OFLK_ERR_INVALID
        assert call(md=-1.0, u8=u8) == _oflk.OFLK_ERR_INVALID
        full = (_oflk.ptr(tr), vis.ctypes.data, born.ctypes.data, det.ctypes.data_as(_oflk._i32p))
        for i in range(4):
            assert call(outs=tuple(None if j == i else p for j, p in enumerate(full)), u8=u8) == _oflk.OFLK_ERR_INVALID, i
    import ctypes

    n = ctypes.c_size_t(0)
    assert L.oflk_replenish_features_workspace(H, W, 5, 3.0, K, None) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_replenish_features_workspace(H, W, 6, 3.0, K, ctypes.byref(n)) == _oflk.OFLK_ERR_UNSUPPORTED
    assert L.oflk_replenish_features_workspace(H, W, 5, 3.0, 0, ctypes.byref(n)) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_replenish_features_workspace(H, W, 5, 3.0, K, ctypes.byref(n)) == 0
    small, big = n.value, ctypes.c_size_t(0)
    assert L.oflk_replenish_features_workspace(H, W, 5, 0.0, K, ctypes.byref(big)) == 0 and big.value < small   # no seed grid
    assert L.oflk_replenish_features_workspace(H, W, 5, 1e9, 10 ** 5, ctypes.byref(big)) == 0 and big.value > small
    xy, v1, qt = np.zeros((K, 2), np.float32), np.zeros(K, np.uint8), np.zeros(K, np.int32)
    qxy, b1, d1 = np.zeros((K, 2), np.float32), np.zeros(K, np.uint8), np.zeros(1, np.int32)
    args = [_oflk.ptr(xy), v1.ctypes.data, qt.ctypes.data_as(_oflk._i32p), _oflk.ptr(qxy), b1.ctypes.data,
            d1.ctypes.data_as(_oflk._i32p)]
    host = L.oflk_replenish_features_host
    assert host(None, H, W, 5, 0.01, 3.0, K, 0, *args) == _oflk.OFLK_ERR_INVALID
    assert host(_oflk.ptr(frames[0]), H, W, 5, 0.01, 3.0, K, -1, *args) == _oflk.OFLK_ERR_INVALID
    assert host(_oflk.ptr(frames[0]), H, W, 4, 0.01, 3.0, K, 0, *args) == _oflk.OFLK_ERR_UNSUPPORTED
    assert host(_oflk.ptr(frames[0]), H, W, 5, 2.0, 3.0, K, 0, *args) == _oflk.OFLK_ERR_INVALID
    for i in range(6):
        a = [None if j == i else p for j, p in enumerate(args)]
        assert host(_oflk.ptr(frames[0]), H, W, 5, 0.01, 3.0, K, 0, *a) == _oflk.OFLK_ERR_INVALID, i
