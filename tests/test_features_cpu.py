"""CPU tests of the Shi-Tomasi statement (tests/feature_model.py), of the corner entry points' argument checks and of the
new C ABI surface.  Nothing here touches a device."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import feature_model as M
import feature_scenes as FS

ROOT = Path(__file__).resolve().parents[1]
FEATURE_SYMBOLS = ["oflk_corner_score", "oflk_corner_score_host", "oflk_corner_score_host_u8", "oflk_good_features_workspace",
                   "oflk_good_features", "oflk_good_features_host", "oflk_good_features_host_u8", "oflk_pyramidal_sequence_klt",
                   "oflk_pyramidal_sequence_klt_u8"]


def _frame(H, W, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (H, W)).astype(np.uint8)


def test_score_is_the_smaller_eigenvalue():
    """the cancellation-free form agrees with eigvalsh of [[a, b], [b, c]] to ~1e-12 relative, in float64"""
    f = _frame(40, 50, 1).astype(np.float32)
    a, b, c = M.tensor(f, 5)
    s = M.min_eig64(a, b, c)
    mats = np.stack([np.stack([a, b], -1), np.stack([b, c], -1)], -2).astype(np.float64)
    ev = np.linalg.eigvalsh(mats)[..., 0]
    det = a.astype(np.float64) * c - b.astype(np.float64) * b
    pos = det > 0
    assert pos.mean() > 0.9
    scale = np.maximum(np.abs(ev), 1e-300)
    assert np.max(np.abs(s[pos] - ev[pos]) / scale[pos]) < 1e-12
    assert (s[~pos] == 0).all()


@pytest.mark.parametrize("win", [3, 5, 7])
def test_tensor_equals_window_sums_of_the_reference_gradients(win):
    """values below 64: every product and partial sum is exact in float32, so the window sums equal np.sum of the
    reference's own window slices of compute_gradients(f, f) whatever the order"""
    f = _frame(23, 31, win, hi=64)
    Ix, Iy = M.gradients(f)
    a, b, c = M.tensor(f, win)
    h = win // 2
    H, W = f.shape
    for y in range(h, H - h):
        for x in range(h, W - h):
            wx, wy = Ix[y - h:y + h + 1, x - h:x + h + 1], Iy[y - h:y + h + 1, x - h:x + h + 1]
            assert a[y - h, x - h] == np.sum(wx * wx)
            assert b[y - h, x - h] == np.sum(wx * wy)
            assert c[y - h, x - h] == np.sum(wy * wy)


def test_score_border_and_small_frames():
    f = _frame(30, 40, 3)
    for win in M.WINDOWS:
        S = M.score(f, win)
        h = win // 2
        assert S.dtype == np.float32 and S.shape == f.shape
        inner = np.zeros_like(S, bool)
        inner[h:30 - h, h:40 - h] = True
        assert (S[~inner] == 0).all() and (S[inner] > 0).mean() > 0.9
    for H, W in ((1, 1), (4, 4), (2, 30)):
        assert (M.score(_frame(H, W, 0), 5) == 0).all()
        assert M.good_features(_frame(H, W, 0), 5)[0] == 0


def _plateau_map():
    """a score map with plateaus (equal neighbours) and ties across the map"""
    rng = np.random.default_rng(7)
    S = np.round(rng.random((40, 60)) * 8).astype(np.float32)
    S[10:14, 20:26] = 9.0
    S[30:32, 5:7] = 9.0
    return S


MAPS = [np.random.default_rng(s).random((50, 70)).astype(np.float32) ** 3 for s in range(3)] + [_plateau_map()]


@pytest.mark.parametrize("q,md,K", [(0.01, 5.0, 40), (0.2, 2.5, 500), (0.0, 10.0, 7), (0.05, 1.5, 1000)])
@pytest.mark.parametrize("m", range(len(MAPS)))
def test_selection_properties(m, q, md, K):
    S = MAPS[m]
    n, xy, sc = M.select(S, q, md, K)
    ys, xs, Mx = M.candidates(S, q)
    acc = xy[:n].astype(np.int64)
    # pairwise at least md apart
    d2 = ((acc[:, None, :] - acc[None]) ** 2).sum(-1).astype(np.float64)
    np.fill_diagonal(d2, np.inf)
    assert (d2 >= np.float64(np.float32(md)) ** 2).all()
    # in priority order: score descending, then raster index
    keys = [(-float(S[y, x]), y * S.shape[1] + x) for x, y in acc]
    assert keys == sorted(keys)
    assert np.array_equal(sc[:n], S[acc[:, 1], acc[:, 0]])
    assert np.isnan(xy[n:]).all() and (sc[n:] == 0).all()
    # every candidate ranked before the K-th acceptance and not accepted has an earlier accepted point within md
    accepted = {(int(x), int(y)) for x, y in acc}
    last = keys[-1] if n else None
    for y, x in zip(ys, xs):
        key = (-float(S[y, x]), y * S.shape[1] + x)
        if n == K and key > last:
            break
        if (x, y) in accepted:
            continue
        near = [(ax, ay) for ax, ay in accepted if (-float(S[ay, ax]), ay * S.shape[1] + ax) < key
                and float((ax - x) ** 2 + (ay - y) ** 2) < np.float64(np.float32(md)) ** 2]
        assert near, (x, y)
    if n < K:
        assert n <= len(ys)


def test_selection_edge_cases():
    S = _plateau_map()
    n, xy, sc = M.select(S, 0.01, 5.0, 1)
    ys, xs, _ = M.candidates(S, 0.01)
    assert n == 1 and tuple(xy[0]) == (xs[0], ys[0]) and sc[0] == S.max()
    assert (ys[0], xs[0]) == (10, 20)   # the plateau's first pixel in raster order
    # md = 0: every candidate, in priority order
    n, xy, _ = M.select(S, 0.0, 0.0, 100000)
    assert n == len(ys) and np.array_equal(xy[:n], np.stack([xs, ys], 1).astype(np.float32))
    # q = 0: every positive local maximum is a candidate; q = 1: none
    pos = (S > 0).sum()
    assert len(M.candidates(S, 0.0)[0]) <= pos and M.select(S, 1.0, 0.0, 10)[0] == 0
    assert M.select(np.zeros((9, 9), np.float32), 0.0, 0.0, 10)[0] == 0
    # md <= 1 does not thin: distinct pixels are >= 1 apart
    assert M.select(S, 0.0, 1.0, 100000)[0] == len(ys)


# ---------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------
INV, UNS = -1, -4


def test_c_layer_rejects_bad_arguments_before_any_device_call():
    """every check runs before the device is touched, so these return on a machine without a GPU too"""
    import _oflk

    L = _oflk.lib()
    F, H, W, K = 2, 16, 20, 8
    fr = np.zeros((F, H, W), np.float32)
    u8 = np.zeros((F, H, W), np.uint8)
    cnt = np.zeros(F, np.int32)
    xy, sc = np.zeros((F, K, 2), np.float32), np.zeros((F, K), np.float32)
    S = np.zeros((F, H, W), np.float32)
    P = _oflk.ptr
    i32 = cnt.ctypes.data_as(_oflk._i32p)

    def gf(u=False, **kw):
        a = dict(f=P(fr) if not u else u8.ctypes.data, F=F, win=5, q=0.01, md=10.0, K=K, cnt=i32, xy=P(xy), sc=P(sc))
        a.update(kw)
        fn = L.oflk_good_features_host_u8 if u else L.oflk_good_features_host
        return fn(a["f"], a["F"], H, W, a["win"], a["q"], a["md"], a["K"], a["cnt"], a["xy"], a["sc"])

    bad = [dict(F=0), dict(F=-1), dict(f=None), dict(cnt=None), dict(xy=None), dict(sc=None), dict(q=-0.01), dict(q=1.5),
           dict(q=float("nan")), dict(q=float("inf")), dict(md=-1.0), dict(md=float("nan")), dict(md=float("inf")), dict(K=0),
           dict(K=-5)]
    for kw in bad:
        assert gf(**kw) == INV, kw
        assert gf(True, **kw) == INV, kw
    for win in (1, 2, 4, 13, 0, -3):
        assert gf(win=win) == UNS and gf(True, win=win) == UNS, win
    for fn, src in ((L.oflk_corner_score_host, P(fr)), (L.oflk_corner_score_host_u8, u8.ctypes.data)):
        assert fn(src, 0, H, W, 5, P(S)) == INV and fn(None, F, H, W, 5, P(S)) == INV and fn(src, F, H, W, 5, None) == INV
        assert fn(src, F, H, W, 6, P(S)) == UNS and fn(src, F, H, W, 13, P(S)) == UNS
    n = ctypes.c_size_t(0)
    ws = L.oflk_good_features_workspace
    assert ws(F, H, W, 5, 10.0, K, None) == INV and ws(0, H, W, 5, 10.0, K, ctypes.byref(n)) == INV
    assert ws(F, H, W, 5, -1.0, K, ctypes.byref(n)) == INV and ws(F, H, W, 5, 10.0, 0, ctypes.byref(n)) == INV
    assert ws(F, H, W, 4, 10.0, K, ctypes.byref(n)) == UNS
    assert ws(F, H, W, 5, 10.0, K, ctypes.byref(n)) == 0 and n.value >= F * H * W * 12
    need = n.value
    buf = ctypes.c_void_p(1 << 20)   # never dereferenced: each call below fails its checks first

    def dgf(**kw):
        a = dict(f=buf, F=F, win=5, q=0.01, md=10.0, K=K, ws=ctypes.c_void_p(1 << 20), nb=need, cnt=buf, xy=buf, sc=buf)
        a.update(kw)
        return L.oflk_good_features(a["f"], 0, a["F"], H, W, a["win"], a["q"], a["md"], a["K"], a["ws"], a["nb"], a["cnt"],
                                    a["xy"], a["sc"], None)

    for kw in bad[:2] + [dict(f=None), dict(ws=None), dict(cnt=None), dict(xy=None), dict(sc=None), dict(q=2.0),
                         dict(md=float("-inf")), dict(K=0), dict(nb=need - 1), dict(ws=ctypes.c_void_p((1 << 20) + 8)),
                         dict(xy=ctypes.c_void_p((1 << 20) + 4))]:
        assert dgf(**kw) == INV, kw
    assert dgf(win=8) == UNS
    assert L.oflk_corner_score(None, 0, F, H, W, 5, buf, None) == INV
    assert L.oflk_corner_score(buf, 0, 0, H, W, 5, buf, None) == INV
    assert L.oflk_corner_score(buf, 0, F, H, W, 5, None, None) == INV
    assert L.oflk_corner_score(buf, 0, F, H, W, 12, buf, None) == UNS

    T = 3
    seq = np.zeros((T, H, W), np.float32)
    tr, vis = np.zeros((T, K, 2), np.float32), np.zeros((T, K), np.uint8)

    def klt(u=False, **kw):
        a = dict(f=P(seq) if not u else u8.ctypes.data, T=T, win=5, q=0.01, md=10.0, K=K, alpha=0.01, beta=0.5, cnt=i32,
                 xy=P(xy), sc=P(sc), tr=P(tr), vis=vis.ctypes.data)
        a.update(kw)
        fn = L.oflk_pyramidal_sequence_klt_u8 if u else L.oflk_pyramidal_sequence_klt
        return fn(a["f"], a["T"], H, W, 3, a["win"], 3, a["alpha"], a["beta"], a["q"], a["md"], a["K"], a["cnt"], a["xy"],
                  a["sc"], a["tr"], a["vis"])

    for kw in [dict(T=1), dict(f=None), dict(cnt=None), dict(xy=None), dict(sc=None), dict(tr=None), dict(vis=None),
               dict(q=-1.0), dict(md=float("nan")), dict(K=0), dict(alpha=-1.0), dict(beta=float("inf"))]:
        assert klt(**kw) == INV, kw
        assert klt(True, **kw) == INV, kw
    for win in (4, 13, 15):   # LK windows the corner kernels do not cover
        assert klt(win=win) == UNS and klt(True, win=win) == UNS, win


def test_python_layer_rejects_bad_input_before_any_device_call(monkeypatch):
    import _oflk
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_oflk, "lib", no_device)
    f = np.zeros((16, 16), np.float32)
    seq = np.zeros((3, 16, 16), np.float32)
    for kw in (dict(max_corners=0), dict(max_corners=2.5), dict(max_corners=True), dict(max_corners=10, quality_level=-0.1),
               dict(max_corners=10, quality_level=1.1), dict(max_corners=10, quality_level=float("nan")),
               dict(max_corners=10, min_distance=-1.0), dict(max_corners=10, min_distance=float("inf")),
               dict(max_corners=10, window_size=4), dict(max_corners=10, window_size=13)):
        with pytest.raises(ValueError):
            K.good_features_to_track(f, **kw)
        with pytest.raises(ValueError):
            K.good_features_to_track_batch(seq, **kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_klt(seq, **kw)
    for w in (2, 4, 13, 1):
        with pytest.raises(ValueError):
            K.corner_min_eigenvalue(f, w)
    for bad in (np.zeros((4,)), np.zeros((2, 3, 4, 5)), np.zeros((0, 4))):
        with pytest.raises(ValueError):
            K.corner_min_eigenvalue(bad)
        with pytest.raises(ValueError):
            K.good_features_to_track_batch(bad, 10)
    with pytest.raises(ValueError):
        K.good_features_to_track(seq, 10)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_klt(seq[:1], 10)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_klt(seq, 10, alpha=-1.0)


def test_features_to_queries():
    import lucas_kanade_core as K

    q = K.features_to_queries(np.array([[1.5, 2.0], [3.0, 4.0]], np.float32))
    assert q.dtype == np.float32 and q.tolist() == [[0, 1.5, 2.0], [0, 3.0, 4.0]]
    xy = np.full((2, 3, 2), np.nan, np.float32)
    xy[0, :2] = [[1, 2], [3, 4]]
    xy[1, :1] = [[5, 6]]
    q = K.features_to_queries(xy, np.array([2, 1]), t=4)
    assert q.tolist() == [[4, 1, 2], [4, 3, 4], [5, 5, 6]]
    assert K.features_to_queries(xy, [0, 0]).shape == (0, 3)
    with pytest.raises(ValueError):
        K.features_to_queries(xy)


def test_new_symbols_are_declared_and_exported():
    import _oflk

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oflk.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oflk_[a-z0-9_]+)\s*\(", text))
    L = _oflk.lib()
    for name in FEATURE_SYMBOLS:
        assert name in declared, f"{name} not declared in include/oflk.h"
        assert hasattr(L, name), f"{name} not exported by liboflk.so"
        assert name in _oflk.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------
# the scenes of tests/test_gpu_feature_edges.py (tests/feature_scenes.py): each reaches its path, and the statement's
# greedy equals a brute force without the grid on it
# ---------------------------------------------------------------------------------------------------------------
NX = FS.f32_next
EDGE_MDS = [0.0, 1.0, NX(1.0, np.inf), 2.5, 7.0, NX(7.0, -np.inf), NX(7.0, np.inf), 10.0, FS.CHAIN_MD, NX(8.0, np.inf)]


def _same_selection(a, b, what):
    n, xy, sc = a
    m, wxy, wsc = b
    assert n == m, (what, n, m)
    assert np.array_equal(xy, wxy, equal_nan=True), what
    assert np.array_equal(sc.view(np.int32), wsc.view(np.int32)), what


@pytest.fixture(scope="module")
def full_size_scenes():
    return {"lattice": M.score(FS.lattice(), 5), "lattice2": M.score(FS.lattice(contrasts=(190.0, 150.0)), 5),
            "klt": M.score(FS.lattice(shift=(0, 0)), 5),
            **{o: M.score(FS.chain_rows(o), 5) for o in FS.CHAIN_ORDERS}}


def test_lattice_scenes_tie_more_than_three_slabs(full_size_scenes):
    """the descent must cut slabs inside the raster-index digits: more than 3 x 4 096 candidates share the top score"""
    for name in ("lattice", "lattice2", "klt"):
        assert FS.top_ties(full_size_scenes[name]) > 3 * 4096, name


def test_chain_scenes_chain_across_batches(full_size_scenes):
    """a run of at least 300 consecutive candidates in priority order, each conflicting with the one before it; in the
    alternating scene each blob has its own score, high and low in turn"""
    for order in ("increasing", "decreasing"):
        assert FS.conflict_runs(full_size_scenes[order], 0.0, FS.CHAIN_MD) >= 300, order
    S = full_size_scenes["alternating"]
    ys, xs, _ = M.candidates(S, 0.0)
    s = S[ys, xs]
    assert len(np.unique(s)) * 4 == len(s), "four tied plateau pixels per blob, every blob its own score"
    row = S[3, 3:3 + 7 * 8:7]
    assert (row[0::2, None] > row[None, 1::2]).all(), row


def test_chain_md_conflicts_with_neighbours_only():
    """in a chain row every pixel of a blob lies within CHAIN_MD of every pixel of its neighbours and not within it of
    any pixel of the blob after next, or of another row"""
    s, g, md2 = FS.CHAIN_STEP, FS.CHAIN_GAP, FS.CHAIN_MD ** 2
    px = [(dx, dy) for dx in (0, 1) for dy in (0, 1)]
    assert all((s + bx - ax) ** 2 + (by - ay) ** 2 < md2 for ax, ay in px for bx, by in px)
    assert all((2 * s + bx - ax) ** 2 + (by - ay) ** 2 >= md2 for ax, ay in px for bx, by in px)
    assert (g - 1) ** 2 >= md2


def test_exact_pair_scene():
    """every dot is one candidate, and candidates lie at each exact offset"""
    f, pairs = FS.exact_pairs()
    S = M.score(f, 3)
    assert len(M.candidates(S, 0.0)[0]) == 2 * len(pairs)
    assert set(FS.PAIR_OFFSETS) <= FS.candidate_offsets(S)
    ys, xs, _ = M.candidates(S, 0.0)
    rank = {(int(x), int(y)): i for i, (y, x) in enumerate(zip(ys, xs))}
    same = [rank[a] // 256 == rank[b] // 256 for _, _, a, b in pairs]
    assert any(same) and not all(same), "some pairs share a 256-key batch, some do not"


def test_value_scenes_reach_overflow_underflow_and_non_finite_pixels():
    for H, W in ((17, 65), (47, 1000)):
        v = FS.value_frames(H, W, seed=3)
        for win in M.WINDOWS:
            tiny = M.score(v["tiny"], win)
            assert (tiny > 0).any() and (tiny[tiny > 0] < np.finfo(np.float32).tiny).all(), "subnormal scores"
        with np.errstate(over="ignore", invalid="ignore"):
            a, b, c = M.tensor(v["huge"], 5)
        assert not np.isfinite(a).all() and (M.score(v["huge"], 3) > 0).any(), "overflowing sums next to finite scores"
        nf = v["nonfinite"]
        assert np.isnan(nf).any() and np.isposinf(nf).any() and np.isneginf(nf).any()
        assert (M.score(nf, 5) > 0).any()
        assert (v["negative"] < 0).all() and v["u16"].max() > 60000 and v["unit"].max() < 1.0


def test_tall_frame_has_its_best_blobs_past_the_grid_caps():
    f = FS.tall_frame()
    assert f.shape == (FS.TALL_H, FS.TALL_W) and (FS.TALL_H + 15) // 16 > 65535 and (FS.TALL_H + 3) // 4 > 65535
    hot = np.flatnonzero((f == 230.0).any(1))
    assert hot.min() >= FS.TALL_H - 64 and hot.max() >= 16 * 65535
    warm = np.flatnonzero((f == 210.0).any(1))
    assert warm.min() >= 262136 and warm.max() >= 4 * 65535


def test_truncation_is_the_smaller_max_corners():
    S = M.score(FS.lattice(240, 320), 5)
    for md in (0.0, NX(7.0, np.inf)):
        full = M.select(S, 0.0, md, 100000)
        for K in (1, 255, 256, 257, full[0] - 1, full[0], full[0] + 1):
            _same_selection(M.select(S, 0.0, md, K), FS.truncate(full, K), f"md={md} K={K}")


def _crop_scenes():
    """every new scene at 240 x 320 or smaller, keeping its spacing: (name, S, md values)"""
    out = [("lattice", M.score(FS.lattice(240, 320), 5), EDGE_MDS),
           ("lattice2", M.score(FS.lattice(240, 320, contrasts=(190.0, 150.0)), 5), EDGE_MDS),
           ("klt", M.score(FS.lattice(240, 320, shift=(3, 6)), 5), EDGE_MDS)]
    out += [(o, M.score(FS.chain_rows(o, 240, 320), 5), EDGE_MDS) for o in FS.CHAIN_ORDERS]
    f, _ = FS.exact_pairs(rows=4, cols=14)
    out.append(("pairs", M.score(f, 3), [5.0, NX(5.0, np.inf), NX(5.0, -np.inf), 2.5, np.sqrt(5.0), np.sqrt(8.0)]))
    out += [(f"grid {H}x{W}", M.score(FS.grid_frame(H, W), 5), FS.grid_mds(H, W)) for H, W in FS.GRID_SHAPES]
    with np.errstate(over="ignore", invalid="ignore"):
        out += [(f"values {k}", M.score(v, 5), [0.0, 2.5, 7.0]) for k, v in FS.value_frames(47, 191, seed=5).items()]
    out += [(f"small {i}", M.score(f, 5), [0.0, 2.5]) for i, f in enumerate(FS.small_frames())]
    out.append(("unlike blob", M.score(FS.small_frames(240, 320)[4], 5), [0.0, 2.5]))
    tall = FS.tall_frame()
    out.append(("tall bottom", M.score(tall[-240:], 5), [0.0, 5.0]))
    return out


@pytest.mark.parametrize("name,S,mds", _crop_scenes(), ids=lambda v: v if isinstance(v, str) else "")
def test_statement_greedy_equals_brute_force_on_scene_crops(name, S, mds):
    for md in mds:
        for q in (0.0, 0.01):
            full = FS.brute_select(S, q, md, S.size + 1)
            for K in sorted({1, 255, 256, 257, max(full[0] - 1, 1), full[0] + 1}):
                _same_selection(M.select(S, q, md, K), FS.truncate(full, K), f"{name} q={q} md={md!r} K={K}")


@pytest.mark.parametrize("name", ["lattice", "lattice2", "increasing", "decreasing", "alternating"])
def test_statement_greedy_at_full_size_is_ordered_and_spaced(full_size_scenes, name):
    """at 1080p the brute force is too slow: the accepted points are in priority order and no two lie closer than md"""
    S = full_size_scenes[name]
    for md in (NX(1.0, np.inf), 2.5, NX(7.0, np.inf), FS.CHAIN_MD):
        n, xy, sc = M.select(S, 0.0, md, 30000)
        assert n > 4096
        FS.check_greedy_output(S, md, n, xy, sc)
