"""GPU tests of the corner entry points on the scenes where the select kernel's rarer paths run (run on an MI355X: python -m
pytest tests/test_gpu_feature_edges.py -m gpu -q).

Every case holds the HIP output to tests/feature_model.py byte for byte.  The scenes (tests/feature_scenes.py) tie
~1.7e5 candidates at 1080p, chain conflicts across 256-key batches and 4 096-key slabs, put candidates at exact distances,
clamp the occupancy grid to one cell, and push the score, candidate and select launches past their 65 535-block grid
caps; tests/test_features_cpu.py checks on the CPU that each scene reaches its path.
"""
import numpy as np
import pytest

import feature_model as M
import feature_scenes as FS
from test_gpu_fb import _same
from test_gpu_features import _frame, _klt_vs_pieces, _norm, _same_features
from test_gpu_sequence import _dev

pytestmark = pytest.mark.gpu

NX = FS.f32_next


def _host(frames, K, q, md, win=5):
    import lucas_kanade_core as LK

    return LK.good_features_to_track_batch(frames, K, q, md, win)


# ---------------------------------------------------------------------------------------------------------------
# 1. the score map on partial tiles and on wide-range, tiny, huge and non-finite pixels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [17, 33, 47])
@pytest.mark.parametrize("W", [65, 100, 127, 129, 191, 1000])
def test_score_on_partial_tiles_and_extreme_values(H, W):
    import lucas_kanade_core as LK

    names, frames = zip(*FS.value_frames(H, W, seed=H * 1000 + W).items())
    frames = np.stack(frames)
    u8 = _frame(H, W, seed=H + W, u8=True)
    for win in M.WINDOWS:
        got = LK.corner_min_eigenvalue(frames, win)
        for i, name in enumerate(names):
            _same(got[i], M.score(frames[i], win), f"{H}x{W} window {win} {name}")
        _same(LK.corner_min_eigenvalue(u8, win), M.score(u8, win), f"{H}x{W} window {win} u8")


@pytest.mark.parametrize("H,W", [(33, 129), (47, 191), (17, 1000)], ids=lambda s: str(s))
def test_features_on_extreme_values(H, W):
    """a pixel whose S is 0 (non-finite pixels in its window, overflowing or underflowing products) is never a candidate,
    and the frame's max is taken over the finite scores only"""
    names, frames = zip(*FS.value_frames(H, W, seed=7 * H + W).items())
    frames = np.stack(frames)
    for q, md, K in ((0.01, 2.5, 200), (0.0, 0.0, H * W), (0.2, NX(1.0, np.inf), 50)):
        got = _host(frames, K, q, md)
        want = [M.good_features(f, 5, q, md, K) for f in frames]
        _same_features(got, want, f"{H}x{W} q={q} md={md} K={K}")
        for i, f in enumerate(frames):
            S, n = M.score(f, 5), int(got[2][i])
            p = got[0][i, :n].astype(np.int64)
            assert (S[p[:, 1], p[:, 0]] > 0).all(), names[i]
            if n:
                assert got[1][i, 0] == S.max(), names[i]
    assert int(got[2][names.index("nonfinite")]) > 0, "the frame with NaN and Inf pixels keeps features elsewhere"
    assert int(got[2][names.index("tiny")]) > 0, "subnormal scores are positive"


# ---------------------------------------------------------------------------------------------------------------
# 2. the tie lattice at 1080p: max_corners on batch and slab boundaries, min_distance on exact lattice distances
# ---------------------------------------------------------------------------------------------------------------
LATTICE_MD = [0.0, 1.0, NX(1.0, np.inf), 2.5, 7.0, NX(7.0, -np.inf), NX(7.0, np.inf), 10.0]
LATTICE_K = [1, 255, 256, 257, 2047, 2048, 2049, 4096, 4097]


@pytest.fixture(scope="module")
def lattices():
    return {c: (f, M.score(f, 5)) for c, f in ((1, FS.lattice()), (2, FS.lattice(contrasts=(190.0, 150.0))))}


@pytest.mark.parametrize("md", LATTICE_MD, ids=lambda v: repr(v))
@pytest.mark.parametrize("contrasts", [1, 2])
def test_tie_lattice(lattices, contrasts, md):
    f, S = lattices[contrasts]
    full = M.select(S, 0.0, md, len(M.candidates(S, 0.0)[0]) + 1)
    n = full[0]
    for K in LATTICE_K + [n - 1, n, n + 1]:
        if K < 1:
            continue
        got = _host(f, K, 0.0, md)
        _same_features(got, [FS.truncate(full, K)], f"lattice {contrasts} md={md!r} K={K}")
    if md in (1.0, NX(1.0, np.inf)):   # the first blob's plateau starts (3, 3), (4, 3): 1 apart
        got = _host(f, 8, 0.0, md)
        pts = {tuple(p) for p in got[0][0, :int(got[2][0])].astype(np.int64).tolist()}
        assert (3, 3) in pts and ((4, 3) in pts) == (md == 1.0), pts


# ---------------------------------------------------------------------------------------------------------------
# 3. chains of conflicts inside 256-key batches, across batches and across slabs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", FS.CHAIN_ORDERS)
def test_conflict_chains(order):
    f = FS.chain_rows(order)
    S = M.score(f, 5)
    for md in (FS.CHAIN_MD, NX(FS.CHAIN_STEP + 1, np.inf)):
        full = M.select(S, 0.0, md, len(M.candidates(S, 0.0)[0]) + 1)
        n = full[0]
        for K in (257, 4097, n - 1, n + 1):
            _same_features(_host(f, K, 0.0, md), [FS.truncate(full, K)], f"chains {order} md={md!r} K={K}")


# ---------------------------------------------------------------------------------------------------------------
# 4. min_distance exactly on a distance between candidates, and one float32 step either side
# ---------------------------------------------------------------------------------------------------------------
def test_exact_distances():
    f, pairs = FS.exact_pairs()
    for md in (5.0, NX(5.0, np.inf), NX(5.0, -np.inf), 2.5):
        K = 4 * len(pairs)
        got = _host(f, K, 0.0, md, win=3)
        _same_features(got, [M.good_features(f, 3, 0.0, md, K)], f"pairs md={md!r}")
        pts = {tuple(p) for p in got[0][0, :int(got[2][0])].astype(np.int64).tolist()}
        for dx, dy, a, b in pairs:
            d2 = dx * dx + dy * dy
            if md != 2.5 and d2 != 25:
                continue
            both = d2 >= np.float64(np.float32(md)) ** 2
            assert a in pts and (b in pts) == both, (md, dx, dy, a, b)


# ---------------------------------------------------------------------------------------------------------------
# 5. the occupancy grid clamped to max(H, W), and one cell
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FS.GRID_SHAPES, ids=lambda s: str(s))
def test_grid_limits(H, W):
    f = FS.grid_frame(H, W)
    for md in FS.grid_mds(H, W):
        for K in (1, 5, 64):
            _same_features(_host(f, K, 0.0, md), [M.good_features(f, 5, 0.0, md, K)], f"{H}x{W} md={md!r} K={K}")


# ---------------------------------------------------------------------------------------------------------------
# 6. quality level at its ends
# ---------------------------------------------------------------------------------------------------------------
def test_quality_level_ends():
    frames = np.stack([_frame(120, 160, seed=61, u8=False), FS.lattice(120, 160)])
    got = _host(frames, 50, 1.0, 0.0)
    assert (got[2] == 0).all() and np.isnan(got[0]).all() and (got[1] == 0).all()
    for f in range(len(frames)):
        S = M.score(frames[f], 5)
        assert S.max() > 0
        K = frames[f].size
        got = _host(frames[f], K, 0.0, 0.0)
        pad = np.pad(S, 1, constant_values=-np.inf)
        peak = S > 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                peak &= S >= pad[1 + dy:1 + dy + S.shape[0], 1 + dx:1 + dx + S.shape[1]]
        assert int(got[2][0]) == int(peak.sum())
        _same_features(got, [M.good_features(frames[f], 5, 0.0, 0.0, K)], f"q=0 frame {f}")


# ---------------------------------------------------------------------------------------------------------------
# 7. batches of unlike frames, and launches past the 65 535-block grid caps
# ---------------------------------------------------------------------------------------------------------------
def _unlike_frames(H=1080, W=1920):
    blob = np.full((H, W), 60.0, np.float32)
    blob[500:502, 900:902] = 190.0
    return np.stack([FS.lattice(H, W), np.zeros((H, W), np.float32), blob, _frame(H, W, seed=71, u8=False)])


def test_unlike_frames_in_one_call_host_and_device_form():
    import torch

    import _oflk

    frames = _unlike_frames()
    F, H, W = frames.shape
    K, q, md = 5000, 0.001, NX(7.0, np.inf)
    want = [M.good_features(f, 5, q, md, K) for f in frames]
    assert want[1][0] == 0 and want[2][0] >= 1 and want[0][0] > 4096
    _same_features(_host(frames, K, q, md), want, "host form")
    dev = torch.device("cuda", 0)
    nbytes = _oflk.good_features_workspace(F, H, W, 5, md, K)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    d_f = _dev(frames)
    d_cnt = torch.full((F,), -1, dtype=torch.int32, device=dev)
    d_xy = torch.full((F, K, 2), 3.0, dtype=torch.float32, device=dev)
    d_sc = torch.full((F, K), 3.0, dtype=torch.float32, device=dev)
    _oflk.good_features(d_f.data_ptr(), F, H, W, ws.data_ptr(), nbytes, d_cnt.data_ptr(), d_xy.data_ptr(), d_sc.data_ptr(),
                        K, q, md, 5, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same_features((d_xy.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy()), want, "device form")


def test_many_small_frames_past_the_grid_caps():
    """F = 65 600 > 65 535: the score, candidate and select launches loop over frames a second time"""
    import lucas_kanade_core as LK

    distinct = FS.small_frames(12, 12)
    F = 65600
    frames = np.stack([distinct[i % len(distinct)] for i in range(F)])
    K, q, md = 12, 0.01, 2.5
    want = [M.good_features(f, 5, q, md, K) for f in distinct]
    xy, sc, cnt = _host(frames, K, q, md)
    for i in range(len(distinct)):
        idx = np.arange(i, F, len(distinct))
        n, wxy, wsc = want[i]
        assert (cnt[idx] == n).all(), (i, np.flatnonzero(cnt[idx] != n)[:5])
        _same(_norm(xy[idx]), np.broadcast_to(_norm(wxy), (len(idx),) + wxy.shape).copy(), f"frame class {i}: xy")
        _same(sc[idx], np.broadcast_to(wsc, (len(idx),) + wsc.shape).copy(), f"frame class {i}: score")
    S = LK.corner_min_eigenvalue(frames, 5)
    for i, f in enumerate(distinct):
        _same(S[i::len(distinct)], np.broadcast_to(M.score(f, 5), S[i::len(distinct)].shape).copy(), f"score class {i}")


def test_tall_frame_past_the_grid_caps():
    """1 048 600 x 24: 65 538 tile rows in the score launch, 262 150 row blocks in the candidate launch; the brightest
    blobs sit in the rows only the second turn of each loop reaches"""
    import lucas_kanade_core as LK

    f = FS.tall_frame()
    H, W = f.shape
    S = M.score(f, 5)
    _same(LK.corner_min_eigenvalue(f, 5), S, "tall frame score")
    K, q, md = 3000, 0.01, 5.0
    want = M.select(S, q, md, K)
    got = _host(f, K, q, md)
    _same_features(got, [want], "tall frame")
    ys = got[0][0, :int(got[2][0]), 1]
    assert (ys >= 16 * 65535).any() and ((ys >= 4 * 65535) & (ys < H - 64)).any(), "the second turns select points"


# ---------------------------------------------------------------------------------------------------------------
# 8. detect then track on the lattice
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_klt_on_the_tie_lattice(u8):
    frames = np.stack([FS.lattice(shift=(t, 2 * t)) for t in range(4)])
    if u8:
        frames = frames.astype(np.uint8)
    n, vis = _klt_vs_pieces(frames, 5000, 0.01, NX(7.0, np.inf))
    assert n == 5000
