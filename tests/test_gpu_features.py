"""GPU tests of the Shi-Tomasi corner entry points (run on an MI355X: python -m pytest tests/test_gpu_features.py -m gpu -q).

oflk_corner_score and oflk_good_features must equal the NumPy statement of tests/feature_model.py byte for byte, on every
shape form and window; oflk_pyramidal_sequence_klt must equal oflk_good_features_host on frame 0 followed by
oflk_pyramidal_sequence_tracks on those points.
"""
import numpy as np
import pytest

import feature_model as M
from test_gpu_fb import _same
from test_gpu_sequence import _dev, _video

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 5), (23, 21), (37, 53), (240, 320), (1080, 1920)]


def _frame(H, W, seed, u8):
    """a textured frame: the synthetic scene plus noise, float32 with fractional values in [0, 255] (uint8 when asked)"""
    from oflk_synth import synth_pair

    rng = np.random.default_rng(seed)
    f = synth_pair(max(H, 8), max(W, 8), pair_index=seed % 5)[0][:H, :W].astype(np.float64)
    f = np.clip(f + rng.normal(0.0, 6.0, (H, W)), 0, 255)
    return np.round(f).astype(np.uint8) if u8 else f.astype(np.float32)


def _norm(xy):
    t = np.array(xy, np.float32, copy=True)
    t[np.isnan(t)] = np.float32(np.nan)
    return t


def _same_features(got, want, what):
    """got = (xy (F, K, 2), score (F, K), count (F,)); want = [(count, xy, score)] per frame"""
    xy, sc, cnt = got
    for f, (n, wxy, wsc) in enumerate(want):
        assert int(cnt[f]) == n, f"{what}: frame {f}: count {int(cnt[f])} != {n}"
        _same(_norm(xy[f]), _norm(wxy), f"{what}: frame {f}: xy")
        _same(sc[f], wsc, f"{what}: frame {f}: score")


# ---------------------------------------------------------------------------------------------------------------
# the score map
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda s: str(s))
def test_score_equals_statement(H, W, u8):
    import lucas_kanade_core as K

    f = _frame(H, W, seed=H + 7 * W, u8=u8)
    for win in M.WINDOWS:
        got = K.corner_min_eigenvalue(f, win)
        want = M.score(f, win)
        _same(got, want, f"{H}x{W} window {win}")
        if H * W >= 1000:
            assert (want > 0).mean() > 0.5, "the frame should be textured"


def test_score_batch_and_device_form_equal_single_frames():
    import torch

    import _oflk
    import lucas_kanade_core as K

    F, H, W = 5, 37, 53
    for u8 in (False, True):
        frames = np.stack([_frame(H, W, seed=s, u8=u8) for s in range(F)])
        want = np.stack([M.score(f, 7) for f in frames])
        _same(K.corner_min_eigenvalue(frames, 7), want, f"batch u8={u8}")
        d_f = _dev(frames)
        d_s = torch.full((F, H, W), -1.0, dtype=torch.float32, device=d_f.device)
        _oflk.corner_score(d_f.data_ptr(), F, H, W, d_s.data_ptr(), 7, u8=u8, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _same(d_s.cpu().numpy(), want, f"device form u8={u8}")


# ---------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------
PARAMS = [(0.01, 10.0, 100), (0.05, 3.5, 50), (0.0, 0.0, 5000), (0.1, 1.0, 200), (0.01, 25.0, 30), (0.3, 1.5, 10000),
          (0.01, 10.0, 1), (1.0, 5.0, 10)]


def _checkerboard(H, W, s):
    y, x = np.mgrid[0:H, 0:W]
    return (((y // s) + (x // s)) % 2 * 200.0 + 20.0).astype(np.float32)


def _plateau(H, W):
    """identical 2x2 bright squares on a flat frame: each gives four adjacent pixels of one score (a plateau of candidates),
    and every square the same scores (ties across the frame, resolved by raster index)"""
    f = np.full((H, W), 50.0, np.float32)
    for y in range(6, H - 8, 13):
        for x in range(6, W - 8, 11):
            f[y:y + 2, x:x + 2] = 180.0
    return f


@pytest.mark.parametrize("q,md,K", PARAMS, ids=lambda v: str(v))
def test_selection_equals_statement(q, md, K):
    import lucas_kanade_core as LK

    frames = [_frame(240, 320, seed=3, u8=False), _frame(37, 53, seed=4, u8=False), _checkerboard(64, 80, 6), _plateau(60, 70),
              np.zeros((40, 50), np.float32)]
    for i, f in enumerate(frames):
        xy, sc, cnt = LK.good_features_to_track_batch(f[None], K, q, md, 5)
        want = M.good_features(f, 5, q, md, K)
        _same_features((xy, sc, cnt), [want], f"frame {i} {f.shape}")
        if i == 4:
            assert int(cnt[0]) == 0
    n, _, _ = M.good_features(frames[3], 5, 0.0, 0.0, 10000)
    assert n >= 4 * len(range(6, 60 - 8, 13)) * len(range(6, 70 - 8, 11)), "the plateau frame should give tied candidates"


def test_selection_on_uint8_and_every_window():
    import lucas_kanade_core as LK

    f = _frame(240, 320, seed=9, u8=True)
    for win in M.WINDOWS:
        got = LK.good_features_to_track_batch(f, 300, 0.02, 6.0, win)
        _same_features(got, [M.good_features(f, win, 0.02, 6.0, 300)], f"u8 window {win}")
    xy, sc = LK.good_features_to_track(f, 300, 0.02, 6.0, 5)
    n, wxy, wsc = M.good_features(f, 5, 0.02, 6.0, 300)
    _same(xy, wxy[:n], "trimmed xy")
    _same(sc, wsc[:n], "trimmed score")


def test_selection_at_1080p_with_many_corners():
    """K = 10 000 over several slabs of the select kernel's LDS"""
    import lucas_kanade_core as LK

    f = _frame(1080, 1920, seed=11, u8=False)
    for q, md, K in ((0.01, 10.0, 10000), (0.0, 1.0, 20000), (0.001, 2.5, 15000)):
        got = LK.good_features_to_track_batch(f, K, q, md, 5)
        want = M.good_features(f, 5, q, md, K)
        assert want[0] > 4096 or md > 5, want[0]
        _same_features(got, [want], f"1080p q={q} md={md} K={K}")


def test_batch_equals_single_frames_and_device_form_equals_host_form():
    import torch

    import _oflk
    import lucas_kanade_core as LK

    F, H, W, K, q, md = 6, 120, 160, 80, 0.01, 7.0
    for u8 in (False, True):
        frames = np.stack([_frame(H, W, seed=20 + s, u8=u8) for s in range(F)])
        frames[2] = 0   # one frame without features
        batch = LK.good_features_to_track_batch(frames, K, q, md)
        _same_features(batch, [M.good_features(f, 5, q, md, K) for f in frames], f"batch u8={u8}")
        for f in range(F):
            one = LK.good_features_to_track_batch(frames[f], K, q, md)
            _same_features(one, [(int(batch[2][f]), batch[0][f], batch[1][f])], f"single frame {f} u8={u8}")
        dev = torch.device("cuda", 0)
        nbytes = _oflk.good_features_workspace(F, H, W, 5, md, K)
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)   # garbage: the call needs no zeroed workspace
        d_f = _dev(frames)
        d_cnt = torch.full((F,), -1, dtype=torch.int32, device=dev)
        d_xy = torch.full((F, K, 2), 3.0, dtype=torch.float32, device=dev)
        d_sc = torch.full((F, K), 3.0, dtype=torch.float32, device=dev)
        _oflk.good_features(d_f.data_ptr(), F, H, W, ws.data_ptr(), nbytes, d_cnt.data_ptr(), d_xy.data_ptr(), d_sc.data_ptr(),
                            K, q, md, 5, u8=u8, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _same_features((d_xy.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy()),
                       [(int(batch[2][f]), batch[0][f], batch[1][f]) for f in range(F)], f"device form u8={u8}")


def test_device_form_replays_from_a_graph():
    import torch

    import _oflk

    F, H, W, K, q, md = 4, 240, 320, 500, 0.01, 6.0
    dev = torch.device("cuda", 0)
    frames = _dev(np.stack([_frame(H, W, seed=40 + s, u8=False) for s in range(F)]))
    nbytes = _oflk.good_features_workspace(F, H, W, 5, md, K)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    d_cnt = torch.empty((F,), dtype=torch.int32, device=dev)
    d_xy = torch.empty((F, K, 2), dtype=torch.float32, device=dev)
    d_sc = torch.empty((F, K), dtype=torch.float32, device=dev)

    def enqueue(s_):
        _oflk.good_features(frames.data_ptr(), F, H, W, ws.data_ptr(), nbytes, d_cnt.data_ptr(), d_xy.data_ptr(), d_sc.data_ptr(),
                            K, q, md, 5, stream=s_)

    enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    eager = (d_xy.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy())
    f_host = frames.cpu().numpy()
    _same_features(eager, [M.good_features(f, 5, q, md, K) for f in f_host], "eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        for t in (ws, d_cnt, d_xy, d_sc):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        _same_features((d_xy.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy()),
                       [(int(eager[2][f]), eager[0][f], eager[1][f]) for f in range(F)], f"replay {rep}")
    del g


# ---------------------------------------------------------------------------------------------------------------
# meaning
# ---------------------------------------------------------------------------------------------------------------
def test_detected_points_are_rectangle_corners():
    """bright rectangles on a flat background: every point lies within 2 px of a true corner; none on a flat area or a
    straight edge"""
    import lucas_kanade_core as LK

    H, W = 200, 300
    f = np.full((H, W), 40.0, np.float32)
    rects = [(20, 30, 60, 90), (100, 40, 170, 120), (30, 160, 90, 270), (120, 180, 180, 260)]   # y0, x0, y1, x1 (exclusive)
    corners = []
    for y0, x0, y1, x1 in rects:
        f[y0:y1, x0:x1] = 200.0
        corners += [(x0, y0), (x1 - 1, y0), (x0, y1 - 1), (x1 - 1, y1 - 1)]   # the corner pixels
    corners = np.array(corners)
    xy, sc = LK.good_features_to_track(f, 100, 0.05, 5.0, 5)
    assert len(xy) == len(corners), xy
    d = np.sqrt(((xy[:, None, :].astype(np.float64) - corners[None]) ** 2).sum(-1))
    assert (d.min(1) <= 2.0).all(), xy[d.min(1) > 2.0]
    assert (d.min(0) <= 2.0).all(), "every corner is found"


# ---------------------------------------------------------------------------------------------------------------
# detect, then track
# ---------------------------------------------------------------------------------------------------------------
def _klt_vs_pieces(frames, K, q, md, levels=3, win=5, iters=3):
    import _oflk
    import lucas_kanade_core as LK
    import lucas_kanade_pyramidal as P

    T, H, W = frames.shape
    u8 = frames.dtype == np.uint8
    xy, sc, cnt = LK.good_features_to_track_batch(frames[0], K, q, md, win)
    tracks = np.empty((T, K, 2), np.float32)
    vis = np.empty((T, K), np.uint8)
    L = _oflk.lib()
    fn = L.oflk_pyramidal_sequence_tracks_u8 if u8 else L.oflk_pyramidal_sequence_tracks
    src = frames.ctypes.data if u8 else _oflk.ptr(frames)
    _oflk.check(fn(src, T, H, W, levels, win, iters, 0.01, 0.5, None, _oflk.ptr(np.ascontiguousarray(xy[0])), K,
                   _oflk.ptr(tracks), vis.ctypes.data))
    # the C entry point of the combined call, every row
    k_cnt = np.zeros(1, np.int32)
    k_xy, k_sc = np.empty((K, 2), np.float32), np.empty(K, np.float32)
    k_tr, k_vis = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
    fn = L.oflk_pyramidal_sequence_klt_u8 if u8 else L.oflk_pyramidal_sequence_klt
    _oflk.check(fn(src, T, H, W, levels, win, iters, 0.01, 0.5, q, md, K, k_cnt.ctypes.data_as(_oflk._i32p), _oflk.ptr(k_xy),
                   _oflk.ptr(k_sc), _oflk.ptr(k_tr), k_vis.ctypes.data))
    assert int(k_cnt[0]) == int(cnt[0])
    _same(_norm(k_xy), _norm(xy[0]), "klt xy")
    _same(k_sc, sc[0], "klt score")
    _same(_norm(k_tr), _norm(tracks), "klt tracks")
    _same(k_vis, vis, "klt visible")
    # the Python call: trimmed to the count, equal to the tracks call on the trimmed features
    n = int(cnt[0])
    res = P.lucas_kanade_pyramidal_sequence_klt(frames, K, q, md, levels, win, iters)
    _same(res.xy, xy[0, :n], "python xy")
    _same(_norm(res.tracks), _norm(tracks[:, :n]), "python tracks")
    assert np.array_equal(res.visible, vis[:, :n].astype(bool))
    if n:
        ref = P.lucas_kanade_pyramidal_sequence_tracks(frames, LK.features_to_queries(xy, cnt), levels, win, iters)
        _same(_norm(ref.tracks), _norm(res.tracks), "tracks call on the features")
    return n, vis


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_klt_equals_detection_then_tracks_small(u8):
    frames = _video(6, 120, 160, seed=5, u8=u8)
    n, vis = _klt_vs_pieces(frames, 300, 0.01, 5.0)
    assert n > 50 and vis[0, :n].all() and vis[-1, :n].mean() > 0.5
    _klt_vs_pieces(frames, 7, 0.2, 12.0, win=7)                   # K below the number of features
    _klt_vs_pieces(frames[:3], 5000, 0.0, 0.0, levels=2, win=3)   # K above it: NaN queries are never-visible tracks


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_klt_equals_detection_then_tracks_chunked_1080p(u8):
    """17 frames of 1080p: four chunks under chunk_pairs"""
    frames = _video(17, 1080, 1920, seed=8, u8=u8)
    n, vis = _klt_vs_pieces(frames, 2000, 0.01, 10.0)
    assert n == 2000 and vis[-1].mean() > 0.5
