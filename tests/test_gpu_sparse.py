"""GPU tests of the sparse pyramidal LK entry points (run on an MI355X: python -m pytest tests/test_gpu_sparse.py -m gpu -q).

oflk_sparse_lk must equal step() of tests/sparse_model.py byte for byte (positions, status, residual; NaN bit patterns
normalised), oflk_plan_sparse_tracks and the host sequence forms must equal its track statement, and the dense tracks on a
plan shape that sparse calls have used must still equal their own statement.
"""
import numpy as np
import pytest

import fb_model as FM
import sparse_model as S
import track_model as TM
from test_gpu_fb import _same
from test_gpu_sequence import _dev
from test_gpu_tracks import _norm, _queries, _same_tracks
from test_sparse_cpu import SHIFTS, _drifting, check_subpixel, subpixel_case

pytestmark = pytest.mark.gpu


def _smooth(H, W, seed):
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    f = gaussian_filter(rng.random((H, W)) * 255.0, 1.2, mode="nearest")
    return ((f - f.min()) / max(f.max() - f.min(), 1e-9) * 230.0 + 10.0).astype(np.float32)


def _shifted(a, dx, dy):
    from scipy.ndimage import shift

    return shift(a.astype(np.float64), (dy, dx), order=1, mode="nearest").astype(np.float32)


def _same_lk(got, want, what):
    _same(_norm(got[0]), _norm(want[0]), f"{what}: next points")
    _same(np.asarray(got[1], np.uint8), np.asarray(want[1], np.uint8), f"{what}: status")
    _same(_norm(got[2]), _norm(want[2]), f"{what}: residual")


# shape, levels, window, iterations: every window and K in {1, 3, 5}; (8, 8) at 3 levels has a 2 x 2 coarsest level
PAIR_CASES = [((8, 8), 3, 3, 1), ((24, 32), 3, 5, 3), ((33, 47), 2, 7, 5), ((96, 128), 3, 9, 3), ((5, 300), 1, 11, 5),
              ((24, 32), 3, 11, 1), ((33, 47), 2, 3, 3)]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,L,w,K", PAIR_CASES, ids=lambda v: str(v))
def test_sparse_lk_equals_step(shape, L, w, K, u8):
    import lucas_kanade_pyramidal as P

    H, W = shape
    a, b = _smooth(H, W, H * 7 + W), _smooth(H, W, H * 7 + W + 1)
    c = _shifted(a, 1.3, -0.6)
    _, pts = _queries(1, H, W, 300, seed=W + w)
    moved = 0
    for name, (p, q) in (("two frames", (a, b)), ("shifted copy", (a, c))):
        if u8:
            p, q = np.rint(p).astype(np.uint8), np.rint(q).astype(np.uint8)
        want = S.sparse_lk(p, q, pts, L, w, K)
        got = P.lucas_kanade_sparse(p, q, pts, L, w, K)
        assert got[1].dtype == bool
        _same_lk(got, want, f"{H}x{W} L={L} w={w} K={K} {name}")
        moved += int(want[1].sum())
    assert moved > 50   # most points solve


@pytest.mark.parametrize("value", [0.0, 80.0])
def test_constant_frames(value):
    """identical constant frames: no point moves; a frame of zeros solves nothing (status 0 everywhere)"""
    import lucas_kanade_pyramidal as P

    H, W = 24, 32
    f = np.full((H, W), value, np.float32)
    _, pts = _queries(1, H, W, 300, seed=5)
    want = S.sparse_lk(f, f, pts, 3, 5, 3)
    got = P.lucas_kanade_sparse(f, f, pts, 3, 5, 3)
    _same_lk(got, want, f"constant {value}")
    inside = ~np.isnan(got[0][:, 0])
    assert inside.sum() > 280 and np.array_equal(got[0][inside], pts[inside] + np.float32(0))
    if value == 0.0:
        assert not got[1].any()
    _same_lk(P.lucas_kanade_sparse(f.astype(np.uint8), f.astype(np.uint8), pts, 3, 5, 3), want, f"constant {value} u8")


@pytest.mark.parametrize("dx,dy", SHIFTS)
def test_subpixel_and_large_motion(dx, dy):
    import lucas_kanade_pyramidal as P

    a, b, pts = subpixel_case(dx, dy)
    nxt, status, _ = P.lucas_kanade_sparse(a, b, pts, 3, 5, 3)
    check_subpixel(nxt, status, pts, dx, dy)


# ---------------------------------------------------------------------------------------------------------------
# the device form
# ---------------------------------------------------------------------------------------------------------------
def _device_sparse(plan, frames, qt, qxy, alpha=0.01, beta=0.5, mr=4.0, t0=0, prev=None, zero_qt=False):
    """one oflk_plan_sparse_tracks launch on frames (B+1, H, W); prev = (row, visible) preset as row 0; qt None: d_qt NULL
    (zero_qt: an all-zero d_qt); the output buffers are prefilled with sentinels"""
    import torch

    import _oflk

    B, N = frames.shape[0] - 1, qxy.shape[0]
    d_f, d_q = _dev(frames), _dev(np.ascontiguousarray(qxy, np.float32))
    d_qt = _dev(np.zeros(N, np.int32) if zero_qt else np.asarray(qt, np.int32)) if (qt is not None or zero_qt) else None
    tr = torch.full((B + 1, N, 2), -7.0, dtype=torch.float32, device=d_q.device)
    vis = torch.full((B + 1, N), 9, dtype=torch.uint8, device=d_q.device)
    if prev is not None:
        tr[0] = torch.from_numpy(np.ascontiguousarray(prev[0], np.float32)).to(tr.device)
        vis[0] = torch.from_numpy(np.asarray(prev[1], np.uint8)).to(tr.device)
    _oflk.sparse_tracks(plan, d_f.data_ptr(), d_q.data_ptr(), N, tr.data_ptr(), vis.data_ptr(), alpha, beta, mr, t0,
                        d_qt.data_ptr() if d_qt is not None else 0, u8=frames.dtype == np.uint8,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tr.cpu().numpy(), vis.cpu().numpy()


@pytest.fixture(scope="module")
def clip():
    """five frames (B = 4), mixed queries, the frames' pyramids and the statement's tracks, computed once"""
    T, H, W = 5, 40, 52
    frames = _drifting(T, H, W, 3)
    qt, qxy = _queries(T - 1, H, W, 400, seed=8)
    pyr = [S.pyramid(f, 3) for f in frames]
    want = S.track(frames, qt, qxy, 3, 5, 3, pyramids=pyr)
    assert 100 < want[1][-1].sum() < want[1][0].sum() + (qt > 0).sum()
    return dict(frames=frames, qt=qt, qxy=qxy, pyr=pyr, want=want)


def test_plan_sparse_tracks_equal_statement(clip):
    import _oflk

    frames, qt, qxy = clip["frames"], clip["qt"], clip["qxy"]
    T, H, W = frames.shape
    plan = _oflk.Plan(0, T - 1, H, W, 3, 5, 3)
    half = _oflk.Plan(0, 2, H, W, 3, 5, 3)
    try:
        ws0 = plan.workspace_bytes
        one = _device_sparse(plan, frames, qt, qxy)
        _same_tracks(one, clip["want"], "one launch")
        # nothing was allocated for the call: these levels take the fused pyramid kernel, and there is no flow to hold
        dims = S.O.pyramid_dims(H, W, 3)
        assert all(_oflk.lib().oflk_pyramid_step_fused(*dims[l + 1], *dims[l], 8) for l in range(2))
        assert plan.workspace_bytes == ws0
        a = _device_sparse(half, frames[:3], qt, qxy)
        b = _device_sparse(half, frames[2:], qt, qxy, t0=2, prev=(a[0][-1], a[1][-1]))
        _same_tracks((np.concatenate([a[0], b[0][1:]]), np.concatenate([a[1], b[1][1:]])), one, "two launches")
        assert np.array_equal(_norm(b[0][0]).view(np.int32), _norm(one[0][2]).view(np.int32))   # row 0 as oflk_track_points
        u8 = np.rint(frames).astype(np.uint8)
        _same_tracks(_device_sparse(plan, u8, qt, qxy, 0.02, 0.25, 6.0),
                     S.track(u8, qt, qxy, 3, 5, 3, 0.02, 0.25, 6.0), "uint8 frames, other thresholds")
        # the first dense pass brings the flow slots (two float2 slots per level) and the blur temporaries
        import torch

        d_f = _dev(frames)
        d_u, d_v = (torch.empty((T - 1, H, W), dtype=torch.float32, device=d_f.device) for _ in range(2))
        plan.pyramidal_sequence(d_f.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert plan.workspace_bytes >= ws0 + 16 * (T - 1) * H * W
        _same_tracks(_device_sparse(plan, frames, qt, qxy), one, "after a dense pass on the same plan")
    finally:
        plan.close()
        half.close()


def test_null_qt_equals_all_zero_qt(clip):
    import _oflk

    frames, qxy = clip["frames"], clip["qxy"]
    T, H, W = frames.shape
    plan = _oflk.Plan(0, T - 1, H, W, 3, 5, 3)
    try:
        a = _device_sparse(plan, frames, None, qxy)
        b = _device_sparse(plan, frames, None, qxy, zero_qt=True)
    finally:
        plan.close()
    _same_tracks(a, b, "NULL d_qt")
    _same_tracks(a, S.track(frames, None, qxy, 3, 5, 3, pyramids=clip["pyr"]), "statement")


def test_other_windows_and_levels_track(clip):
    """the track kernel's other instantiations: 7x7 at 2 levels and 5 iterations, 3x3 at 1 level and 1 iteration"""
    import _oflk

    frames, qt, qxy = clip["frames"][:3], np.minimum(clip["qt"], 2)[:150], clip["qxy"][:150]
    for L, w, K in ((2, 7, 5), (1, 3, 1), (3, 11, 2), (2, 9, 3)):
        plan = _oflk.Plan(0, 2, frames.shape[1], frames.shape[2], L, w, K)
        try:
            got = _device_sparse(plan, frames, qt, qxy)
        finally:
            plan.close()
        _same_tracks(got, S.track(frames, qt, qxy, L, w, K), f"L={L} w={w} K={K}")


# ---------------------------------------------------------------------------------------------------------------
# the host sequence forms
# ---------------------------------------------------------------------------------------------------------------
def test_sequence_forms_equal_statement(clip):
    import lucas_kanade_pyramidal as P

    frames, qt, qxy = clip["frames"], clip["qt"], clip["qxy"]
    queries = np.concatenate([qt[:, None].astype(np.float32), qxy], 1)
    r = P.lucas_kanade_pyramidal_sequence_sparse_tracks(frames, queries)
    assert r.visible.dtype == bool
    _same_tracks(r, clip["want"], "float32")
    u8 = np.rint(frames).astype(np.uint8)
    want = S.track(u8, qt, qxy, 3, 5, 3)
    _same_tracks(P.lucas_kanade_pyramidal_sequence_sparse_tracks(u8, queries), want, "uint8")
    _same_tracks(P.lucas_kanade_pyramidal_sequence_sparse_tracks(u8.astype(np.float32), queries), want, "8-bit values as float32")
    r2 = P.lucas_kanade_pyramidal_sequence_sparse_tracks(frames, qxy, max_residual=np.inf)
    _same_tracks(r2, S.track(frames, None, qxy, 3, 5, 3, max_residual=np.inf, pyramids=clip["pyr"]), "(N, 2) queries, no residual test")


def test_a_long_sequence_is_cut_into_chunks():
    """T = 70 small frames: the chunk rule holds at most 64 pairs, so the 69 pairs go as 64 + 5 with the row carried"""
    import lucas_kanade_pyramidal as P

    T, H, W = 70, 24, 32
    from scipy.ndimage import gaussian_filter, shift

    rng = np.random.default_rng(9)
    base = gaussian_filter(rng.random((H + 40, W + 60)) * 255.0, 1.5)
    base = (base - base.min()) / (base.max() - base.min()) * 220.0 + 15.0
    frames = np.stack([shift(base, (0.11 * t, -0.23 * t), order=1, mode="nearest")[20:20 + H, 40:40 + W] +
                       rng.normal(0, 0.7, (H, W)) for t in range(T)]).astype(np.float32)
    qt, qxy = _queries(T - 1, H, W, 96, seed=4)
    queries = np.concatenate([qt[:, None].astype(np.float32), qxy], 1)
    want = S.track(frames, qt, qxy, 3, 5, 3)
    assert want[1][65:].sum() > 20   # tracks live across the cut
    _same_tracks(P.lucas_kanade_pyramidal_sequence_sparse_tracks(frames, queries), want, "70 frames")
    # The detect-then-track form across the same cut: its detection runs once, ahead of chunk 0, and chunk 1 continues
    # the carried row.  It must equal the given-queries form on its own corners (which the line above ties to the
    # statement).  Live marks are counted as above, over rows 65 .. 69: tests/sparse_model.py on these frames with
    # min_distance = 3 gives 31 (float32: 16 corners, 7 alive on frame 65) and 21 (uint8: 16 corners, 5 alive).  The
    # 24 x 32 scene has no more than 19 corners at any min_distance, so the count cannot be of distinct tracks.
    for name, f in (("float32", frames), ("uint8", np.rint(frames).astype(np.uint8))):
        r = P.lucas_kanade_pyramidal_sequence_klt_sparse(f, 96, 0.01, 3.0)
        assert r.visible[65:].sum() >= 20 and r.visible[65].sum() >= 5, name   # marks after the cut; tracks that cross it
        _same_tracks((r.tracks, r.visible), P.lucas_kanade_pyramidal_sequence_sparse_tracks(f, r.xy), f"klt_sparse, {name}")


def _scene():
    T, Sc = 5, TM.SCENE
    frames, corners = FM.occluder_scene(T, Sc["H"], Sc["W"], Sc["size"], Sc["step"])
    return T, Sc, frames, corners


def test_klt_sparse_is_detection_then_sparse_tracks():
    import lucas_kanade_core as C
    import lucas_kanade_pyramidal as P

    _, _, frames, _ = _scene()
    r = P.lucas_kanade_pyramidal_sequence_klt_sparse(frames, 150, 0.01, 6.0)
    xy, _ = C.good_features_to_track(frames[0], 150, 0.01, 6.0, 5)
    assert len(xy) > 50
    _same(r.xy, xy, "features")
    _same_tracks((r.tracks, r.visible), P.lucas_kanade_pyramidal_sequence_sparse_tracks(frames, xy), "tracks")
    _same_tracks((r.tracks, r.visible), S.track(frames, None, xy, 3, 5, 3), "statement")


def test_occluder_scene_meaning_and_dense_tracks_untouched(oracle):
    """the meaning check through the host entry point (which equals the statement on the way), and then, on the plan shape
    the sparse calls have just used and cached, the dense tracks: still their own statement on the oracle's flows"""
    import lucas_kanade_pyramidal as P

    T, Sc, frames, corners = _scene()
    pyr = [S.pyramid(f, 3) for f in frames]

    def run(q, mr=4.0):
        r = P.lucas_kanade_pyramidal_sequence_sparse_tracks(frames, q, max_residual=mr)
        _same_tracks(r, S.track(frames, q[:, 0].astype(np.int64), q[:, 1:], 3, 5, 3, max_residual=mr, pyramids=pyr), "scene")
        return r.tracks, r.visible

    S.check_scene_sparse_tracks(run, T, corners, Sc["H"], Sc["W"], Sc["size"], Sc["step"], run_no_residual=lambda q: run(q, np.inf))

    fl = [[], [], [], []]
    for t in range(T - 1):
        for lst, a in zip(fl, oracle.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3) +
                          oracle.lucas_kanade_pyramidal(frames[t + 1], frames[t], 3, 5, 3)):
            lst.append(a)
    flows = [np.stack(x) for x in fl]
    square, _, covered = TM.scene_queries(corners, T, Sc["H"], Sc["W"], Sc["size"], Sc["step"])
    for q in (square, covered[1]):
        r = P.lucas_kanade_pyramidal_sequence_tracks(frames, q)
        _same_tracks(r, TM.track(*flows, q[:, 0].astype(np.int64), q[:, 1:]), "dense tracks after sparse calls")
        r = P.lucas_kanade_pyramidal_sequence_sparse_tracks(frames, q)   # and back again on the same plan
        _same_tracks(r, S.track(frames, q[:, 0].astype(np.int64), q[:, 1:], 3, 5, 3, pyramids=pyr), "sparse after dense")


# ---------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_sparse_tracks_replay_from_a_graph(clip):
    """after one eager call, the device form captured on a side stream replays to the eager rows"""
    import torch

    import _oflk

    frames, qt, qxy = clip["frames"], clip["qt"], clip["qxy"]
    T, H, W = frames.shape
    N = len(qxy)
    d_f, d_q, d_qt = _dev(frames), _dev(qxy), _dev(qt.astype(np.int32))
    tr = torch.empty((T, N, 2), dtype=torch.float32, device=d_f.device)
    vis = torch.empty((T, N), dtype=torch.uint8, device=d_f.device)
    plan = _oflk.Plan(0, T - 1, H, W, 3, 5, 3)
    try:
        def enqueue(s_):
            _oflk.sparse_tracks(plan, d_f.data_ptr(), d_q.data_ptr(), N, tr.data_ptr(), vis.data_ptr(), d_qt=d_qt.data_ptr(), stream=s_)

        enqueue(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        eager = (tr.cpu().numpy(), vis.cpu().numpy())
        _same_tracks(eager, clip["want"], "eager")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            enqueue(torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            tr.zero_()
            vis.zero_()
            g.replay()
            torch.cuda.synchronize()
            _same_tracks((tr.cpu().numpy(), vis.cpu().numpy()), eager, f"replay {rep}")
        del g
    finally:
        plan.close()
