"""GPU tests of the point-track entry points (run on an MI355X: python -m pytest tests/test_gpu_tracks.py -m gpu -q).

oflk_track_points must equal the NumPy statement of tests/track_model.py byte for byte (NaN bit patterns normalised), on
every shape form, every (alpha, beta) of test_gpu_fb and queries on cell edges, on the last row and column and outside the
frame.  oflk_pyramidal_sequence_tracks must equal that statement on oflk_pyramidal_sequence_fb's flows, and through them the
CPU oracle.
"""
import numpy as np
import pytest

import fb_model as FM
import track_model as M
from test_gpu_fb import ALPHA_BETA, _host_fb, _same
from test_gpu_sequence import CASES, _dev, _video

pytestmark = pytest.mark.gpu


def _norm(tracks):
    """NaN bit patterns normalised to the canonical quiet NaN (everything else kept as bytes)"""
    t = np.array(tracks, np.float32, copy=True)
    t[np.isnan(t)] = np.float32(np.nan)
    return t


def _same_tracks(got, want, what):
    _same(_norm(got[0]), _norm(want[0]), f"{what}: tracks")
    _same(np.asarray(got[1], np.uint8), np.asarray(want[1], np.uint8), f"{what}: visible")


def _device_track(flows, qt, qxy, alpha=0.01, beta=0.5, t0=0, prev=None, zero_qt=False):
    """one oflk_track_points launch; prev = (row, visible) preset as row 0; qt None: d_qt NULL (zero_qt: an all-zero d_qt)"""
    import torch

    import _oflk

    B, H, W = flows[0].shape
    N = qxy.shape[0]
    d = [_dev(f) for f in flows]
    d_q = _dev(np.ascontiguousarray(qxy, np.float32))
    d_qt = _dev(np.zeros(N, np.int32) if zero_qt else np.asarray(qt, np.int32)) if (qt is not None or zero_qt) else None
    tr = torch.full((B + 1, N, 2), -7.0, dtype=torch.float32, device=d_q.device)
    vis = torch.full((B + 1, N), 9, dtype=torch.uint8, device=d_q.device)
    if prev is not None:
        tr[0] = torch.from_numpy(np.ascontiguousarray(prev[0], np.float32)).to(tr.device)
        vis[0] = torch.from_numpy(np.asarray(prev[1], np.uint8)).to(tr.device)
    _oflk.track_points(*(x.data_ptr() for x in d), B, H, W, d_q.data_ptr(), N, tr.data_ptr(), vis.data_ptr(), alpha, beta, t0,
                       d_qt.data_ptr() if d_qt is not None else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tr.cpu().numpy(), vis.cpu().numpy()


def _queries(B, H, W, N, seed):
    """mixed query frames in [0, B]: random points, points on cell edges (integers and half-integers), on the last row and
    column and at (W-1, H-1), and points outside the frame (just beyond an edge, NaN, inf)"""
    rng = np.random.default_rng(seed)
    xy = rng.random((N, 2)) * [W - 1, H - 1]
    k = N // 8
    xy[:k] = np.floor(xy[:k])
    xy[k:2 * k] = np.floor(xy[k:2 * k]) + 0.5
    xy[2 * k:2 * k + 4] = [[W - 1, H - 1], [W - 1, 0], [0, H - 1], [0, 0]]
    xy[2 * k + 4:3 * k, 0] = W - 1
    xy[3 * k:4 * k, 1] = H - 1
    xy = xy.astype(np.float32)
    bad = np.array([[-2.0 ** -20, 0], [W - 1 + 2.0 ** -18, 0], [0, H - 1 + 2.0 ** -18], [np.nan, 1], [1, np.inf],
                    [-1, -1]], np.float32)
    xy[4 * k:4 * k + len(bad)] = bad
    qt = rng.integers(0, B + 1, N).astype(np.int32)
    qt[:N // 2] = 0
    return qt, xy


SHAPES = sorted({(c[0], c[1]) for c in CASES} | {(1, 1), (1, 7), (9, 1), (1, 300), (64, 64)})


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda s: str(s))
def test_kernel_equals_statement(H, W):
    B = 6
    flows = M.smooth_flows(B, H, W, seed=H * 31 + W, scale=max(1.5, min(H, W) / 6))
    N = 1000 if H * W > 1 else 64
    qt, q = _queries(B, H, W, N, seed=W)
    for alpha, beta in ALPHA_BETA:
        want = M.track(*flows, qt, q, alpha, beta)
        got = _device_track(flows, qt, q, alpha, beta)
        _same_tracks(got, want, f"{H}x{W} alpha={alpha} beta={beta}")
    assert 0 < want[1][-1].sum() or H * W == 1


def test_flows_that_push_points_out():
    """a constant drift of 7.75 px per pair to the right with an exact backward flow: each point ends at the step that
    leaves the frame, and on the way stays exact"""
    B, H, W = 9, 20, 50
    flows = tuple(np.full((B, H, W), v, np.float32) for v in (7.75, 0.25, -7.75, -0.25))
    qt, q = _queries(B, H, W, 500, seed=3)
    want = M.track(*flows, qt, q)
    _same_tracks(_device_track(flows, qt, q), want, "drift")
    assert want[1][1].sum() < want[1][0].sum() and want[1][-1].sum() < want[1][1].sum()


def test_pieces_equal_one_call():
    B, H, W = 12, 37, 53
    flows = M.smooth_flows(B, H, W, seed=11, scale=3.0)
    qt, q = _queries(B, H, W, 2000, seed=12)
    one = _device_track(flows, qt, q)
    _same_tracks(one, M.track(*flows, qt, q), "one call")
    rows_tr, rows_vis, prev = [one[0][:0]], [one[1][:0]], None
    cuts = [0, 3, 7, 8, B]
    for a, b in zip(cuts[:-1], cuts[1:]):
        tr, vis = _device_track([f[a:b] for f in flows], qt, q, t0=a, prev=prev)
        k = 0 if a == 0 else 1
        rows_tr.append(tr[k:])
        rows_vis.append(vis[k:])
        prev = (tr[-1], vis[-1])
        if a > 0:   # row 0: read for earlier queries, rewritten (same values) for qt == t0, NaN for later ones
            assert np.array_equal(_norm(tr[0]).view(np.int32), _norm(one[0][a]).view(np.int32))
    _same_tracks((np.concatenate(rows_tr), np.concatenate(rows_vis)), one, "pieces")


def test_null_qt_equals_all_zero_qt():
    B, H, W = 5, 40, 48
    flows = M.smooth_flows(B, H, W, seed=5, scale=2.0)
    _, q = _queries(B, H, W, 700, seed=6)
    a = _device_track(flows, None, q)
    b = _device_track(flows, None, q, zero_qt=True)
    _same_tracks(a, b, "NULL d_qt")
    _same_tracks(a, M.track(*flows, None, q), "statement")


def test_flow_metrics_host_form_equals_statement():
    import flow_metrics

    B, H, W = 4, 45, 61
    flows = M.smooth_flows(B, H, W, seed=8, scale=3.0)
    qt, q = _queries(B, H, W, 900, seed=9)
    tr, vis = flow_metrics.track_points(*flows, np.concatenate([qt[:, None].astype(np.float32), q], 1), 0.02, 0.25)
    assert vis.dtype == bool
    _same_tracks((tr, vis), M.track(*flows, qt, q, 0.02, 0.25), "flow_metrics.track_points")
    tr, vis = flow_metrics.track_points(*flows, q)
    _same_tracks((tr, vis), M.track(*flows, None, q), "flow_metrics.track_points (N, 2)")


# ---------------------------------------------------------------------------------------------------------------
# the pipeline: frames in, tracks out
# ---------------------------------------------------------------------------------------------------------------
def _grid_queries(T, H, W, step, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    xy[::3] += rng.random((len(xy[::3]), 2)) * 0.9
    xy = np.minimum(xy, [W - 1, H - 1]).astype(np.float32)
    qt = rng.integers(0, T, len(xy))
    qt[::2] = 0
    return np.concatenate([qt[:, None].astype(np.float32), xy], 1)


@pytest.mark.parametrize("T,H,W", [(6, 240, 320), (3, 37, 53), (4, 23, 21)], ids=["small", "odd", "tiny"])
def test_sequence_tracks_equal_statement_on_fb_flows(T, H, W):
    import _oflk
    import lucas_kanade_pyramidal as P

    queries = _grid_queries(T, H, W, 3 if H * W < 5000 else 7, seed=T + W)
    results = {}
    for u8 in (False, True):
        frames = _video(T, H, W, seed=T + H, u8=True)
        if not u8:
            frames = frames.astype(np.float32)   # 8-bit values as float32: the uint8 path must give the same bytes
        for arith in (0, 2):
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
            try:
                fb, n_fb = _host_fb(frames, 3, 5, 3)
                r = P.lucas_kanade_pyramidal_sequence_tracks(frames, queries, 3, 5, 3)
                n_tr = int(_oflk.lib().oflk_last_resolved())
            finally:
                _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
            assert n_tr == n_fb
            want = M.track(*fb[:4], queries[:, 0].astype(np.int64), queries[:, 1:])
            _same_tracks(r, want, f"T={T} {H}x{W} arith {arith} {'u8' if u8 else 'f32'}")
            results[(u8, arith)] = r
    for arith in (0, 2):
        _same_tracks(results[(True, arith)], results[(False, arith)], f"u8 = f32, arith {arith}")


def test_chunked_1080p_equals_host_form_on_the_downloaded_flows():
    """T = 18 at 1080p: the chunk rule (chunk_pairs) cuts the 17 pairs into chunks of 4, 4, 4, 4 and 1"""
    import flow_metrics
    import lucas_kanade_pyramidal as P

    T, H, W = 18, 1080, 1920
    frames = _video(T, H, W, seed=4, u8=True)
    queries = _grid_queries(T, H, W, 24, seed=1)
    r = P.lucas_kanade_pyramidal_sequence_tracks(frames, queries)
    fb, _ = _host_fb(frames, 3, 5, 3)
    host = flow_metrics.track_points(*fb[:4], queries)
    _same_tracks(r, host, "1080p pipeline vs host form")
    _same_tracks(r, M.track(*fb[:4], queries[:, 0].astype(np.int64), queries[:, 1:]), "1080p statement")
    assert r.visible[-1].mean() > 0.3


def test_oracle_anchors_the_tracks(oracle):
    """on a small sequence the tracks equal the statement on the CPU oracle's flows of both directions"""
    import lucas_kanade_pyramidal as P

    T, H, W = 5, 60, 80
    frames = _video(T, H, W, seed=17)
    fl = [[], [], [], []]
    for t in range(T - 1):
        for lst, a in zip(fl, oracle.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3) +
                          oracle.lucas_kanade_pyramidal(frames[t + 1], frames[t], 3, 5, 3)):
            lst.append(a)
    flows = [np.stack(x) for x in fl]
    queries = _grid_queries(T, H, W, 2, seed=3)
    r = P.lucas_kanade_pyramidal_sequence_tracks(frames, queries)
    _same_tracks(r, M.track(*flows, queries[:, 0].astype(np.int64), queries[:, 1:]), "oracle flows")
    assert 0.2 < r.visible[-1].mean()


def test_occluder_scene_meaning(oracle):
    import lucas_kanade_pyramidal as P

    T, S = 5, M.SCENE
    frames, corners = FM.occluder_scene(T, S["H"], S["W"], S["size"], S["step"])
    fl = [[], [], [], []]
    for t in range(T - 1):
        for lst, a in zip(fl, oracle.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3) +
                          oracle.lucas_kanade_pyramidal(frames[t + 1], frames[t], 3, 5, 3)):
            lst.append(a)
    flows = [np.stack(x) for x in fl]

    def run(q):
        r = P.lucas_kanade_pyramidal_sequence_tracks(frames, q)
        want = M.track(*flows, q[:, 0].astype(np.int64), q[:, 1:])
        _same_tracks(r, want, "scene")
        return r.tracks, r.visible

    M.check_scene_tracks(run, T, corners, S["H"], S["W"], S["size"], S["step"])


# ---------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_fb_pass_and_tracks_replay_from_a_graph():
    """after one eager call, the bidirectional plan pass and the track launch captured on a side stream replay to the eager
    bytes"""
    import torch

    import _oflk

    T, H, W, L, K = 6, 240, 320, 3, 3
    B = T - 1
    dev = torch.device("cuda", 0)
    frames = _dev(_video(T, H, W, seed=21))
    queries = _grid_queries(T, H, W, 5, seed=2)
    N = len(queries)
    d_q = _dev(np.ascontiguousarray(queries[:, 1:]))
    d_qt = _dev(queries[:, 0].astype(np.int32))
    d = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(4)]
    tr = torch.empty((B + 1, N, 2), dtype=torch.float32, device=dev)
    vis = torch.empty((B + 1, N), dtype=torch.uint8, device=dev)
    for arith in (0, 2):
        plan = _oflk.Plan(0, B, H, W, L, 5, K)
        try:
            plan.set_arithmetic(arith)

            def enqueue(s_):
                plan.pyramidal_sequence_fb(frames.data_ptr(), *(t.data_ptr() for t in d), s_)
                _oflk.track_points(*(t.data_ptr() for t in d), B, H, W, d_q.data_ptr(), N, tr.data_ptr(), vis.data_ptr(),
                                   d_qt=d_qt.data_ptr(), stream=s_)

            enqueue(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            eager = (tr.cpu().numpy(), vis.cpu().numpy())
            flows = [t.cpu().numpy() for t in d]
            _same_tracks(eager, M.track(*flows, queries[:, 0].astype(np.int64), queries[:, 1:]), f"arith {arith} eager")
            side = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                enqueue(torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                for t in d + [tr, vis]:
                    t.zero_()
                g.replay()
                torch.cuda.synchronize()
                _same_tracks((tr.cpu().numpy(), vis.cpu().numpy()), eager, f"arith {arith} replay {rep}")
            del g
        finally:
            plan.close()
