"""GPU tests of direct image alignment (run on an MI355X: python -m pytest tests/test_gpu_align.py -m gpu -q).

The model, the status and the stats of oflk_align_refine, oflk_align_sequence and their host forms must equal the statement
(tests/align_model.py) byte for byte, a NaN equal to a NaN: float32 and uint8 frames, affine and homography models, at the
smallest sizes at which the reduction can go wrong -- one partial tile, exactly one tile column, a tile column past a multiple
by one pixel, several tile rows -- with one and three levels, one and four iterations, and every kind of step in one call.  No
tolerance anywhere but in the one end-to-end accuracy case, whose yardstick is the planted chain.
"""
import numpy as np
import pytest

import align_model as AM
import mosaic_model as M
import stabilize_model as SM

pytestmark = pytest.mark.gpu

KINDS = [("homography", AM.HOMOGRAPHY), ("affine", AM.AFFINE)]
SIZES = [(33, 47), (64, 64), (70, 257), (96, 130)]


def _as(frames, dtype):
    return np.rint(frames).astype(np.uint8) if dtype == np.uint8 else np.ascontiguousarray(frames, np.float32)


def _mixed_steps(H, W, kind, seed):
    """S = 5 steps of every sort in one call: (a, b (5, H, W) float32, model (5, nc) float32, status (5,) int32)
    0  equal frames under the identity      1  a held step (status 0) of a planted pair
    2  a model that throws b off the frame  3  a planted pair seen through a shift of a third of the frame: the mask matters
    4  a flat template"""
    A, B, planted = AM.planted_pair(H, W, seed, kind, move=2.0)
    ident = AM.IDENTITY[kind]
    off = ident.copy()
    off[2], off[5] = 3.0 * W, -2.0 * H
    dx = float(W // 3)
    canvas = AM.texture(H, W + W // 3, seed + 1)
    wide = AM.view(canvas, H, W + W // 3, AM.IDENTITY[AM.HOMOGRAPHY])
    shifted = ident.copy()
    shifted[2] = 0.4 - dx
    a = np.stack([A, A, A, wide[:, :W], np.full((H, W), 9.0, np.float32)])
    b = np.stack([A, B, B, wide[:, W // 3:], B])
    model = np.stack([ident, AM.pushed(planted, H, W, kind, 0.5), off, shifted, ident])
    return a, b, model, np.array([1, 0, 1, 1, 1], np.int32)


def _device(a, b, model, status, code, levels, iterations, min_share=0.25, sequence=False):
    """the device form: outputs preset with bytes that the call must overwrite; b None with sequence"""
    import torch

    import _oflk

    d = "cuda:0"
    S = len(model)
    H, W = a.shape[1:]
    u8 = a.dtype == np.uint8
    nbytes = _oflk.align_workspace(S, H, W, levels, code)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=d)
    t_a = torch.from_numpy(a).to(d)
    t_b = None if sequence else torch.from_numpy(b).to(d)
    t_model = torch.from_numpy(np.ascontiguousarray(model, np.float32)).to(d)
    t_status = None if status is None else torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(d)
    out = torch.full(model.shape, -7.0, dtype=torch.float32, device=d)
    st = torch.full((S,), 9, dtype=torch.int32, device=d)
    stats = torch.full((S, 4), -7.0, dtype=torch.float64, device=d)
    tail = (H, W, levels, iterations, code, min_share, t_model.data_ptr(), 0 if t_status is None else t_status.data_ptr(), ws.data_ptr(),
            nbytes, out.data_ptr(), st.data_ptr(), stats.data_ptr(), u8)
    if sequence:
        _oflk.align_sequence(t_a.data_ptr(), S + 1, *tail)
    else:
        _oflk.align_refine(t_a.data_ptr(), t_b.data_ptr(), S, *tail)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_every_kind_of_step_equals_the_model(oracle, H, W, kind, code, dtype):
    import _oflk

    a, b, model, status = _mixed_steps(H, W, code, H + W)
    a, b = _as(a, dtype), _as(b, dtype)
    seen = set()
    for levels, iterations in ((1, 1), (3, 4)):
        want = AM.refine(a, b, model, status, code, levels, iterations)
        what = f"{W}x{H} {kind} {np.dtype(dtype).name} L={levels} n={iterations}"
        AM.same(_device(a, b, model, status, code, levels, iterations), want, what + " device")
        AM.same(_oflk.align_host(a, b, model, status, levels, iterations, code, 0.25), want, what + " host")
        seen |= set(want[1].tolist())
        assert want[1][0] == 1 and want[0][0].tobytes() == AM.IDENTITY[code].tobytes() and want[2][0, 3] == levels * iterations
        assert want[1][1] == 0 and want[1][2] == 0 and want[1][4] == 0 and not want[2][1].any() and np.isnan(want[2][2, 0])
        assert want[1][3] != 0 and 0.3 < want[2][3, 2] < 0.75   # the shifted step is refined on the overlap alone
    assert seen >= {0, 1}


@pytest.mark.parametrize("kind,code", KINDS)
def test_one_step_no_status_and_a_rejected_step(oracle, kind, code):
    import _oflk

    A, B, planted = AM.planted_pair(70, 257, 5, code)
    m0 = AM.pushed(planted, 70, 257, code)[None]
    for levels, iterations in ((1, 1), (3, 4)):
        want = AM.refine(A[None], B[None], m0, None, code, levels, iterations)
        assert want[1][0] == 1 and AM.corner_error(want[0][0], planted, 70, 257) < AM.corner_error(m0[0], planted, 70, 257)
        AM.same(_device(A[None], B[None], m0, None, code, levels, iterations), want, f"S=1 {kind} device")
        AM.same(_oflk.align_host(A[None], B[None], m0, None, levels, iterations, code, 0.25), want, f"S=1 {kind} host")
    ca, cb = AM.checker_pair(40, 56)
    ident = AM.IDENTITY[code][None]
    want = AM.refine(ca[None], cb[None], ident, None, code, 1, 1)
    assert want[1][0] == 2
    AM.same(_device(ca[None], cb[None], ident, None, code, 1, 1), want, f"rejected {kind}")
    # min_share: the shifted step of the mixed call freezes at once when more than its overlap is asked for
    a, b, model, status = _mixed_steps(64, 64, code, 128)
    want = AM.refine(a[3:4], b[3:4], model[3:4], None, code, 1, 2, 0.9)
    assert want[1][0] == 0 and want[2][0, 3] == 0
    AM.same(_device(a[3:4], b[3:4], model[3:4], None, code, 1, 2, 0.9), want, f"min_share {kind}")


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_the_sequence_form_equals_the_pair_form_and_two_runs_agree(oracle, dtype):
    import _oflk

    frames, _ = M.pan_frames(M.smooth_field(48 + 8, 70 + 3 * 5 + 8, 11), 6, 48, 70, 3, 0, 4, 4)
    frames = _as(frames.astype(np.float32), dtype)
    for kind, code in KINDS:
        model = np.stack([AM.IDENTITY[code]] * 5)
        model[:, 2] = -2.5
        model[3, 2] = np.nan
        status = np.array([1, 1, 0, 1, 1], np.int32)
        want = AM.sequence(frames, model, status, code, 2, 3)
        assert want[1].tolist() == [1, 1, 0, 0, 1]
        pair = _device(frames[:-1].copy(), frames[1:].copy(), model, status, code, 2, 3)
        AM.same(pair, want, f"{kind} pair form")
        seq = _device(frames, None, model, status, code, 2, 3, sequence=True)
        AM.same(seq, want, f"{kind} sequence form")
        AM.same(_device(frames, None, model, status, code, 2, 3, sequence=True), seq, f"{kind} second run")
        AM.same(_oflk.align_host(frames, None, model, status, 2, 3, code, 0.25), want, f"{kind} sequence host form")


def test_the_device_form_replays_from_a_graph_on_new_frames(oracle):
    """one chain of launches and nothing else: captured once after one eager call and replayed on new frame contents (the
    process keeps the default number of hardware queues); the outputs are scribbled over between replays"""
    import torch

    import _oflk

    d, S, H, W, L, n, code = "cuda:0", 2, 40, 70, 2, 2, AM.HOMOGRAPHY
    nbytes = _oflk.align_workspace(S, H, W, L, code)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    t_a, t_b = torch.zeros((S, H, W), dtype=torch.float32, device=d), torch.zeros((S, H, W), dtype=torch.float32, device=d)
    model = np.stack([AM.IDENTITY[code]] * S)
    t_model = torch.from_numpy(model).to(d)
    out, st, stats = torch.empty_like(t_model), torch.empty(S, dtype=torch.int32, device=d), torch.empty((S, 4), dtype=torch.float64, device=d)

    def enqueue(stream):
        _oflk.align_refine(t_a.data_ptr(), t_b.data_ptr(), S, H, W, L, n, code, 0.25, t_model.data_ptr(), 0, ws.data_ptr(), nbytes,
                           out.data_ptr(), st.data_ptr(), stats.data_ptr(), False, stream)

    def scene(seed):
        pairs = [AM.planted_pair(H, W, seed + k, code, move=1.0)[:2] for k in range(S)]
        a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        t_a.copy_(torch.from_numpy(a))
        t_b.copy_(torch.from_numpy(b))
        return AM.refine(a, b, model, None, code, L, n)

    want = scene(40)
    enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    AM.same((out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy()), want, "eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        want = scene(50 + 10 * rep)
        out.fill_(-7.0)
        st.fill_(9)
        stats.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        AM.same((out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy()), want, f"replay {rep}")
        assert (want[1] == 1).all()
    del g


def test_the_host_forms_over_a_chunk_boundary_equal_one_chunk(oracle):
    """the host forms go up in chunks of at most 64 steps: 66 steps are 64 + 2 (the sequence form: 65 + 3 frames, the boundary
    frame shared); every step must equal the same step refined alone in one chunk, which is the model's"""
    import _oflk

    S, H, W = 66, 16, 24
    rng = np.random.default_rng(2)
    base = AM.texture(H, W + S + 2, 9, sigma=1.5, margin=0)
    frames = np.stack([base[:, t:t + W] for t in range(S + 1)]).astype(np.float32)
    frames += rng.standard_normal(frames.shape).astype(np.float32)
    model = np.stack([AM.IDENTITY[AM.AFFINE]] * S)
    model[:, 2] = -0.5
    want = AM.sequence(frames, model, None, AM.AFFINE, 1, 2)
    assert (want[1] == 1).sum() > S // 2
    AM.same(_oflk.align_host(frames, None, model, None, 1, 2, AM.AFFINE, 0.25), want, "sequence host form, 66 steps")
    a, b = frames[:-1].copy(), frames[1:].copy()
    AM.same(_oflk.align_host(a, b, model, None, 1, 2, AM.AFFINE, 0.25), want, "pair host form, 66 steps")
    for s in (0, 63, 64, 65):
        AM.same(_oflk.align_host(a[s:s + 1], b[s:s + 1], model[s:s + 1], None, 1, 2, AM.AFFINE, 0.25), tuple(x[s:s + 1] for x in want),
                f"step {s} alone")


def test_the_python_functions_return_the_model(oracle):
    import lucas_kanade_core as K

    A, B, planted = AM.planted_pair(64, 64, 3, AM.HOMOGRAPHY)
    m0 = AM.pushed(planted, 64, 64, AM.HOMOGRAPHY)
    want = AM.refine(A[None], B[None], m0[None], None, AM.HOMOGRAPHY, 3, 5)
    one = K.refine_alignment(A, B, m0.reshape(3, 3))
    assert one.model.shape == (3, 3) and one.status == 1 and one.stats.shape == (4,)
    AM.same((one.model.reshape(1, 9), np.array([one.status], np.int32), one.stats[None]), want, "refine_alignment, one step")
    frames = np.stack([A, B, A])
    models = np.stack([m0, AM.IDENTITY[AM.HOMOGRAPHY]]).reshape(2, 3, 3)
    got = K.sequence_refine_alignment(frames, models, [1, 0], levels=2, iterations=2)
    AM.same((got.model.reshape(2, 9), got.status, got.stats), AM.sequence(frames, models, [1, 0], AM.HOMOGRAPHY, 2, 2), "sequence")
    aff = K.refine_alignment(frames[:2], frames[1:], np.stack([AM.IDENTITY[AM.AFFINE]] * 2), kind="affine", levels=2, iterations=3)
    assert aff.model.shape == (2, 2, 3)
    AM.same((aff.model.reshape(2, 6), aff.status, aff.stats),
            AM.refine(frames[:2], frames[1:], np.stack([AM.IDENTITY[AM.AFFINE]] * 2), None, AM.AFFINE, 2, 3), "affine batch")
    for bad in (dict(kind="similarity"), dict(levels=0), dict(iterations=0), dict(min_share=0.0), dict(min_share=1.5)):
        with pytest.raises(ValueError):
            K.refine_alignment(A, B, m0, **bad)
    with pytest.raises(ValueError):
        K.refine_alignment(A, B[:32], m0)
    with pytest.raises(ValueError):
        K.sequence_refine_alignment(frames, models[:1])


def _pan(T, H, W, step, seed):
    image = M.smooth_field(H + 8, W + step * (T - 1) + 8, seed)
    frames, _ = M.pan_frames(image, T, H, W, step, 0, 4, 4)
    return image, frames


def test_refine_iterations_zero_is_todays_call_and_above_zero_the_chain_of_parts():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    _, frames = _pan(8, 96, 128, 5, 3)
    kw = dict(max_corners=300, detect_every=4)
    # the mosaic
    base = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=3, **kw)
    zero = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=3, refine_iterations=0, **kw)
    for g, w, name in zip(zero, base, base._fields):
        SM.same(np.asarray(g), np.asarray(w), f"mosaic refine_iterations=0: {name}")
    got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=3, refine_iterations=2, refine_levels=2, **kw)
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, **kw)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born, 128, 1.0, seed=5)
    al = K.sequence_refine_alignment(frames, fit.model, fit.status, "homography", 2, 2)
    chain = K.mosaic_chain(al.model, fit.status, (96, 128), anchor=3)
    canvas, count = K.mosaic_composite(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", return_count=True)
    assert got.origin == chain.origin and (al.status == 1).any() and not np.array_equal(al.model, fit.model)
    for g, w, name in ((got.canvas, canvas, "canvas"), (got.count, count, "count"), (got.to_anchor, chain.to_anchor, "to_anchor"),
                       (got.model, al.model, "model"), (got.status, fit.status, "status"), (got.held, chain.held, "held"),
                       (got.dropped, chain.dropped, "dropped")):
        SM.same(np.asarray(g), np.asarray(w), f"mosaic refine_iterations=2: {name}")
    # the stabiliser
    base = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5)
    zero = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5, refine_iterations=0)
    for g, w, name in zip(zero, base, base._fields):
        SM.same(np.asarray(g), np.asarray(w), f"stabilize refine_iterations=0: {name}")
    got = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5, refine_iterations=2, refine_levels=2)
    fit = K.tracks_motion(rows.tracks, rows.visible, rows.born, "affine", 256, 1.0, 5)
    al = K.sequence_refine_alignment(frames, fit.model, fit.status, "affine", 2, 2)
    tr = K.stabilize_trajectory(al.model, fit.status, 3)
    for g, w, name in ((got.frames, K.warp_affine(frames, tr.map), "frames"), (got.correction, tr.correction, "correction"),
                       (got.model, al.model, "model"), (got.status, fit.status, "status"), (got.held, tr.held, "held")):
        SM.same(np.asarray(g), np.asarray(w), f"stabilize refine_iterations=2: {name}")
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_mosaic(frames, refine_iterations=-1, **kw)


def test_a_refined_pan_chain_is_no_further_from_the_planted_chain():
    """8 frames of 120 x 160 cut 6 px apart from one textured image, so the planted step is the translation (-6, 0) and the
    planted chain its multiples.  The largest distance of a frame corner under the chain of refined steps (L = 3, n = 5) from
    the same corner under the planted chain must not exceed that of the chain of fitted steps."""
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    T, H, W, step = 8, 120, 160, 6
    _, frames = _pan(T, H, W, step, 17)
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, 500, 4)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born)
    al = K.sequence_refine_alignment(frames, fit.model, fit.status, "homography", 3, 5)
    assert fit.status.all() and (al.status == 1).all()

    def worst(model):
        ch = K.mosaic_chain(model, None, (H, W), anchor=0)
        assert not ch.dropped.any() and not ch.held.any()
        return max(AM.corner_error(ch.from_anchor[t].reshape(9), M.translation(-step * t, 0), H, W) for t in range(T))

    fitted, refined = worst(fit.model), worst(al.model)
    print(f"pan chain of {T} frames: largest corner error {fitted:.4g} px fitted, {refined:.4g} px refined; "
          f"mean squared residual {al.stats[:, 0].mean():.4g} -> {al.stats[:, 1].mean():.4g}")
    assert refined <= fitted
