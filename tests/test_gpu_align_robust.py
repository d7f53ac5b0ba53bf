"""GPU tests of robust direct image alignment (run on an MI355X: python -m pytest tests/test_gpu_align_robust.py -m gpu -q).

The model, the status, the eight stats and the (gain, bias) of oflk_align_refine_robust, oflk_align_sequence_robust and their
host forms, and the map of oflk_align_weights, must equal the statement (tests/align_robust_model.py) byte for byte, a NaN
equal to a NaN: on a batch that mixes every kind of step, at one partial tile, exactly one tile, five tile columns with the last
one pixel wide (70 x 257: where the two-wave split of the photometric homography's 69 sums or a tail can go wrong) and three
tile rows; across the host forms' chunk boundary; from a captured graph; and with the step loops taken twice.  There is no
tolerance in this file: what the weights reach is tested on the statement (tests/test_align_robust_cpu.py) and the device
equals it.
"""
import numpy as np
import pytest

import align_model as AM
import align_photo_model as APM
import align_robust_model as ARM
import align_robust_scenes as RS
import step_loop_scenes as SC

pytestmark = pytest.mark.gpu

KINDS = [("homography", AM.HOMOGRAPHY), ("affine", AM.AFFINE)]
PHOTO = [pytest.param(False, id="plain"), pytest.param(True, id="photometric")]
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.uint8, id="u8")]
SIZES = [(33, 47), (64, 64), (70, 257), (96, 130)]
ONE = ARM.ONE.tobytes()
# mixed_steps' step 6 is rejected (status 2) everywhere but here, where the statement refines it (status 1)
NOT_REJECTED = {(70, 257, AM.HOMOGRAPHY, "uint8", True), (70, 257, AM.AFFINE, "uint8", True), (96, 130, AM.AFFINE, "float32", True)}


def _device(a, b, model, status, code, levels, iterations, delta, photometric, min_share=0.25, sequence=False):
    """the device form: outputs preset with bytes that the call must overwrite; b None with sequence.  Without photometric
    d_photo_out is NULL and the photo that comes back is the (1, 0) the host forms report"""
    import torch

    import _oflk

    d = "cuda:0"
    S = len(model)
    H, W = a.shape[1:]
    u8 = a.dtype == np.uint8
    nbytes = _oflk.align_workspace(S, H, W, levels, code, photometric, robust=True)
    assert nbytes > _oflk.align_workspace(S, H, W, levels, code, photometric)
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=d)
    t_a = torch.from_numpy(a).to(d)
    t_b = None if sequence else torch.from_numpy(b).to(d)
    t_model = torch.from_numpy(np.ascontiguousarray(model, np.float32)).to(d)
    t_status = None if status is None else torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(d)
    out = torch.full(model.shape, -7.0, dtype=torch.float32, device=d)
    st = torch.full((S,), 9, dtype=torch.int32, device=d)
    stats = torch.full((S, 8), -7.0, dtype=torch.float64, device=d)
    photo = torch.full((S, 2), -7.0, dtype=torch.float32, device=d)
    tail = (H, W, levels, iterations, code, min_share, t_model.data_ptr(), 0 if t_status is None else t_status.data_ptr(), ws.data_ptr(),
            nbytes, out.data_ptr(), st.data_ptr(), stats.data_ptr(), u8, 0, photo.data_ptr() if photometric else None, delta)
    if sequence:
        _oflk.align_sequence(t_a.data_ptr(), S + 1, *tail)
    else:
        _oflk.align_refine(t_a.data_ptr(), t_b.data_ptr(), S, *tail)
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0x5A).all().item(), "nothing is written past the workspace"
    ph = photo.cpu().numpy()
    if not photometric:
        assert (ph == -7.0).all(), "d_photo_out is not written without photometric"
        ph = np.stack([ARM.ONE] * S)
    return out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy(), ph


def _host(a, b, model, status, code, levels, iterations, delta, photometric, min_share=0.25):
    import _oflk

    return _oflk.align_robust_host(a, b, model, status, levels, iterations, code, min_share, delta, photometric)


@pytest.mark.parametrize("photometric", PHOTO)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_every_kind_of_step_equals_the_model(oracle, H, W, kind, code, dtype, photometric):
    """refined, held, thrown off the frame (frozen by min_share), refined on an overlap, frozen on a flat template, a NaN
    model, rejected, and a step with a moving object, in one call; 3 levels, 2 iterations, delta = 4"""
    a, b, model, status = RS.mixed_steps(H, W, code, H + W, dtype, photometric)
    want = ARM.refine(a, b, model, RS.DELTA, status, code, 3, 2, 0.25, photometric)
    what = f"{W}x{H} {kind} {np.dtype(dtype).name} photometric={photometric}"
    ARM.same(_device(a, b, model, status, code, 3, 2, RS.DELTA, photometric), want, what + " device")
    ARM.same(_host(a, b, model, status, code, 3, 2, RS.DELTA, photometric), want, what + " host")
    # the batch is what it is meant to be
    rejected = 1 if (H, W, code, np.dtype(dtype).name, photometric) in NOT_REJECTED else 2
    assert want[1].tolist() == [1, 0, 0, 1, 0, 0, rejected, 1]
    assert want[2][0, 3] == 6 and want[2][7, 3] == 6 and want[2][6, 3] >= 1
    assert not want[2][1].any() and not want[2][5].any() and np.isnan(want[2][2, 0]) and want[2][2, 2] == 0
    assert 0.3 < want[2][3, 2] < 0.75 and want[2][4, 3] == 0 and want[2][4, 2] > 0.5
    assert want[2][7, 7] < 0.95   # the moving object is down-weighted
    for s in range(8):
        assert (photometric and want[1][s] == 1) or want[3][s].tobytes() == ONE
    if photometric:
        g, bb = want[3][0].astype(np.float64)
        assert abs((g * 128 + bb) - (0.8 * 128 + 12)) < 0.5


@pytest.mark.parametrize("photometric", PHOTO)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_sequence_form_equals_the_pair_form_and_two_runs_agree(oracle, dtype, photometric):
    frames, _, _, _ = APM.pan_scene(6, 48, 70, 3, 11)
    frames = np.ascontiguousarray(frames.astype(dtype))
    for kind, code in KINDS:
        model = np.stack([AM.IDENTITY[code]] * 5)
        model[:, 2] = -2.5
        model[3, 2] = np.nan
        status = np.array([1, 1, 0, 1, 1], np.int32)
        want = ARM.sequence(frames, model, RS.DELTA, status, code, 2, 3, 0.25, photometric)
        assert want[1].tolist() == [1, 1, 0, 0, 1]
        ARM.same(_device(frames[:-1].copy(), frames[1:].copy(), model, status, code, 2, 3, RS.DELTA, photometric), want, f"{kind} pair form")
        seq = _device(frames, None, model, status, code, 2, 3, RS.DELTA, photometric, sequence=True)
        ARM.same(seq, want, f"{kind} sequence form")
        ARM.same(_device(frames, None, model, status, code, 2, 3, RS.DELTA, photometric, sequence=True), seq, f"{kind} second run")
        ARM.same(_host(frames, None, model, status, code, 2, 3, RS.DELTA, photometric), want, f"{kind} sequence host form")


@pytest.mark.parametrize("photometric", PHOTO)
def test_the_host_forms_over_a_chunk_boundary_equal_one_chunk(oracle, photometric):
    """the host forms go up in chunks of at most 64 steps: S = 65 at 16 x 17 is 64 + 1; every step must equal the same step
    refined alone in one chunk, which is the model's"""
    S, H, W = 65, 16, 17
    rng = np.random.default_rng(2)
    base = AM.texture(H, W + S + 2, 9, sigma=1.5, margin=0)
    frames = np.stack([(1.0 + 0.002 * t) * base[:, t:t + W] - 0.3 * t for t in range(S + 1)]).astype(np.float32)
    frames += rng.standard_normal(frames.shape).astype(np.float32)
    frames[:, 4:9, 3:8] += np.float32(40.0) * (np.arange(S + 1) % 2).astype(np.float32)[:, None, None]   # something that flickers
    model = np.stack([AM.IDENTITY[AM.AFFINE]] * S)
    model[:, 2] = -0.5
    want = ARM.sequence(frames, model, RS.DELTA, None, AM.AFFINE, 1, 2, 0.25, photometric)
    assert (want[1] == 1).sum() > S // 2 and (want[2][want[1] == 1, 7] < 1.0).all()
    ARM.same(_host(frames, None, model, None, AM.AFFINE, 1, 2, RS.DELTA, photometric), want, "sequence host form, 65 steps")
    a, b = frames[:-1].copy(), frames[1:].copy()
    ARM.same(_host(a, b, model, None, AM.AFFINE, 1, 2, RS.DELTA, photometric), want, "pair host form, 65 steps")
    for s in (0, 63, 64):
        ARM.same(_host(a[s:s + 1], b[s:s + 1], model[s:s + 1], None, AM.AFFINE, 1, 2, RS.DELTA, photometric),
                 tuple(x[s:s + 1] for x in want), f"step {s} alone")


@pytest.mark.parametrize("photometric", PHOTO)
def test_the_device_form_replays_from_a_graph_on_new_frames(oracle, photometric):
    """one chain of launches and nothing else: captured once after one eager call and replayed on new frame contents (the
    process keeps the default number of hardware queues); the outputs are scribbled over between replays"""
    import torch

    import _oflk

    d, S, H, W, L, n, code = "cuda:0", 2, 40, 70, 2, 2, AM.HOMOGRAPHY
    nbytes = _oflk.align_workspace(S, H, W, L, code, photometric, robust=True)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    t_a, t_b = torch.zeros((S, H, W), dtype=torch.float32, device=d), torch.zeros((S, H, W), dtype=torch.float32, device=d)
    model = np.stack([AM.IDENTITY[code]] * S)
    t_model = torch.from_numpy(model).to(d)
    out, st, stats = torch.empty_like(t_model), torch.empty(S, dtype=torch.int32, device=d), torch.empty((S, 8), dtype=torch.float64, device=d)
    photo = torch.empty((S, 2), dtype=torch.float32, device=d)

    def enqueue(stream):
        _oflk.align_refine(t_a.data_ptr(), t_b.data_ptr(), S, H, W, L, n, code, 0.25, t_model.data_ptr(), 0, ws.data_ptr(), nbytes,
                           out.data_ptr(), st.data_ptr(), stats.data_ptr(), False, stream, photo.data_ptr() if photometric else None,
                           RS.DELTA)

    def scene(seed):
        pairs = [RS.moving_object_pair(H, W, seed + k, code, (0.9 + 0.001 * seed, 5.0) if photometric else None)[:2] for k in range(S)]
        a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        t_a.copy_(torch.from_numpy(a))
        t_b.copy_(torch.from_numpy(b))
        return ARM.refine(a, b, model, RS.DELTA, None, code, L, n, 0.25, photometric)

    def read():
        ph = photo.cpu().numpy() if photometric else np.stack([ARM.ONE] * S)
        return out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy(), ph

    want = scene(40)
    enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ARM.same(read(), want, "eager")
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
        photo.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        ARM.same(read(), want, f"replay {rep}")
        assert (want[1] == 1).all()
    del g


def _same_map(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, f"{what}: {got.shape} {got.dtype}"
    eq = got.view(np.uint32) == want.view(np.uint32)
    assert eq.all(), f"{what}: differs at {np.argwhere(~eq)[:5].tolist()}: got {got[~eq][:5]}, want {want[~eq][:5]}"


@pytest.mark.parametrize("photometric", PHOTO)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W", [(33, 47), (70, 257)])
def test_the_weight_map_equals_the_model(oracle, H, W, kind, code, dtype, photometric):
    """oflk_align_weights, device and host form, on the mixed batch under its input models (a NaN model and one that throws b
    off the frame among them: all zeros) and, photometric, under gains and biases of its own; and the Python call"""
    import torch

    import _oflk
    import lucas_kanade_core as K

    a, b, model, _ = RS.mixed_steps(H, W, code, H + W, dtype, photometric)
    S = len(model)
    photo = np.stack([np.float32([0.8 + 0.01 * s, 12.0 - s]) for s in range(S)]) if photometric else None
    want = np.stack([ARM.weights(a[s], b[s], model[s], code, RS.DELTA, *(photo[s] if photometric else ())) for s in range(S)])
    assert not want[2].any() and not want[5].any() and 0.0 < want[7].mean() < 1.0 and want.max() == 1.0
    what = f"{W}x{H} {kind} {np.dtype(dtype).name} photometric={photometric}"
    _same_map(_oflk.align_weights_host(a, b, model, code, RS.DELTA, photo), want, what + " host")
    d = "cuda:0"
    t_a, t_b, t_m = torch.from_numpy(a).to(d), torch.from_numpy(b).to(d), torch.from_numpy(model).to(d)
    t_p = torch.from_numpy(photo).to(d) if photometric else None
    out = torch.full((S * H * W + 64,), -7.0, dtype=torch.float32, device=d)
    _oflk.align_weights(t_a.data_ptr(), t_b.data_ptr(), S, H, W, code, RS.DELTA, t_m.data_ptr(), t_p.data_ptr() if photometric else 0,
                        out.data_ptr(), dtype == np.uint8)
    torch.cuda.synchronize()
    assert (out[S * H * W:] == -7.0).all().item(), "nothing is written past the map"
    _same_map(out[:S * H * W].cpu().numpy().reshape(S, H, W), want, what + " device")
    shape = (3, 3) if code == AM.HOMOGRAPHY else (2, 3)
    gb = dict(gain=photo[:, 0], bias=photo[:, 1]) if photometric else {}
    _same_map(K.alignment_weights(a, b, model.reshape(S, *shape), kind, RS.DELTA, **gb), want, what + " python")
    one = K.alignment_weights(a[7], b[7], model[7].reshape(shape), kind, RS.DELTA, **({k: v[7] for k, v in gb.items()}))
    _same_map(one, want[7:8], what + " python, one frame")


def test_robust_delta_none_is_the_existing_call(oracle):
    """None returns today's types with today's bytes (the statements that the existing GPU tests hold those calls to); a number
    returns a RobustAlignment that equals the robust statement"""
    import lucas_kanade_core as K

    A, B, planted = RS.moving_object_pair(64, 64, 3, AM.HOMOGRAPHY, (0.8, 12.0))
    m0 = AM.pushed(planted, 64, 64, AM.HOMOGRAPHY)
    want = AM.refine(A[None], B[None], m0[None], None, AM.HOMOGRAPHY, 3, 5)
    for one in (K.refine_alignment(A, B, m0.reshape(3, 3)), K.refine_alignment(A, B, m0.reshape(3, 3), robust_delta=None)):
        assert type(one) is K.Alignment
        AM.same((one.model.reshape(1, 9), np.array([one.status], np.int32), one.stats[None]), want, "robust_delta=None")
    ph = K.refine_alignment(A, B, m0.reshape(3, 3), photometric=True, robust_delta=None)
    assert type(ph) is K.PhotometricAlignment
    APM.same((ph.model.reshape(1, 9), np.array([ph.status], np.int32), ph.stats[None], np.array([[ph.gain, ph.bias]], np.float32)),
             APM.refine(A[None], B[None], m0[None], None, AM.HOMOGRAPHY, 3, 5), "photometric, robust_delta=None")
    frames = np.stack([A, B, A])
    models = np.stack([m0, AM.IDENTITY[AM.HOMOGRAPHY]]).reshape(2, 3, 3)
    seq = K.sequence_refine_alignment(frames, models, [1, 0], levels=2, iterations=2, robust_delta=None)
    assert type(seq) is K.Alignment
    AM.same((seq.model.reshape(2, 9), seq.status, seq.stats), AM.sequence(frames, models, [1, 0], AM.HOMOGRAPHY, 2, 2), "sequence")
    for photometric in (False, True):
        got = K.refine_alignment(A, B, m0.reshape(3, 3), photometric=photometric, robust_delta=RS.DELTA)
        assert type(got) is K.RobustAlignment and got.model.shape == (3, 3) and got.stats.shape == (8,) and got.gain.shape == ()
        ARM.same((got.model.reshape(1, 9), np.array([got.status], np.int32), got.stats[None], np.array([[got.gain, got.bias]], np.float32)),
                 ARM.refine(A[None], B[None], m0[None], RS.DELTA, None, AM.HOMOGRAPHY, 3, 5, 0.25, photometric), f"robust, photometric={photometric}")
        sq = K.sequence_refine_alignment(frames, models, [1, 0], levels=2, iterations=2, photometric=photometric, robust_delta=RS.DELTA)
        assert type(sq) is K.RobustAlignment and sq.stats.shape == (2, 8)
        ARM.same((sq.model.reshape(2, 9), sq.status, sq.stats, np.stack([sq.gain, sq.bias], 1)),
                 ARM.sequence(frames, models, RS.DELTA, [1, 0], AM.HOMOGRAPHY, 2, 2, 0.25, photometric), f"robust sequence, photometric={photometric}")


@pytest.mark.parametrize("photometric", PHOTO)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,code", KINDS)
def test_a_delta_above_every_residual_gives_the_base_calls_model_and_status(oracle, kind, code, dtype, photometric):
    """robust_delta = 3.0e38 against the plain / photometric GPU call on the mixed batch at 70 x 257: the model and status (and
    photo) bytes are equal, the squared-residual stats are the base call's stats"""
    import _oflk

    a, b, model, status = RS.mixed_steps(70, 257, code, 70 + 257, dtype, photometric)
    got = _host(a, b, model, status, code, 3, 2, RS.NO_DELTA, photometric)
    base = _oflk.align_host(a, b, model, status, 3, 2, code, 0.25, *([True] if photometric else []))
    what = f"{kind} {np.dtype(dtype).name} photometric={photometric}"
    AM.same((got[0], got[1], np.ascontiguousarray(got[2][:, [4, 5, 2, 3]])), base[:3], what)
    if photometric:
        assert got[3].tobytes() == base[3].tobytes()
    live = ~np.isnan(got[2][:, 0]) & (got[2][:, 2] > 0)
    assert (got[2][live][:, 6:8] == 1.0).all() and (got[2][live][:, 0:2] == 0.5 * got[2][live][:, 4:6]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the step loops past the 65 535-block grid (tests/step_loop_scenes.py)
# ---------------------------------------------------------------------------------------------------------------------
def _loop_model(code, photometric, form, levels, iterations, dtype):
    """step_loop_scenes.align_model for the robust statement: the seven kinds"""
    if form == "pair":
        a, b, model, status = SC.align_pairs(code, photometric)
        return ARM.refine(a, b, model, RS.DELTA, status, code, levels, iterations, 0.25, photometric)
    frames, model, status = SC.align_frames(code, photometric, dtype)
    return ARM.sequence(frames, model, RS.DELTA, status, code, levels, iterations, 0.25, photometric)


# one pair and one sequence form for each of the four reduce kernels (plain / photometric x affine / homography)
LOOPS = [("pair", 2, 2, np.float32, "homography", AM.HOMOGRAPHY, True), ("sequence", 2, 2, np.float32, "affine", AM.AFFINE, False),
         ("pair", 1, 1, np.float32, "homography", AM.HOMOGRAPHY, False), ("sequence", 1, 1, np.uint8, "affine", AM.AFFINE, True)]


@pytest.mark.parametrize("form,levels,iterations,dtype,kind,code,photometric", LOOPS,
                         ids=["pair f32 L2 homography photometric", "sequence f32 L2 affine plain", "pair f32 L1 homography plain",
                              "sequence u8 L1 affine photometric"])
def test_robust_alignment_past_the_grid_limit(oracle, form, levels, iterations, dtype, kind, code, photometric):
    """S = 65 549 steps of 16 x 24: the steps do not depend on their index, so the whole batch is the statement on the seven
    kinds, tiled; and the first 14 steps equal a call of 14"""
    want = tuple(SC.tiled(x) for x in _loop_model(code, photometric, form, levels, iterations, dtype))
    assert {0, 1} <= set(want[1][:SC.P].tolist())
    what = f"{kind} {form} form, {np.dtype(dtype).name}, L={levels} n={iterations} photometric={photometric}"
    if form == "pair":
        a, b, model, status = (SC.tiled(x) for x in SC.align_pairs(code, photometric))
        seq = False
    else:
        frames, model, status = SC.align_frames(code, photometric, dtype)
        a, b, model, status, seq = SC.tiled(frames[:SC.P], SC.S + 1), None, SC.tiled(model), SC.tiled(status), True
    got = _device(a, b, model, status, code, levels, iterations, RS.DELTA, photometric, sequence=seq)
    ARM.same(got, want, f"{what}: {SC.S} steps against the statement")
    n = 2 * SC.P
    few = _device(a[:n + seq], None if seq else b[:n], model[:n], status[:n], code, levels, iterations, RS.DELTA, photometric, sequence=seq)
    ARM.same(tuple(x[:n] for x in got), few, f"{what}: the first {n} of {SC.S} steps against a call of {n}")


@pytest.mark.parametrize("photometric", PHOTO)
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W,levels", SC.FLOOR)
def test_the_floor_of_the_alignments_sizes(oracle, H, W, levels, kind, code, photometric):
    """8 x 8 per level is the least the calls accept: the smallest frame, a coarsest level of exactly 8 x 8, and one tile row
    with a second tile column of one pixel; device and host form succeed and equal the statement"""
    for dtype in (np.float32, np.uint8):
        a, b, model = SC.floor_steps(H, W, code, photometric, dtype)
        want = ARM.refine(a, b, model, RS.DELTA, None, code, levels, SC.FLOOR_ITERATIONS, 0.25, photometric)
        what = f"{W}x{H} {kind} {np.dtype(dtype).name} L={levels} photometric={photometric}"
        ARM.same(_device(a, b, model, None, code, levels, SC.FLOOR_ITERATIONS, RS.DELTA, photometric), want, what + " device")
        ARM.same(_host(a, b, model, None, code, levels, SC.FLOOR_ITERATIONS, RS.DELTA, photometric), want, what + " host")


# ---------------------------------------------------------------------------------------------------------------------
# the Python wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_refine_robust_delta_is_the_chain_of_the_public_parts():
    """the 8-frame 96 x 128 pan through the tracker: the mosaic (plain and photometric) and the two stabilisers with
    refine_robust_delta equal the chain made of their public parts.  max_residual=16 as in tests/test_gpu_mosaic_exposure.py"""
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P
    import stabilize_model as SM

    frames, _, _, _ = APM.pan_scene()
    anchor = 3
    kw = dict(max_corners=300, detect_every=4, max_residual=16.0)
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, **kw)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born, 128, 1.0, seed=5)
    for photometric in (False, True):
        got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=anchor, refine_iterations=2, refine_levels=2,
                                                       refine_photometric=photometric, refine_robust_delta=RS.DELTA, **kw)
        al = K.sequence_refine_alignment(frames, fit.model, fit.status, "homography", 2, 2, photometric=photometric, robust_delta=RS.DELTA)
        assert type(al) is K.RobustAlignment and fit.status.all() and (al.status == 1).any()
        chain = K.mosaic_chain(al.model, fit.status, (96, 128), anchor=anchor)
        ex = K.exposure_chain(al.gain, al.bias, al.status == 1, anchor=anchor) if photometric else None
        canvas, count = K.mosaic_composite(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", True,
                                           exposure=ex)
        assert type(got) is (P.PhotometricMosaic if photometric else P.Mosaic) and got.origin == chain.origin
        pairs = [(got.canvas, canvas, "canvas"), (got.count, count, "count"), (got.to_anchor, chain.to_anchor, "to_anchor"),
                 (got.model, al.model, "model"), (got.status, fit.status, "status"), (got.held, chain.held, "held"),
                 (got.dropped, chain.dropped, "dropped")] + ([(got.exposure, ex, "exposure")] if photometric else [])
        for g, w, name in pairs:
            SM.same(np.asarray(g), np.asarray(w), f"mosaic refine_robust_delta, photometric={photometric}: {name}")
    fa = K.tracks_motion(rows.tracks, rows.visible, rows.born, "affine", 256, 1.0, 5)
    aa = K.sequence_refine_alignment(frames, fa.model, fa.status, "affine", 2, 2, robust_delta=RS.DELTA)
    tr = K.stabilize_trajectory(aa.model, fa.status, 3)
    st = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5, max_residual=16.0,
                                                     refine_iterations=2, refine_levels=2, refine_robust_delta=RS.DELTA)
    for g, w, name in ((st.frames, K.warp_affine(frames, tr.map), "frames"), (st.correction, tr.correction, "correction"),
                       (st.model, aa.model, "model"), (st.status, fa.status, "status"), (st.held, tr.held, "held")):
        SM.same(np.asarray(g), np.asarray(w), f"stabilize refine_robust_delta: {name}")
    nv12 = P.nv12_from_planes(frames, np.full((8, 48, 64, 2), 128, np.uint8))
    sn = P.lucas_kanade_pyramidal_sequence_stabilize_nv12(nv12, 300, 4, model="affine", radius=3, seed=5, max_residual=16.0,
                                                          refine_iterations=2, refine_levels=2, refine_robust_delta=RS.DELTA)
    for g, w, name in ((sn.frames, P.warp_affine_nv12(nv12, tr.map), "frames"), (sn.correction, tr.correction, "correction"),
                       (sn.model, aa.model, "model"), (sn.status, fa.status, "status"), (sn.held, tr.held, "held")):
        SM.same(np.asarray(g), np.asarray(w), f"stabilize_nv12 refine_robust_delta: {name}")
