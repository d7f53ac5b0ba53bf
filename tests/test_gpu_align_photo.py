"""GPU tests of direct image alignment with a photometric gain and bias (run on an MI355X:
python -m pytest tests/test_gpu_align_photo.py -m gpu -q).

The model, the status, the stats and the (gain, bias) of oflk_align_refine_photo, oflk_align_sequence_photo and their host
forms must equal the statement (tests/align_photo_model.py) byte for byte, a NaN equal to a NaN, on the mixed call of
tests/test_gpu_align.py with the planted steps re-exposed, at its sizes: one partial tile, exactly one tile, a one-column tile
and a six-row tile (70 x 257: where the two-wave split of the homography sums or a tail can go wrong), several tile rows.  The
only tolerances are the recovery test's: they hold for the statement (tests/test_align_photo_cpu.py)
and the device equals it.
"""
import numpy as np
import pytest

import align_model as AM
import align_photo_model as APM

pytestmark = pytest.mark.gpu

KINDS = [("homography", AM.HOMOGRAPHY), ("affine", AM.AFFINE)]
SIZES = [(33, 47), (64, 64), (70, 257), (96, 130)]
ONE = np.array([1.0, 0.0], np.float32).tobytes()


def _mixed_steps(H, W, kind, seed, dtype):
    """test_gpu_align's S = 5 steps of every sort with b's planted steps re-exposed (gain 0.8, bias +12).  uint8: the source
    is compressed to 40 + 0.5 v first, so that nothing clips
    0  equal frames under the identity, b re-exposed   1  a held step (status 0) of a planted pair
    2  a model that throws b off the frame             3  a planted pair seen through a shift of a third of the frame
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
    if dtype == np.uint8:
        a, b = np.float32(40.0) + np.float32(0.5) * a, np.float32(40.0) + np.float32(0.5) * b
    b = APM.exposed(b, 0.8, 12.0)
    if dtype == np.uint8:
        assert b.min() >= 0.5 and b.max() <= 254.5 and a.max() <= 254.5
        a, b = np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8)
    model = np.stack([ident, AM.pushed(planted, H, W, kind, 0.5), off, shifted, ident])
    return np.ascontiguousarray(a), np.ascontiguousarray(b), model, np.array([1, 0, 1, 1, 1], np.int32)


def _device(a, b, model, status, code, levels, iterations, min_share=0.25, sequence=False):
    """the device form: outputs preset with bytes that the call must overwrite; b None with sequence"""
    import torch

    import _oflk

    d = "cuda:0"
    S = len(model)
    H, W = a.shape[1:]
    u8 = a.dtype == np.uint8
    nbytes = _oflk.align_workspace(S, H, W, levels, code, photometric=True)
    assert nbytes > _oflk.align_workspace(S, H, W, levels, code)
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=d)
    t_a = torch.from_numpy(a).to(d)
    t_b = None if sequence else torch.from_numpy(b).to(d)
    t_model = torch.from_numpy(np.ascontiguousarray(model, np.float32)).to(d)
    t_status = None if status is None else torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(d)
    out = torch.full(model.shape, -7.0, dtype=torch.float32, device=d)
    st = torch.full((S,), 9, dtype=torch.int32, device=d)
    stats = torch.full((S, 4), -7.0, dtype=torch.float64, device=d)
    photo = torch.full((S, 2), -7.0, dtype=torch.float32, device=d)
    tail = (H, W, levels, iterations, code, min_share, t_model.data_ptr(), 0 if t_status is None else t_status.data_ptr(), ws.data_ptr(),
            nbytes, out.data_ptr(), st.data_ptr(), stats.data_ptr(), u8, 0, photo.data_ptr())
    if sequence:
        _oflk.align_sequence(t_a.data_ptr(), S + 1, *tail)
    else:
        _oflk.align_refine(t_a.data_ptr(), t_b.data_ptr(), S, *tail)
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0x5A).all().item(), "nothing is written past the workspace"
    return out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy(), photo.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_every_kind_of_step_equals_the_model(oracle, H, W, kind, code, dtype):
    import _oflk

    a, b, model, status = _mixed_steps(H, W, code, H + W, dtype)
    for levels, iterations in ((1, 1), (3, 4)):
        want = APM.refine(a, b, model, status, code, levels, iterations)
        what = f"{W}x{H} {kind} {np.dtype(dtype).name} L={levels} n={iterations}"
        APM.same(_device(a, b, model, status, code, levels, iterations), want, what + " device")
        APM.same(_oflk.align_host(a, b, model, status, levels, iterations, code, 0.25, True), want, what + " host")
        assert want[1][0] == 1 and want[2][0, 3] == levels * iterations
        assert want[1][1] == 0 and want[1][2] == 0 and want[1][4] == 0 and not want[2][1].any() and np.isnan(want[2][2, 0])
        assert want[1][3] != 0 and 0.3 < want[2][3, 2] < 0.75   # the shifted step is refined on the overlap alone
        for s in range(5):
            assert want[1][s] == 1 or want[3][s].tobytes() == ONE
        # step 0 is the exposure alone: the model stays near the identity and the exposure map is the planted one
        g, bb = want[3][0].astype(np.float64)
        assert abs((g * 128 + bb) - (0.8 * 128 + 12)) < 0.5 and AM.corner_error(want[0][0], AM.IDENTITY[AM.HOMOGRAPHY], H, W) < 0.05


PAIRS = [(70, 257), (96, 130)]
EXPOSURES = [(0.7, 20.0), (1.3, -15.0), (1.0, 0.0)]


@pytest.mark.parametrize("kind,code", KINDS)
@pytest.mark.parametrize("H,W", PAIRS)
def test_a_planted_map_is_recovered_under_a_planted_exposure(oracle, H, W, kind, code):
    """the GPU call on the planted pairs: corner error below 0.05 px, below a tenth of the plain call's on the same frames for
    the two changed exposures, and the exposure map g v + b at v = 128 within 0.5 grey levels"""
    import lucas_kanade_core as K

    A, B, planted = AM.planted_pair(H, W, 5, code)
    m0 = AM.pushed(planted, H, W, code)
    shape = (3, 3) if code == AM.HOMOGRAPHY else (2, 3)
    b = np.stack([APM.exposed(B, g, o) for g, o in EXPOSURES])
    a = np.stack([A] * 3)
    m = np.stack([m0.reshape(shape)] * 3)
    got = K.refine_alignment(a, b, m, None, kind, 3, 4, photometric=True)
    plain = K.refine_alignment(a, b, m, None, kind, 3, 4)
    assert isinstance(got, K.PhotometricAlignment) and isinstance(plain, K.Alignment)
    for k, (gain, bias) in enumerate(EXPOSURES):
        err = AM.corner_error(got.model[k].reshape(-1), planted, H, W)
        perr = AM.corner_error(plain.model[k].reshape(-1), planted, H, W)
        level = abs((float(got.gain[k]) * 128.0 + float(got.bias[k])) - (gain * 128.0 + bias))
        print(f"{W}x{H} {kind} gain {gain} bias {bias}: corner error {err:.4f} px (plain call {perr:.4f}, status {plain.status[k]}), "
              f"|g 128 + b - planted| {level:.4f}, residual {got.stats[k, 0]:.4g} -> {got.stats[k, 1]:.4g}")
        assert got.status[k] == 1 and err < 0.05 and level < 0.5
        if (gain, bias) != (1.0, 0.0):
            assert err < perr / 10.0


@pytest.mark.parametrize("kind,code", KINDS)
def test_a_gain_that_would_not_be_positive_freezes_the_step(oracle, kind, code):
    """B = 255 - A: the first update would make g' = -1 (tests/test_align_photo_cpu.py shows it on the statement)"""
    A, _, _ = AM.planted_pair(70, 257, 5, code)
    B = (np.float32(255.0) - A).astype(np.float32)
    ident = AM.IDENTITY[code][None]
    want = APM.refine(A[None], B[None], ident, None, code, 1, 1)
    assert want[1][0] == 0 and want[2][0, 3] == 0 and want[3][0].tobytes() == ONE
    APM.same(_device(A[None], B[None], ident, None, code, 1, 1), want, f"negative gain {kind}")


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_the_sequence_form_equals_the_pair_form_and_two_runs_agree(oracle, dtype):
    import _oflk

    frames, _, _, _ = APM.pan_scene(6, 48, 70, 3, 11)
    frames = np.ascontiguousarray(frames.astype(dtype))
    for kind, code in KINDS:
        model = np.stack([AM.IDENTITY[code]] * 5)
        model[:, 2] = -2.5
        model[3, 2] = np.nan
        status = np.array([1, 1, 0, 1, 1], np.int32)
        want = APM.sequence(frames, model, status, code, 2, 3)
        assert want[1].tolist() == [1, 1, 0, 0, 1]
        APM.same(_device(frames[:-1].copy(), frames[1:].copy(), model, status, code, 2, 3), want, f"{kind} pair form")
        seq = _device(frames, None, model, status, code, 2, 3, sequence=True)
        APM.same(seq, want, f"{kind} sequence form")
        APM.same(_device(frames, None, model, status, code, 2, 3, sequence=True), seq, f"{kind} second run")
        APM.same(_oflk.align_host(frames, None, model, status, 2, 3, code, 0.25, True), want, f"{kind} sequence host form")


def test_the_device_form_replays_from_a_graph_on_new_frames(oracle):
    """one chain of launches and nothing else: captured once after one eager call and replayed on new frame contents (the
    process keeps the default number of hardware queues); the outputs are scribbled over between replays"""
    import torch

    import _oflk

    d, S, H, W, L, n, code = "cuda:0", 2, 40, 70, 2, 2, AM.HOMOGRAPHY
    nbytes = _oflk.align_workspace(S, H, W, L, code, photometric=True)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    t_a, t_b = torch.zeros((S, H, W), dtype=torch.float32, device=d), torch.zeros((S, H, W), dtype=torch.float32, device=d)
    model = np.stack([AM.IDENTITY[code]] * S)
    t_model = torch.from_numpy(model).to(d)
    out, st, stats = torch.empty_like(t_model), torch.empty(S, dtype=torch.int32, device=d), torch.empty((S, 4), dtype=torch.float64, device=d)
    photo = torch.empty((S, 2), dtype=torch.float32, device=d)

    def enqueue(stream):
        _oflk.align_refine(t_a.data_ptr(), t_b.data_ptr(), S, H, W, L, n, code, 0.25, t_model.data_ptr(), 0, ws.data_ptr(), nbytes,
                           out.data_ptr(), st.data_ptr(), stats.data_ptr(), False, stream, photo.data_ptr())

    def scene(seed):
        pairs = [AM.planted_pair(H, W, seed + k, code, move=1.0)[:2] for k in range(S)]
        a, b = np.stack([p[0] for p in pairs]), np.stack([APM.exposed(p[1], 0.9 + 0.001 * seed, 5.0) for p in pairs])
        t_a.copy_(torch.from_numpy(a))
        t_b.copy_(torch.from_numpy(b))
        return APM.refine(a, b, model, None, code, L, n)

    def read():
        return out.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy(), photo.cpu().numpy()

    want = scene(40)
    enqueue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    APM.same(read(), want, "eager")
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
        APM.same(read(), want, f"replay {rep}")
        assert (want[1] == 1).all()
    del g


def test_the_host_forms_over_a_chunk_boundary_equal_one_chunk(oracle):
    """the host forms go up in chunks of at most 64 steps: S = 65 at 33 x 47 is 64 + 1; every step must equal the same step
    refined alone in one chunk, which is the model's"""
    import _oflk

    S, H, W = 65, 33, 47
    rng = np.random.default_rng(2)
    base = AM.texture(H, W + S + 2, 9, sigma=1.5, margin=0)
    frames = np.stack([(1.0 + 0.002 * t) * base[:, t:t + W] - 0.3 * t for t in range(S + 1)]).astype(np.float32)
    frames += rng.standard_normal(frames.shape).astype(np.float32)
    model = np.stack([AM.IDENTITY[AM.AFFINE]] * S)
    model[:, 2] = -0.5
    want = APM.sequence(frames, model, None, AM.AFFINE, 1, 2)
    assert (want[1] == 1).sum() > S // 2
    APM.same(_oflk.align_host(frames, None, model, None, 1, 2, AM.AFFINE, 0.25, True), want, "sequence host form, 65 steps")
    a, b = frames[:-1].copy(), frames[1:].copy()
    APM.same(_oflk.align_host(a, b, model, None, 1, 2, AM.AFFINE, 0.25, True), want, "pair host form, 65 steps")
    for s in (0, 63, 64):
        APM.same(_oflk.align_host(a[s:s + 1], b[s:s + 1], model[s:s + 1], None, 1, 2, AM.AFFINE, 0.25, True),
                 tuple(x[s:s + 1] for x in want), f"step {s} alone")


def test_photometric_false_is_the_plain_call(oracle):
    import lucas_kanade_core as K

    A, B, planted = AM.planted_pair(64, 64, 3, AM.HOMOGRAPHY)
    m0 = AM.pushed(planted, 64, 64, AM.HOMOGRAPHY)
    Be = APM.exposed(B, 0.8, 12.0)
    want = AM.refine(A[None], Be[None], m0[None], None, AM.HOMOGRAPHY, 3, 5)
    for one in (K.refine_alignment(A, Be, m0.reshape(3, 3)), K.refine_alignment(A, Be, m0.reshape(3, 3), photometric=False)):
        assert type(one) is K.Alignment
        AM.same((one.model.reshape(1, 9), np.array([one.status], np.int32), one.stats[None]), want, "photometric=False")
    frames = np.stack([A, Be, A])
    models = np.stack([m0, AM.IDENTITY[AM.HOMOGRAPHY]]).reshape(2, 3, 3)
    seq = K.sequence_refine_alignment(frames, models, [1, 0], levels=2, iterations=2, photometric=False)
    assert type(seq) is K.Alignment
    AM.same((seq.model.reshape(2, 9), seq.status, seq.stats), AM.sequence(frames, models, [1, 0], AM.HOMOGRAPHY, 2, 2), "sequence")
    # and with it: the statement, one step unbatched
    got = K.refine_alignment(A, Be, m0.reshape(3, 3), photometric=True)
    assert type(got) is K.PhotometricAlignment and got.model.shape == (3, 3) and got.gain.shape == () and got.bias.shape == ()
    pw = APM.refine(A[None], Be[None], m0[None], None, AM.HOMOGRAPHY, 3, 5)
    APM.same((got.model.reshape(1, 9), np.array([got.status], np.int32), got.stats[None], np.array([[got.gain, got.bias]], np.float32)),
             pw, "photometric=True, one step")
    sq = K.sequence_refine_alignment(frames, models, [1, 0], levels=2, iterations=2, photometric=True)
    APM.same((sq.model.reshape(2, 9), sq.status, sq.stats, np.stack([sq.gain, sq.bias], 1)),
             APM.sequence(frames, models, [1, 0], AM.HOMOGRAPHY, 2, 2), "photometric sequence")
