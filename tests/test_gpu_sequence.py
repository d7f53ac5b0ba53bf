"""GPU tests of the frame-sequence entry points (run on an MI355X: python -m pytest tests/test_gpu_sequence.py -m gpu -q).

A sequence of T frames is the batch of the T-1 pairs (f[t], f[t+1]) whose pyramids are built once per frame.  Every result
-- flow, residual log, iteration counts, uncertain flags, coarser levels' flows, flagged pairs resolved -- must equal the
pair batch's bit for bit, in every arithmetic mode, for float32 and uint8 frames, on the vector and the element-wise
kernels, the unfused pyramid chain and the per-pair generic windows; and the pyramid stage must cost about half.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_exit_band import ARITH, THR, _reference
from test_tolerant_model import device_mean_error, level_sum_path, numpy_mean_error

pytestmark = pytest.mark.gpu

f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int)


def _video(T, H, W, seed=0, u8=False):
    """T frames of a textured scene drifting by a sub-pixel step per frame, with a little per-frame noise (float32 values
    in [0, 255]; uint8 when asked)"""
    from scipy.ndimage import shift

    from oflk_synth import synth_pair

    rng = np.random.default_rng(1000 + seed)
    base = synth_pair(H, W, pair_index=seed)[0].astype(np.float64)
    out = np.empty((T, H, W), np.float32)
    for t in range(T):
        f = shift(base, (-0.4 * t, 0.7 * t), order=1, mode="nearest") + rng.normal(0.0, 1.5, (H, W))
        out[t] = np.clip(f, 0, 255)
    return np.rint(out).astype(np.uint8) if u8 else out


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _read(plan, d_u, d_v, st):
    import torch

    log, runs = plan.read_log(st)
    flags = plan.read_uncertain(st)
    torch.cuda.synchronize()
    return d_u.cpu().numpy(), d_v.cpu().numpy(), log, runs, flags


def _pair_and_sequence(frames, L, window, K, mode, u8):
    """the same plan run on the pair batch (separate copies of f[:-1] and f[1:]) and on the sequence: both results, and
    both sets of coarser-level flows of the first and the last pair"""
    import torch

    import _oflk

    T, H, W = frames.shape
    B = T - 1
    st = torch.cuda.current_stream().cuda_stream
    d_f = _dev(frames)
    d_p, d_c = _dev(frames[:-1].copy()), _dev(frames[1:].copy())
    d_u = torch.empty((B, H, W), dtype=torch.float32, device=d_f.device)
    d_v = torch.empty_like(d_u)
    plan = _oflk.Plan(0, B, H, W, L, window, K)
    try:
        plan.set_arithmetic(ARITH[mode])
        res = []
        for seq in (False, True):
            d_u.fill_(np.nan)
            d_v.fill_(np.nan)
            if seq:
                plan.pyramidal_sequence(d_f.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st, u8=u8)
            else:
                (plan.pyramidal_u8 if u8 else plan.pyramidal)(d_p.data_ptr(), d_c.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
            r = _read(plan, d_u, d_v, st)
            dims = _oflk_dims(H, W, L)
            lv = [plan.read_level_flow(l, b, dims[l], st) for l in range(L - 1) for b in (0, B - 1)]
            res.append((r, lv))
        return res
    finally:
        plan.close()


def _oflk_dims(H, W, L):
    import lucas_kanade_pyramidal as P

    return P.pyramid_level_shapes((H, W), L)


def _assert_same(a, b, what):
    (ra, lva), (rb, lvb) = a, b
    for name, x, y in zip(("u", "v", "log", "iters_run", "uncertain"), ra, rb):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {name} differs"
    for (xu, xv), (yu, yv) in zip(lva, lvb):
        assert np.array_equal(xu.view(np.uint8), yu.view(np.uint8)) and np.array_equal(xv.view(np.uint8), yv.view(np.uint8)), \
            f"{what}: a coarser level's flow differs"


# ---------------------------------------------------------------------------------------------------------------
# 1. the sequence pass equals the pair pass, bit for bit
# ---------------------------------------------------------------------------------------------------------------
CASES = (
    # (H, W, L, K, window, T values, modes)
    # 240 x 320: 16-byte aligned planes, the vector kernels
    (240, 320, 3, 3, 5, (2, 3, 9, 33), ("exact", "contracted", "tolerant")),
    (240, 320, 3, 3, 3, (9,), ("exact", "tolerant")),
    (240, 320, 3, 3, 7, (9,), ("exact", "tolerant")),
    (240, 320, 2, 3, 5, (9,), ("tolerant",)),            # outside the tolerant envelope: runs exactly
    (240, 320, 3, 2, 5, (9,), ("tolerant",)),            # envelope cell (3, 2)
    # 37 x 53: an odd plane, so curr is misaligned (uint8: 1-byte aligned) -- the element-wise instantiations
    (37, 53, 3, 3, 5, (2, 3, 9, 33), ("exact", "contracted", "tolerant")),
    (37, 53, 3, 3, 7, (9,), ("exact",)),
    (241, 321, 4, 3, 5, (3, 9), ("exact", "contracted", "tolerant")),
    # tiny levels: the unfused pyramid chain (uint8: the float32 staging of the frames)
    (23, 21, 3, 3, 5, (2, 9), ("exact", "tolerant")),
    (6, 9, 2, 2, 5, (2, 5), ("exact",)),
    # 13 x 13: no fused iteration kernel, the pairs run one by one through the exact path
    (120, 160, 3, 3, 13, (2, 4), ("exact", "tolerant")),
    (37, 53, 2, 2, 13, (3,), ("exact",)),
)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-L{c[2]}K{c[3]}-w{c[4]}")
def test_sequence_equals_pair_batch(case, u8):
    H, W, L, K, window, Ts, modes = case
    for T in Ts:
        frames = _video(T, H, W, seed=T + H, u8=u8)
        for mode in modes:
            pair, seq = _pair_and_sequence(frames, L, window, K, mode, u8)
            _assert_same(pair, seq, f"{H}x{W} L{L} K{K} w{window} T={T} {mode} {'u8' if u8 else 'f32'}")
            assert (seq[0][3] >= 1).all()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,T", [((1081, 1923), 3), ((1080, 1920), 5)])
def test_sequence_equals_pair_batch_large(shape, T, u8):
    H, W = shape
    frames = _video(T, H, W, seed=7, u8=u8)
    for mode in ("exact", "tolerant"):
        pair, seq = _pair_and_sequence(frames, 3, 5, 3, mode, u8)
        _assert_same(pair, seq, f"{H}x{W} T={T} {mode} {'u8' if u8 else 'f32'}")


# ---------------------------------------------------------------------------------------------------------------
# 2. against the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_pattern_sequence_equals_oracle(oracle, golden_dir, u8):
    """frame_0 followed by the 13 patterns' second frames: every flow (and its iteration counts) is the oracle's on that pair"""
    import lucas_kanade_pyramidal as P

    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    assert len(names) == 13
    frames = np.stack([z["frame_0"]] + [z[f"frame_1__{n}"] for n in names])
    frames = frames.astype(np.uint8) if u8 else frames.astype(np.float32)
    u, v, log, runs = P.lucas_kanade_pyramidal_sequence_with_log(frames, 3, 5, 3)
    assert u.shape == v.shape == (13, 240, 320) and runs.shape == (13, 3) and log.shape == (13, 3, 3, 2)
    for t in range(13):
        ou, ov, olog, oruns = oracle.lucas_kanade_pyramidal_ex(frames[t].astype(np.float32), frames[t + 1].astype(np.float32), 3, 5, 3)
        assert list(runs[t]) == list(oruns), (t, runs[t], oruns)
        assert np.array_equal(u[t], ou) and np.array_equal(v[t], ov), f"pair {t} differs from the oracle"


# ---------------------------------------------------------------------------------------------------------------
# 3. a flagged exit decision inside a sequence, resolved through the aliased pointers
# ---------------------------------------------------------------------------------------------------------------
def test_flagged_inner_pair_resolves_with_aliased_pointers(oracle):
    """frames [A, prev, curr, Z]: the first decision of pair 1 (prev -> curr) is bisected to an exact mean just inside the
    band (as in test_gpu_exit_band).  The sequence pass flags pair 1 only; oflk_plan_resolve_uncertain(d_frames,
    d_frames + H*W) redoes it to the oracle's flow and counts and leaves pairs 0 and 2 as they were."""
    import torch

    import _oflk
    from oflk_synth import synth_pair

    H, W, L, K, mode = 48, 64, 2, 2, "exact"
    h, w = oracle.pyramid_dims(H, W, L)[0]
    path = level_sum_path(ARITH[mode], L, K, 5, oracle.pyramid_dims(H, W, L), 0)
    S = numpy_mean_error(h * w) + device_mean_error(path, h, w, THR)
    st = torch.cuda.current_stream().cuda_stream

    def place(seed, off):
        prev, shifted = synth_pair(H, W, seed, dx=0.75, dy=-0.5)
        delta = (shifted - prev).astype(np.float64)
        frames = lambda t: (prev + t * delta).astype(np.float32)  # noqa: E731
        mean = lambda t: float(max(_reference(oracle, mode, prev, frames(t), L, K, 5)[4][0, 0]))  # noqa: E731
        target = THR * (1.0 + off)
        lo, hi = 0.0, 1.0
        assert mean(lo) < target < mean(hi)
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean(mid) < target else (lo, mid)
        t = min((lo, hi), key=lambda e: abs(mean(e) - target))
        return prev, frames(t), mean(t) / THR - 1.0

    tried = []
    for seed in range(16):
        prev, curr, rel = place(seed, 0.5 * S)
        tried.append(rel)
        if 0.0 < rel < S:
            break
    assert 0.0 < tried[-1] < S, f"no pair landed inside the band: {tried}"
    A = synth_pair(H, W, 90, dx=1.0, dy=0.5)[0]
    Z = synth_pair(H, W, 91, dx=-1.0, dy=0.25)[0]
    seq = np.stack([A, prev, curr, Z]).astype(np.float32)
    d_f = _dev(seq)
    d_u = torch.empty((3, H, W), dtype=torch.float32, device=d_f.device)
    d_v = torch.empty_like(d_u)
    plan = _oflk.Plan(0, 3, H, W, L, 5, K)
    try:
        plan.pyramidal_sequence(d_f.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
        u0, v0, log0, runs0, flags = _read(plan, d_u, d_v, st)
        assert flags[1, 0] & 1, f"pair 1 not flagged: {flags}"
        assert not flags[0].any() and not flags[2].any(), flags
        n = plan.resolve_uncertain(d_f.data_ptr(), d_f.data_ptr() + H * W * 4, d_u.data_ptr(), d_v.data_ptr(), st)
        assert n == 1
        u1, v1, log1, runs1, flags1 = _read(plan, d_u, d_v, st)
        assert not flags1.any()
        ou, ov, _, oruns = oracle.lucas_kanade_pyramidal_ex(prev, curr, L, 5, K)
        assert list(runs1[1]) == list(oruns), (runs1[1], oruns)
        assert np.array_equal(u1[1], ou) and np.array_equal(v1[1], ov)
        for b in (0, 2):   # the neighbours are untouched, and are the oracle's
            assert np.array_equal(u1[b], u0[b]) and np.array_equal(v1[b], v0[b]), b
            assert np.array_equal(log1[b], log0[b]) and np.array_equal(runs1[b], runs0[b]), b
            ru, rv, _, rr = oracle.lucas_kanade_pyramidal_ex(seq[b], seq[b + 1], L, 5, K)
            assert np.array_equal(u1[b], ru) and np.array_equal(v1[b], rv) and list(runs1[b]) == list(rr), b
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. host entry points
# ---------------------------------------------------------------------------------------------------------------
def _host_pairs(frames, L, window, K):
    import _oflk

    T, H, W = frames.shape
    B = T - 1
    p, c = np.ascontiguousarray(frames[:-1]), np.ascontiguousarray(frames[1:])
    u, v = np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)
    log, runs = np.zeros((B, L, K, 2), np.float32), np.zeros((B, L), np.int32)
    if frames.dtype == np.uint8:
        rc = _oflk.lib().oflk_pyramidal_u8(p.ctypes.data, c.ctypes.data, B, H, W, L, window, K, _oflk.ptr(u), _oflk.ptr(v),
                                          _oflk.ptr(log), runs.ctypes.data_as(i32p))
    else:
        rc = _oflk.lib().oflk_pyramidal_batch(_oflk.ptr(p), _oflk.ptr(c), B, H, W, L, window, K, _oflk.ptr(u), _oflk.ptr(v),
                                             _oflk.ptr(log), runs.ctypes.data_as(i32p))
    _oflk.check(rc)
    return u, v, log, runs, int(_oflk.lib().oflk_last_resolved())


def _host_sequence(frames, L, window, K, n_gpus=None):
    import _oflk

    T, H, W = frames.shape
    B = T - 1
    f = np.ascontiguousarray(frames)
    u, v = np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)
    log, runs = np.zeros((B, L, K, 2), np.float32), np.zeros((B, L), np.int32)
    out = (_oflk.ptr(u), _oflk.ptr(v), _oflk.ptr(log), runs.ctypes.data_as(i32p))
    if n_gpus is not None:
        rc = _oflk.lib().oflk_pyramidal_sequence_multi(_oflk.ptr(f), T, H, W, L, window, K, n_gpus, *out)
    elif f.dtype == np.uint8:
        rc = _oflk.lib().oflk_pyramidal_sequence_u8(f.ctypes.data, T, H, W, L, window, K, *out)
    else:
        rc = _oflk.lib().oflk_pyramidal_sequence(_oflk.ptr(f), T, H, W, L, window, K, *out)
    _oflk.check(rc)
    return u, v, log, runs, int(_oflk.lib().oflk_last_resolved())


def _eq(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: output {i} differs"
        else:
            assert x == y, (what, i, x, y)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("T,H,W", [(9, 240, 320), (2, 37, 53), (19, 1080, 1920)], ids=["unchunked", "tiny", "chunked-ragged"])
def test_host_sequence_equals_host_pairs(T, H, W, u8):
    """(19, 1080p): 18 pairs go in chunks of four with a tail of two; each chunk uploads its five frames"""
    import _oflk

    frames = _video(T, H, W, seed=T, u8=u8)
    for arith in (0, 2):
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
        try:
            _eq(_host_sequence(frames, 3, 5, 3), _host_pairs(frames, 3, 5, 3), f"T={T} {H}x{W} arith {arith}")
        finally:
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))


def test_host_sequence_equals_plan_sequence():
    import torch

    import _oflk

    T, H, W = 7, 240, 320
    frames = _video(T, H, W, seed=5)
    st = torch.cuda.current_stream().cuda_stream
    d_f = _dev(frames)
    d_u = torch.empty((T - 1, H, W), dtype=torch.float32, device=d_f.device)
    d_v = torch.empty_like(d_u)
    plan = _oflk.Plan(0, T - 1, H, W, 3, 5, 3)
    try:
        plan.pyramidal_sequence(d_f.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
        u, v, log, runs, _ = _read(plan, d_u, d_v, st)
    finally:
        plan.close()
    _eq(_host_sequence(frames, 3, 5, 3)[:4], (u, v, log, runs), "host vs plan")


@pytest.mark.parametrize("window", [5, 7])
def test_single_scale_sequence_equals_batch(window):
    import _oflk

    for T, H, W in ((6, 240, 320), (3, 37, 53), (18, 1080, 1920)):
        frames = _video(T, H, W, seed=T)
        B = T - 1
        u, v = np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)
        _oflk.check(_oflk.lib().oflk_single_scale_sequence(_oflk.ptr(frames), T, H, W, window, _oflk.ptr(u), _oflk.ptr(v)))
        p, c = np.ascontiguousarray(frames[:-1]), np.ascontiguousarray(frames[1:])
        pu, pv = np.empty_like(u), np.empty_like(v)
        _oflk.check(_oflk.lib().oflk_single_scale_batch(_oflk.ptr(p), _oflk.ptr(c), B, H, W, window, _oflk.ptr(pu), _oflk.ptr(pv)))
        assert np.array_equal(u, pu) and np.array_equal(v, pv), (T, H, W, window)


def test_multi_sequence_under_rehearsal_equals_single_worker():
    import _oflk

    T, H, W = 12, 240, 320
    frames = _video(T, H, W, seed=12)
    want = _host_sequence(frames, 3, 5, 3)
    try:
        for workers in range(1, 6):
            _oflk.check(_oflk.lib().oflk_multi_rehearsal(workers))
            _eq(_host_sequence(frames, 3, 5, 3, n_gpus=1), want, f"{workers} workers")
    finally:
        _oflk.check(_oflk.lib().oflk_multi_rehearsal(0))


def test_invalid_sequence_calls_raise():
    import torch

    import _oflk
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    L = _oflk.lib()
    f = np.zeros((3, 16, 16), np.float32)
    u = np.empty((2, 16, 16), np.float32)
    log, runs = np.zeros((2, 3, 3, 2), np.float32), np.zeros((2, 3), np.int32)
    out = (_oflk.ptr(u), _oflk.ptr(u), _oflk.ptr(log), runs.ctypes.data_as(i32p))
    for T in (1, 0, -1):
        assert L.oflk_pyramidal_sequence(_oflk.ptr(f), T, 16, 16, 3, 5, 3, *out) == _oflk.OFLK_ERR_INVALID
        assert L.oflk_pyramidal_sequence_u8(f.ctypes.data, T, 16, 16, 3, 5, 3, *out) == _oflk.OFLK_ERR_INVALID
        assert L.oflk_pyramidal_sequence_multi(_oflk.ptr(f), T, 16, 16, 3, 5, 3, 1, *out) == _oflk.OFLK_ERR_INVALID
        assert L.oflk_single_scale_sequence(_oflk.ptr(f), T, 16, 16, 5, _oflk.ptr(u), _oflk.ptr(u)) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_pyramidal_sequence(None, 3, 16, 16, 3, 5, 3, *out) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_pyramidal_sequence(_oflk.ptr(f), 3, 16, 16, 3, 5, 3, None, _oflk.ptr(u), None, None) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_single_scale_sequence(_oflk.ptr(f), 3, 16, 16, 5, _oflk.ptr(u), None) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_pyramidal_sequence(_oflk.ptr(f), 3, 16, 16, 0, 5, 3, *out) == _oflk.OFLK_ERR_INVALID
    plan = _oflk.Plan(0, 2, 16, 16, 2, 5, 2)
    d = torch.zeros((3, 16, 16), dtype=torch.float32, device="cuda")
    try:
        with pytest.raises(ValueError):
            plan.pyramidal_sequence(0, d.data_ptr(), d.data_ptr())
        with pytest.raises(ValueError):
            plan.pyramidal_sequence(d.data_ptr(), 0, d.data_ptr())
    finally:
        plan.close()
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence(f[:1])
    with pytest.raises(ValueError):
        K.lucas_kanade_single_scale_sequence([f[0], f[0, :8]])


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_python_shims_equal_the_c_calls(u8):
    import _oflk
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    T, H, W = 5, 120, 160
    frames = _video(T, H, W, seed=4, u8=u8)
    u, v, log, runs, _ = _host_sequence(frames, 3, 5, 3)
    for given in (frames, list(frames)):
        su, sv, slog, sruns = P.lucas_kanade_pyramidal_sequence_with_log(given, 3, 5, 3)
        _eq((su, sv, slog, sruns), (u, v, log, runs), "pyramidal shim")
        pu, pv = P.lucas_kanade_pyramidal_sequence(given)
        assert np.array_equal(pu, u) and np.array_equal(pv, v)
    f32 = frames.astype(np.float32)
    cu, cv = np.empty((T - 1, H, W), np.float32), np.empty((T - 1, H, W), np.float32)
    _oflk.check(_oflk.lib().oflk_single_scale_sequence(_oflk.ptr(f32), T, H, W, 5, _oflk.ptr(cu), _oflk.ptr(cv)))
    ku, kv = K.lucas_kanade_single_scale_sequence(frames, 5)
    assert np.array_equal(ku, cu) and np.array_equal(kv, cv)
    for t in (0, T - 2):   # and the per-pair drop-ins
        pu, pv = P.lucas_kanade_pyramidal(frames[t], frames[t + 1])
        assert np.array_equal(pu, u[t]) and np.array_equal(pv, v[t])


# ---------------------------------------------------------------------------------------------------------------
# 5. the pyramid is built once per frame
# ---------------------------------------------------------------------------------------------------------------
def test_sequence_builds_each_pyramid_once():
    """129 frames of 1080p against the 128 pairs they make: the sequence's pyr_down time is at most 0.6 x the batch's
    (expected 0.50: 129 images instead of 256)"""
    import torch

    import _oflk

    T, H, W, B = 129, 1080, 1920, 128
    rng = np.random.default_rng(11)
    frames = (rng.random((T, H, W), dtype=np.float32) * 255.0).astype(np.float32)
    st = torch.cuda.current_stream().cuda_stream
    d_f = _dev(frames)
    d_p, d_c = d_f[:-1].clone(), d_f[1:].clone()
    d_u = torch.empty((B, H, W), dtype=torch.float32, device=d_f.device)
    d_v = torch.empty_like(d_u)
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)

    def pyr_ms(seq):
        plan.set_profiling(True)
        for _ in range(3):
            if seq:
                plan.pyramidal_sequence(d_f.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
            else:
                plan.pyramidal(d_p.data_ptr(), d_c.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), st)
        torch.cuda.synchronize()
        times = plan.kernel_times()
        plan.set_profiling(False)
        return sum(t["total_ms"] for name, t in times.items() if name.startswith("pyr_") or name == "blur")

    try:
        pyr_ms(False)
        pyr_ms(True)   # warm-up of both forms
        pairs, seqs = [], []
        for _ in range(2):
            pairs.append(pyr_ms(False))
            seqs.append(pyr_ms(True))
    finally:
        plan.close()
    ratio = min(seqs) / min(pairs)
    assert min(pairs) > 0
    assert ratio <= 0.6, f"sequence pyramid {min(seqs):.3f} ms vs pair batch {min(pairs):.3f} ms: ratio {ratio:.3f}"
