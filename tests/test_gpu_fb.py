"""GPU tests of the forward-backward entry points (run on an MI355X: python -m pytest tests/test_gpu_fb.py -m gpu -q).

The bidirectional sequence pass builds the B+1 frames' pyramid once and runs the level loop twice.  Its forward half must
equal oflk_plan_pyramidal_sequence on the frames, and its backward half the same call on the reversed frames, bit for
bit (flows, logs, iteration counts, uncertain flags, level flows), in every arithmetic mode and on every kernel path.
oflk_fb_consistency must equal the NumPy statement of tests/fb_model.py byte for byte.
"""
import ctypes
import itertools

import numpy as np
import pytest

import fb_model as M
from test_gpu_exit_band import ARITH, THR, _reference
from test_gpu_sequence import CASES, _dev, _oflk_dims, _video
from test_tolerant_model import device_mean_error, level_sum_path, numpy_mean_error

pytestmark = pytest.mark.gpu

ALPHA_BETA = ((0.01, 0.5), (0.0, 0.0), (0.05, 1e6))


def _same(x, y, what):
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
    if not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
        bad = np.argwhere(x != y) if x.dtype != np.float32 else np.argwhere(x.view(np.int32) != y.view(np.int32))
        first = tuple(bad[0]) if len(bad) else None
        pytest.fail(f"{what} differs at {len(bad)} elements, first {first}: {x[first] if first else ''} vs {y[first] if first else ''}")


def _run(plan, frames_dev, B, H, W, L, st, u8, fb):
    """one pass of `plan`: the sequence (fb False) or the bidirectional pass; flows, logs, flags and level flows of every
    pair after it (level flows: the backward pass's after a bidirectional pass)"""
    import torch

    du = [torch.full((B, H, W), float("nan"), dtype=torch.float32, device=frames_dev.device) for _ in range(4 if fb else 2)]
    if fb:
        plan.pyramidal_sequence_fb(frames_dev.data_ptr(), *(d.data_ptr() for d in du), st, u8=u8)
    else:
        plan.pyramidal_sequence(frames_dev.data_ptr(), du[0].data_ptr(), du[1].data_ptr(), st, u8=u8)
    out = {"fwd": [d.cpu().numpy() for d in du[:2]] + list(plan.read_log(st)) + [plan.read_uncertain(st)]}
    if fb:
        out["bwd"] = [d.cpu().numpy() for d in du[2:]] + list(plan.read_log_backward(st)) + [plan.read_uncertain_backward(st)]
    dims = _oflk_dims(H, W, L)
    out["levels"] = [[plan.read_level_flow(l, b, dims[l], st) for l in range(L - 1)] for b in range(B)]
    torch.cuda.synchronize()
    return out


def _fb_and_references(frames, L, window, K, mode, u8):
    import torch

    import _oflk

    T, H, W = frames.shape
    B = T - 1
    st = torch.cuda.current_stream().cuda_stream
    d_f, d_r = _dev(frames), _dev(frames[::-1].copy())
    plan = _oflk.Plan(0, B, H, W, L, window, K)
    try:
        plan.set_arithmetic(ARITH[mode])
        fwd = _run(plan, d_f, B, H, W, L, st, u8, False)
        rev = _run(plan, d_r, B, H, W, L, st, u8, False)
        fb = _run(plan, d_f, B, H, W, L, st, u8, True)
        fb2 = _run(plan, d_f, B, H, W, L, st, u8, True)   # the second call (state block already there) is the same
    finally:
        plan.close()
    return fwd, rev, fb, fb2


def _assert_fb_is_two_sequences(fwd, rev, fb, what):
    names = ("u", "v", "log", "iters_run", "uncertain")
    for name, x, y in zip(names, fb["fwd"], fwd["fwd"]):
        _same(x, y, f"{what}: forward {name}")
    B = fb["bwd"][0].shape[0]
    for name, x, y in zip(names, fb["bwd"], rev["fwd"]):
        _same(x, y[::-1], f"{what}: backward {name}")
    for b in range(B):
        for l, ((xu, xv), (yu, yv)) in enumerate(zip(fb["levels"][b], rev["levels"][B - 1 - b])):
            _same(xu, yu, f"{what}: backward level {l} u of pair {b}")
            _same(xv, yv, f"{what}: backward level {l} v of pair {b}")


# ---------------------------------------------------------------------------------------------------------------
# 1. backward = the sequence pass on the reversed frames, forward = the sequence pass, bit for bit
# ---------------------------------------------------------------------------------------------------------------
FB_CASES = CASES + (
    (240, 320, 1, 1, 5, (3,), ("exact", "tolerant")),    # (L, K) = (1, 1): no pyramid at all
    (37, 53, 1, 1, 3, (4,), ("exact",)),
)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("case", FB_CASES, ids=lambda c: f"{c[0]}x{c[1]}-L{c[2]}K{c[3]}-w{c[4]}")
def test_fb_equals_sequence_and_reversed_sequence(case, u8):
    H, W, L, K, window, Ts, modes = case
    for T in Ts:
        frames = _video(T, H, W, seed=3 * T + W, u8=u8)
        for mode in modes:
            what = f"{H}x{W} L{L} K{K} w{window} T={T} {mode} {'u8' if u8 else 'f32'}"
            fwd, rev, fb, fb2 = _fb_and_references(frames, L, window, K, mode, u8)
            _assert_fb_is_two_sequences(fwd, rev, fb, what)
            _assert_fb_is_two_sequences(fwd, rev, fb2, what + " (second call)")


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_fb_equals_sequences_1080p(u8):
    frames = _video(4, 1080, 1920, seed=8, u8=u8)
    for mode in ("exact", "tolerant"):
        fwd, rev, fb, _ = _fb_and_references(frames, 3, 5, 3, mode, u8)
        _assert_fb_is_two_sequences(fwd, rev, fb, f"1080p {mode}")


# ---------------------------------------------------------------------------------------------------------------
# 2. against the oracle, and 4a. the consistency of those flows = the statement
# ---------------------------------------------------------------------------------------------------------------
def test_patterns_backward_equals_oracle_and_check_equals_statement(oracle, golden_dir):
    import flow_metrics
    import lucas_kanade_pyramidal as P

    z = np.load(golden_dir / "patterns_320x240.npz")
    names = [k[len("frame_1__"):] for k in z.files if k.startswith("frame_1__")]
    assert len(names) == 13
    prev = z["frame_0"].astype(np.float32)
    for name in names:
        curr = z[f"frame_1__{name}"].astype(np.float32)
        r = P.lucas_kanade_pyramidal_sequence_fb(np.stack([prev, curr]))
        assert all(a.shape == (1, 240, 320) for a in r)
        ou, ov = oracle.lucas_kanade_pyramidal(prev, curr, 3, 5, 3)
        bu, bv = oracle.lucas_kanade_pyramidal(curr, prev, 3, 5, 3)
        assert np.array_equal(r.u_fwd[0], ou) and np.array_equal(r.v_fwd[0], ov), f"{name}: forward differs from the oracle"
        assert np.array_equal(r.u_bwd[0], bu) and np.array_equal(r.v_bwd[0], bv), f"{name}: backward differs from the oracle"
        ef, eb, qf, qb = M.fb_check(r.u_fwd, r.v_fwd, r.u_bwd, r.v_bwd, 0.01, 0.5)
        _same(r.err_fwd, ef, f"{name}: err_fwd")
        _same(r.err_bwd, eb, f"{name}: err_bwd")
        _same(r.valid_fwd, qf.astype(bool), f"{name}: valid_fwd")
        _same(r.valid_bwd, qb.astype(bool), f"{name}: valid_bwd")
        for alpha, beta in ALPHA_BETA:
            got = flow_metrics.forward_backward_consistency(r.u_fwd, r.v_fwd, r.u_bwd, r.v_bwd, alpha, beta)
            want = M.fb_check(r.u_fwd, r.v_fwd, r.u_bwd, r.v_bwd, alpha, beta)
            for i, (x, y) in enumerate(zip(got, want)):
                _same(x, y.astype(bool) if i >= 2 else y, f"{name} alpha={alpha} beta={beta} output {i}")


# ---------------------------------------------------------------------------------------------------------------
# 3. a flagged backward decision, resolved in the backward state only
# ---------------------------------------------------------------------------------------------------------------
def test_flagged_backward_pair_resolves(oracle):
    """frames [A, X, Y, Z] with (Y, X) bisected so that its exit decision after iteration 1 lands just inside the band (as in
    test_flagged_inner_pair_resolves_with_aliased_pointers): backward pair 1 is Y -> X.  Only it is flagged, in the
    backward state; resolve_uncertain_sequence_fb redoes it to the oracle's flow and counts, and the forward results and
    the other backward pairs stay as they were."""
    import torch

    import _oflk
    from oflk_synth import synth_pair

    H, W, L, K, mode = 48, 64, 2, 3, "exact"
    h, w = oracle.pyramid_dims(H, W, L)[0]
    path = level_sum_path(ARITH[mode], L, K, 5, oracle.pyramid_dims(H, W, L), 0)
    S = numpy_mean_error(h * w) + device_mean_error(path, h, w, THR)
    st = torch.cuda.current_stream().cuda_stream

    # The first decision of a pair and of its reverse are the same number: the reference's gradients use the average of
    # the two frames and It changes sign, so iteration 0's update is exactly negated.  The decision after iteration 1
    # (after a warp) differs by ~10 % between the directions: that one is placed in the band.
    def place(seed, off):
        a, shifted = synth_pair(H, W, seed, dx=0.75, dy=-0.5)
        delta = (shifted - a).astype(np.float64)
        frames = lambda t: (a + t * delta).astype(np.float32)  # noqa: E731
        mean = lambda t: float(max(_reference(oracle, mode, a, frames(t), L, K, 5)[4][0, 1]))  # noqa: E731
        target = THR * (1.0 + off)
        lo, hi = 0.0, 1.0
        assert mean(lo) < target < mean(hi)   # t = 0: equal frames, the level exits after iteration 0 (mean 0 here)
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean(mid) < target else (lo, mid)
        t = min((lo, hi), key=lambda e: abs(mean(e) - target))
        return a, frames(t), mean(t) / THR - 1.0

    A = synth_pair(H, W, 90, dx=1.0, dy=0.5)[0]
    Z = synth_pair(H, W, 91, dx=-1.0, dy=0.25)[0]
    tried = []
    plan = _oflk.Plan(0, 3, H, W, L, 5, K)
    try:
        for seed in range(16):
            y_, x_, rel = place(seed, 0.5 * S)   # the pair (Y, X) = (y_, x_) is in the band
            tried.append(rel)
            if not 0.0 < rel < S:
                continue
            seq = np.stack([A, x_, y_, Z]).astype(np.float32)
            d_f = _dev(seq)
            d = [torch.empty((3, H, W), dtype=torch.float32, device=d_f.device) for _ in range(4)]
            plan.pyramidal_sequence_fb(d_f.data_ptr(), *(t.data_ptr() for t in d), st)
            flags_f, flags_b = plan.read_uncertain(st), plan.read_uncertain_backward(st)
            if flags_f.any():   # X -> Y happened to land in its band too: take another seed
                tried[-1] = ("forward flagged", rel)
                continue
            break
        else:
            pytest.fail(f"no backward-only flagged pair: {tried}")
        assert flags_b[1, 0] & 2, f"backward pair 1 not flagged after iteration 1: {flags_b}"
        assert not flags_b[0].any() and not flags_b[2].any(), flags_b
        before = [t.cpu().numpy() for t in d]
        log_f0, runs_f0 = plan.read_log(st)
        log_b0, runs_b0 = plan.read_log_backward(st)
        n = plan.resolve_uncertain_sequence_fb(d_f.data_ptr(), *(t.data_ptr() for t in d), st)
        assert n == 1
        after = [t.cpu().numpy() for t in d]
        log_f1, runs_f1 = plan.read_log(st)
        log_b1, runs_b1 = plan.read_log_backward(st)
        assert not plan.read_uncertain_backward(st).any() and not plan.read_uncertain(st).any()
        for i in (0, 1):   # forward results untouched
            _same(after[i], before[i], f"forward output {i}")
        _same(log_f1, log_f0, "forward log")
        _same(runs_f1, runs_f0, "forward iters_run")
        ou, ov, _, oruns = oracle.lucas_kanade_pyramidal_ex(y_, x_, L, 5, K)
        assert list(runs_b1[1]) == list(oruns), (runs_b1[1], oruns)
        assert np.array_equal(after[2][1], ou) and np.array_equal(after[3][1], ov)
        for b in (0, 2):
            _same(after[2][b], before[2][b], f"backward pair {b}")
            _same(runs_b1[b], runs_b0[b], f"backward runs {b}")
            ru, rv, _, rr = oracle.lucas_kanade_pyramidal_ex(seq[b + 1], seq[b], L, 5, K)
            assert np.array_equal(after[2][b], ru) and np.array_equal(after[3][b], rv) and list(runs_b1[b]) == list(rr), b
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 4b. the consistency kernel = the statement on random flows, every shape form and every subset of outputs
# ---------------------------------------------------------------------------------------------------------------
def _random_flows(B, H, W, seed):
    """smooth random flows up to +-W px (and +-H vertically), with every tenth pixel's target put exactly on a border or
    one float32 step outside it"""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(4):
        f = np.stack([gaussian_filter(rng.standard_normal((H, W)), 2.0, mode="wrap") for _ in range(B)])
        f = f / max(np.abs(f).max(), 1e-12)
        out.append(f)
    uf, vf, ub, vb = (out[0] * W).astype(np.float32), (out[1] * H).astype(np.float32), (out[2] * W).astype(np.float32), \
        (out[3] * H).astype(np.float32)
    xx = np.broadcast_to(np.arange(W, dtype=np.float32)[None, None, :], (B, H, W))
    yy = np.broadcast_to(np.arange(H, dtype=np.float32)[None, :, None], (B, H, W))
    for u, v in ((uf, vf), (ub, vb)):
        pick = rng.random((B, H, W)) < 0.1
        kind = rng.integers(0, 4, (B, H, W))
        tx = np.where(kind == 0, 0.0, np.where(kind == 1, W - 1.0, np.where(kind == 2, -np.float32(2.0 ** -20), W - 1 + 2.0 ** -18)))
        u[pick] = (tx - xx)[pick].astype(np.float32)
        pick = rng.random((B, H, W)) < 0.1
        kind = rng.integers(0, 4, (B, H, W))
        ty = np.where(kind == 0, 0.0, np.where(kind == 1, H - 1.0, np.where(kind == 2, -np.float32(2.0 ** -20), H - 1 + 2.0 ** -18)))
        v[pick] = (ty - yy)[pick].astype(np.float32)
    return uf, vf, ub, vb


def _device_check(flows, alpha, beta, want=(True, True, True, True)):
    import torch

    import _oflk

    B, H, W = flows[0].shape
    d = [_dev(f) for f in flows]
    outs = [torch.full((B, H, W), -7.0, dtype=torch.float32, device=d[0].device) for _ in range(2)] + \
        [torch.full((B, H, W), 9, dtype=torch.uint8, device=d[0].device) for _ in range(2)]
    ptrs = [o.data_ptr() if w else 0 for o, w in zip(outs, want)]
    _oflk.fb_consistency(*(x.data_ptr() for x in d), B, H, W, alpha, beta, *ptrs,
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 7), (3, 9, 1), (4, 37, 53), (1, 240, 320), (2, 64, 64), (1, 1, 300)])
def test_check_equals_statement_on_random_flows(shape):
    B, H, W = shape
    flows = _random_flows(B, H, W, seed=B * 1000 + H * 7 + W)
    for alpha, beta in ALPHA_BETA:
        got = _device_check(flows, alpha, beta)
        want = M.fb_check(*flows, alpha, beta)
        for i, (x, y) in enumerate(zip(got, want)):
            _same(x, y, f"{shape} alpha={alpha} beta={beta} output {i}")


def test_check_writes_exactly_the_outputs_asked_for():
    flows = _random_flows(2, 23, 29, seed=5)
    want = M.fb_check(*flows, 0.01, 0.5)
    for mask in itertools.product((False, True), repeat=4):
        if not any(mask):
            continue
        got = _device_check(flows, 0.01, 0.5, mask)
        for i, (x, y, asked) in enumerate(zip(got, want, mask)):
            if asked:
                _same(x, y, f"outputs {mask}: output {i}")
            else:   # left as filled
                assert (x == (-7.0 if i < 2 else 9)).all(), f"outputs {mask}: output {i} was written"


# ---------------------------------------------------------------------------------------------------------------
# 5. the host form = the plan form + resolve + check
# ---------------------------------------------------------------------------------------------------------------
def _host_fb(frames, L, window, K, alpha=0.01, beta=0.5):
    import _oflk

    T, H, W = frames.shape
    f = np.ascontiguousarray(frames)
    out = [np.empty((T - 1, H, W), np.float32) for _ in range(6)] + [np.empty((T - 1, H, W), np.uint8) for _ in range(2)]
    fn = _oflk.lib().oflk_pyramidal_sequence_fb_u8 if f.dtype == np.uint8 else _oflk.lib().oflk_pyramidal_sequence_fb
    _oflk.check(fn(f.ctypes.data if f.dtype == np.uint8 else _oflk.ptr(f), T, H, W, L, window, K, alpha, beta,
                   *(_oflk.ptr(o) for o in out[:6]), out[6].ctypes.data, out[7].ctypes.data))
    return out, int(_oflk.lib().oflk_last_resolved())


def _plan_fb(frames, L, window, K, alpha=0.01, beta=0.5, arith=0):
    import torch

    import _oflk

    T, H, W = frames.shape
    B = T - 1
    u8 = frames.dtype == np.uint8
    st = torch.cuda.current_stream().cuda_stream
    d_f = _dev(frames)
    d = [torch.empty((B, H, W), dtype=torch.float32, device=d_f.device) for _ in range(6)] + \
        [torch.empty((B, H, W), dtype=torch.uint8, device=d_f.device) for _ in range(2)]
    plan = _oflk.Plan(0, B, H, W, L, window, K)
    try:
        plan.set_arithmetic(arith)
        plan.pyramidal_sequence_fb(d_f.data_ptr(), *(t.data_ptr() for t in d[:4]), st, u8=u8)
        n = plan.resolve_uncertain_sequence_fb(d_f.data_ptr(), *(t.data_ptr() for t in d[:4]), st, u8=u8)
        _oflk.fb_consistency(*(t.data_ptr() for t in d[:4]), B, H, W, alpha, beta, *(t.data_ptr() for t in d[4:]), stream=st)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in d], n
    finally:
        plan.close()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("T,H,W", [(5, 240, 320), (2, 37, 53), (33, 1080, 1920)], ids=["small", "odd", "chunked-1080p"])
def test_host_equals_plan(T, H, W, u8):
    """(33, 1080p): 32 pairs go in eight chunks of four, each uploading five frames"""
    import _oflk

    frames = _video(T, H, W, seed=T + 1, u8=u8)
    for arith in (0, 2):
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
        try:
            got, n_host = _host_fb(frames, 3, 5, 3)
        finally:
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
        want, n_plan = _plan_fb(frames, 3, 5, 3, arith=arith)
        assert n_host == n_plan
        for i, (x, y) in enumerate(zip(got, want)):
            _same(x, y, f"T={T} {H}x{W} arith {arith} output {i}")


def test_python_shim_equals_host_call():
    import lucas_kanade_pyramidal as P

    frames = _video(4, 120, 160, seed=2, u8=True)
    got, _ = _host_fb(frames, 3, 5, 3, 0.02, 0.25)
    for given in (frames, list(frames)):
        r = P.lucas_kanade_pyramidal_sequence_fb(given, 3, 5, 3, alpha=0.02, beta=0.25)
        for i, (x, y) in enumerate(zip(r, got)):
            _same(x, y.astype(bool) if i >= 6 else y, f"field {r._fields[i]}")


# ---------------------------------------------------------------------------------------------------------------
# 6. meaning: an occluder's covered strip fails the test, pixels far from motion boundaries pass
# ---------------------------------------------------------------------------------------------------------------
def test_occluded_strip_is_invalid_and_far_pixels_are_valid(oracle):
    import lucas_kanade_pyramidal as P

    H, W, S, step = 96, 128, 36, (3, 1)
    frames, corners = M.occluder_scene(3, H, W, S, step)
    r = P.lucas_kanade_pyramidal_sequence_fb(frames)
    for t in range(2):
        uf, vf = oracle.lucas_kanade_pyramidal(frames[t], frames[t + 1], 3, 5, 3)
        ub, vb = oracle.lucas_kanade_pyramidal(frames[t + 1], frames[t], 3, 5, 3)
        ef, eb, qf, qb = M.fb_check(uf, vf, ub, vb)
        _same(r.err_fwd[t], ef, "err_fwd")
        _same(r.err_bwd[t], eb, "err_bwd")
        _same(r.valid_fwd[t], qf.astype(bool), "valid_fwd")
        _same(r.valid_bwd[t], qb.astype(bool), "valid_bwd")
        covered, far = M.scene_regions(corners, t, H, W, S, step, 6)
        assert r.valid_fwd[t][covered].mean() <= 0.35, r.valid_fwd[t][covered].mean()
        assert r.valid_fwd[t][far].mean() >= 0.85, r.valid_fwd[t][far].mean()


# ---------------------------------------------------------------------------------------------------------------
# 7. graph capture
# ---------------------------------------------------------------------------------------------------------------
def test_fb_pass_and_check_replay_from_a_graph():
    """after one eager call on a single stream, the bidirectional pass plus the check captured on a side stream replay to
    the eager bytes (tolerant mode: the streaming kernels too)"""
    import torch

    import _oflk

    T, H, W, L, K = 5, 240, 320, 3, 3
    B = T - 1
    dev = torch.device("cuda", 0)
    frames = _dev(_video(T, H, W, seed=21))
    d = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(6)] + \
        [torch.empty((B, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    for arith in (0, 2):
        plan = _oflk.Plan(0, B, H, W, L, 5, K)
        try:
            plan.set_arithmetic(arith)

            def enqueue(s_):
                plan.pyramidal_sequence_fb(frames.data_ptr(), *(t.data_ptr() for t in d[:4]), s_)
                _oflk.fb_consistency(*(t.data_ptr() for t in d[:4]), B, H, W, 0.01, 0.5, *(t.data_ptr() for t in d[4:]), stream=s_)

            enqueue(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            eager = [t.cpu().numpy() for t in d]
            side = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                enqueue(torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                for t in d:
                    t.zero_()
                g.replay()
                torch.cuda.synchronize()
                for i, (x, y) in enumerate(zip(d, eager)):
                    _same(x.cpu().numpy(), y, f"arith {arith} replay {rep} output {i}")
            del g
        finally:
            plan.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. invalid calls
# ---------------------------------------------------------------------------------------------------------------
def test_invalid_fb_calls_raise():
    import torch

    import _oflk
    import lucas_kanade_pyramidal as P

    L = _oflk.lib()
    H = W = 16
    f = np.zeros((3, H, W), np.float32)
    o = [np.empty((2, H, W), np.float32) for _ in range(6)]
    q = [np.empty((2, H, W), np.uint8) for _ in range(2)]
    outs = [_oflk.ptr(x) for x in o] + [x.ctypes.data for x in q]
    INV = _oflk.OFLK_ERR_INVALID
    for T in (1, 0, -1):
        assert L.oflk_pyramidal_sequence_fb(_oflk.ptr(f), T, H, W, 3, 5, 3, 0.01, 0.5, *outs) == INV
        assert L.oflk_pyramidal_sequence_fb_u8(f.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, *outs) == INV
    for alpha, beta in ((-1.0, 0.5), (0.01, -0.5), (float("nan"), 0.5), (0.01, float("nan")), (float("inf"), 0.5)):
        assert L.oflk_pyramidal_sequence_fb(_oflk.ptr(f), 3, H, W, 3, 5, 3, alpha, beta, *outs) == INV
        assert L.oflk_fb_consistency_host(*outs[:4], 2, H, W, alpha, beta, *outs[4:]) == INV
    assert L.oflk_pyramidal_sequence_fb(None, 3, H, W, 3, 5, 3, 0.01, 0.5, *outs) == INV
    for i in range(4):   # each flow output is required
        bad = list(outs)
        bad[i] = None
        assert L.oflk_pyramidal_sequence_fb(_oflk.ptr(f), 3, H, W, 3, 5, 3, 0.01, 0.5, *bad) == INV
    assert L.oflk_fb_consistency_host(*outs[:4], 2, H, W, 0.01, 0.5, None, None, None, None) == INV
    assert L.oflk_fb_consistency_host(*outs[:4], 0, H, W, 0.01, 0.5, *outs[4:]) == INV

    dev = torch.device("cuda", 0)
    d_f = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    d = [torch.empty((2, H, W), dtype=torch.float32, device=dev) for _ in range(4)]
    dq = torch.empty((2, H, W), dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in d]
    plan = _oflk.Plan(0, 2, H, W, 2, 5, 2)
    try:
        with pytest.raises(ValueError):   # read / resolve of a backward pass that never ran
            plan.read_log_backward()
        with pytest.raises(ValueError):
            plan.read_uncertain_backward()
        with pytest.raises(ValueError):
            plan.resolve_uncertain_sequence_fb(d_f.data_ptr(), *p)
        for i in range(5):
            args = [d_f.data_ptr()] + p
            args[i] = 0
            with pytest.raises(ValueError):
                plan.pyramidal_sequence_fb(*args)
        with pytest.raises(ValueError):
            _oflk.fb_consistency(*p, 2, H, W, 0.01, 0.5)   # no output
        for B in (0, -1):
            with pytest.raises(ValueError):
                _oflk.fb_consistency(*p, B, H, W, 0.01, 0.5, d_valid_f=dq.data_ptr())
        for alpha, beta in ((-0.1, 0.5), (float("nan"), 0.5), (0.01, -2.0), (0.01, float("inf"))):
            with pytest.raises(ValueError):
                _oflk.fb_consistency(*p, 2, H, W, alpha, beta, d_valid_f=dq.data_ptr())
    finally:
        plan.close()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_fb(f[:1])
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_fb(f, alpha=float("nan"))
