"""GPU tests of frame interpolation (run on an MI355X: python -m pytest tests/test_gpu_interp.py -m gpu -q).

oflk_interpolate_frames and its host forms must equal the NumPy statement of tests/interp_model.py byte for byte, frames and
status, float32 and uint8, on every shape form, on flows that throw points out of the frame and on flows with NaN, infinities
and 1e30 planted in them.  oflk_interpolate_sequence must equal oflk_pyramidal_sequence_fb followed by the host form.
"""
import numpy as np
import pytest

import fb_model as FM
import interp_model as M
from test_gpu_fb import _host_fb, _same
from test_gpu_sequence import _dev, _video

pytestmark = pytest.mark.gpu

TAUS = [0.5, 1 / 3, 0.25, 2.0 ** -20, 1 - 2.0 ** -20]
BLOCK = (4, 64)   # k_interp's block: rows x columns of output pixels
SHAPES = [(1, 1), (1, 7), (5, 1), (2, 2), (37, 53)] + [(BLOCK[0] + d, BLOCK[1] + d) for d in (-1, 0, 1)]
# (B, taus, refine, status given): every B, n, R and status form of the statement's cases, each tau of TAUS in some case
CONFIGS = [
    (1, TAUS[:1], 2, True),
    (3, TAUS[1:4], 1, False),
    (1, TAUS + list(np.linspace(0.05, 0.95, 11)), 4, True),
    (3, TAUS[4:], 2, True),
    (1, TAUS[2:5], 4, False),
]


def _frames(B, H, W, seed, u8):
    f = np.random.default_rng(seed).random((B + 1, H, W)) * 255.0
    return np.rint(f).astype(np.uint8) if u8 else f.astype(np.float32)


def _amplitude(H, W, px):
    """per plane (u, v, u, v) the size of a tame flow: up to px, a third of the axis at most, 0 along an axis of one pixel"""
    ax, ay = min(px, (W - 1) / 3), min(px, (H - 1) / 3)
    return np.array([ax, ay, ax, ay]).reshape(4, 1, 1, 1)


def _wild_flows(B, H, W, seed):
    """random fields of up to 2 W px (most points leave the frame on the first step), a quarter of the pixels tamed to a
    few px so that every branch is taken"""
    rng = np.random.default_rng(seed)
    f = (rng.random((4, B, H, W)) * 2 - 1) * 2 * W
    tame = rng.random((B, H, W)) < 0.25
    small = (rng.random((4, B, H, W)) * 2 - 1) * _amplitude(H, W, 3.0)
    small[2:] = -small[:2] + 0.2 * small[2:]
    f[:, tame] = small[:, tame]
    return [np.ascontiguousarray(a, np.float32) for a in f]


def _planted_flows(B, H, W, seed):
    """small consistent flows with NaN, +-inf and 1e30 planted at a handful of pixels of every plane"""
    rng = np.random.default_rng(seed)
    f = (rng.random((4, B, H, W)) * 2 - 1) * _amplitude(H, W, 2.0)
    f[2:] = -f[:2] + 0.1 * f[2:]
    f = f.astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    for p in range(4):
        k = min(5, H * W) if H * W > 1 else (1 if p == seed % 4 else 0)
        idx = rng.choice(B * H * W, size=k, replace=False)
        f[p].reshape(-1)[idx] = rng.permutation(bad)[:k]
    return [np.ascontiguousarray(a) for a in f]


def _device(frames, flows, taus, alpha=0.01, beta=0.5, refine=2, status=True):
    import torch

    import _oflk

    B, H, W = flows[0].shape
    n = len(taus)
    d_fr, d = _dev(frames), [_dev(f) for f in flows]
    out = torch.full((B, n, H, W), 77, dtype=d_fr.dtype, device=d_fr.device)
    st = torch.full((B, n, H, W), 9, dtype=torch.uint8, device=d_fr.device)
    _oflk.interpolate_frames(d_fr.data_ptr(), B, H, W, *(x.data_ptr() for x in d), taus, out.data_ptr(), st.data_ptr() if status else 0,
                             alpha, beta, refine, u8=frames.dtype == np.uint8, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if not status:
        assert (st == 9).all()
    return out.cpu().numpy(), st.cpu().numpy() if status else None


def _check_all_forms(frames, flows, taus, refine, status, what, alpha=0.01, beta=0.5):
    """the device form and the host form against the statement; returns the statement's (new, status)"""
    import lucas_kanade_pyramidal as P

    want = M.interpolate(frames, *flows, taus, alpha, beta, refine)
    assert np.isfinite(want[0].astype(np.float64)).all()
    got = _device(frames, flows, taus, alpha, beta, refine, status)
    _same(got[0], want[0], f"{what}: device frames")
    if status:
        _same(got[1], want[1], f"{what}: device status")
    host = P.interpolate_frames(frames, *flows, taus=taus, alpha=alpha, beta=beta, refine=refine, return_status=status)
    _same(host[0] if status else host, want[0], f"{what}: host frames")
    if status:
        _same(host[1], want[1], f"{what}: host status")
    return want


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda s: str(s))
def test_kernel_equals_statement(H, W, u8):
    codes = set()
    for i, (B, taus, refine, status) in enumerate(CONFIGS):
        frames = _frames(B, H, W, seed=H * 100 + W + i, u8=u8)
        for kind, make in (("wild", _wild_flows), ("planted", _planted_flows)):
            flows = make(B, H, W, seed=H * 7 + W + i)
            want = _check_all_forms(frames, flows, taus, refine, status, f"{H}x{W} {kind} config {i}")
            codes |= set(np.unique(want[1]).tolist())
    if H * W > 100:
        assert codes == {0, 1, 2, 3}


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_oracle_flows_on_the_occluder_scene(oracle, u8):
    frames, _ = FM.occluder_scene(T=3)
    flows = M.oracle_flows(oracle, frames)
    if u8:
        frames = np.rint(frames).astype(np.uint8)
    want = _check_all_forms(frames, flows, TAUS[:3], 2, True, "occluder scene")
    counts = np.bincount(want[1][:, 0].ravel(), minlength=4)
    assert (counts > 0).all() and counts[3] > 0.7 * want[1][:, 0].size
    for alpha, beta in ((0.0, 0.0), (0.05, 1e6)):
        _check_all_forms(frames, flows, [0.5], 2, True, f"occluder scene alpha={alpha} beta={beta}", alpha, beta)


def test_more_slices_than_the_grid_z_limit():
    """B = 4100 pairs of 2 x 3 frames at n = 16: 65600 slices, cut at 65535.  Frames and flows repeat with period 7 (7 divides
    neither 16 nor 65535), so the statement is evaluated on 7 pairs; a slice given another pair's data or time shows"""
    B, H, W, P_ = 4100, 2, 3, 7
    taus = TAUS + list(np.linspace(0.05, 0.95, 11))
    base = _frames(P_ - 1, H, W, seed=5, u8=False)                      # P_ frames
    fbase = _planted_flows(P_, H, W, seed=7)
    for k in range(4):
        fbase[k][::3] = _wild_flows(P_, H, W, seed=6)[k][::3]
        fbase[k][1] *= np.float32(0.125)   # a pair whose points stay inside
    want = M.interpolate(np.concatenate([base, base[:1]]), *fbase, taus)
    for u8 in (False, True):
        if u8:
            base8 = np.rint(base).astype(np.uint8)
            want = M.interpolate(np.concatenate([base8, base8[:1]]), *fbase, taus)
        src = base8 if u8 else base
        frames = src[np.arange(B + 1) % P_]
        flows = [f[np.arange(B) % P_] for f in fbase]
        got = _device(frames, flows, taus)
        idx = np.arange(B) % P_
        _same(got[0], want[0][idx], f"z limit u8={u8}: frames")
        _same(got[1], want[1][idx], f"z limit u8={u8}: status")


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_sequence_equals_fb_then_host_form(u8):
    import _oflk
    import lucas_kanade_pyramidal as P

    T, H, W = 4, 64, 80
    frames = _video(T, H, W, seed=3, u8=u8)
    taus = [0.25, 0.5, 0.75]
    for arith in (0, 2):
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
        try:
            fb, n_fb = _host_fb(frames, 3, 5, 3)
            r = P.lucas_kanade_pyramidal_sequence_interpolate(frames, taus=taus)
            n_seq = int(_oflk.lib().oflk_last_resolved())
        finally:
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
        assert n_seq == n_fb
        new, status = P.interpolate_frames(frames, *fb[:4], taus=taus, return_status=True)
        _same(r.new, new, f"arith {arith}: new frames")
        _same(r.status, status, f"arith {arith}: status")
        if arith == 0:
            want = M.interpolate(frames, *fb[:4], taus)
            _same(r.new, want[0], "statement: frames")
            _same(r.status, want[1], "statement: status")
            assert (status == 3).mean() > 0.5   # not a comparison of fallbacks: most pixels pass on both sides


def test_chunked_1080p_equals_host_form_on_the_downloaded_flows():
    """T = 18 at 1080p: the chunk rule (chunk_pairs) cuts the 17 pairs into chunks of 4, 4, 4, 4 and 1"""
    import lucas_kanade_pyramidal as P

    T, H, W = 18, 1080, 1920
    frames = _video(T, H, W, seed=4, u8=True)
    r = P.lucas_kanade_pyramidal_sequence_interpolate(frames, factor=2)
    fb, _ = _host_fb(frames, 3, 5, 3)
    new, status = P.interpolate_frames(frames, *fb[:4], return_status=True)
    _same(r.new, new, "1080p pipeline vs host form: frames")
    _same(r.status, status, "1080p pipeline vs host form: status")
    assert (status == 3).mean() > 0.5   # not a comparison of fallbacks: most pixels pass on both sides


@pytest.mark.parametrize("factor", [2, 4])
def test_python_wrapper_interleaves_in_time_order(factor):
    import lucas_kanade_pyramidal as P

    T, H, W = 3, 37, 53
    n = factor - 1
    for u8 in (False, True):
        frames = _video(T, H, W, seed=factor, u8=u8)
        r = P.lucas_kanade_pyramidal_sequence_interpolate(list(frames), factor=factor)
        assert r.frames.shape == ((T - 1) * n + T, H, W) and r.frames.dtype == frames.dtype
        assert r.new.shape == r.status.shape == (T - 1, n, H, W) and r.new.dtype == frames.dtype and r.status.dtype == np.uint8
        for t in range(T):
            _same(r.frames[t * factor], frames[t], f"original {t}")
        for t in range(T - 1):
            for j in range(n):
                _same(r.frames[t * factor + 1 + j], r.new[t, j], f"new frame {t}, {j}")
        explicit = P.lucas_kanade_pyramidal_sequence_interpolate(frames, factor=9, taus=[(j + 1) / factor for j in range(n)])
        _same(explicit.frames, r.frames, "explicit taus")


def test_device_form_replays_from_a_graph():
    """one eager call, then the same call captured on a side stream: replays give the eager bytes"""
    import torch

    import _oflk

    B, H, W = 2, 96, 128
    frames, _ = FM.occluder_scene(T=B + 1)
    flows = _wild_flows(B, H, W, seed=1)
    for k in range(4):
        flows[k][:, :, ::2] *= 0.01
    taus = TAUS[:3]
    for u8 in (False, True):
        fr = np.rint(frames).astype(np.uint8) if u8 else frames
        eager = _device(fr, flows, taus)
        want = M.interpolate(fr, *flows, taus)
        _same(eager[0], want[0], "eager frames")
        _same(eager[1], want[1], "eager status")
        d_fr, d = _dev(fr), [_dev(f) for f in flows]
        out = torch.zeros((B, len(taus), H, W), dtype=d_fr.dtype, device=d_fr.device)
        st = torch.zeros((B, len(taus), H, W), dtype=torch.uint8, device=d_fr.device)
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            _oflk.interpolate_frames(d_fr.data_ptr(), B, H, W, *(x.data_ptr() for x in d), taus, out.data_ptr(), st.data_ptr(), u8=u8,
                                     stream=torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            out.zero_()
            st.zero_()
            g.replay()
            torch.cuda.synchronize()
            _same(out.cpu().numpy(), eager[0], f"replay {rep} frames")
            _same(st.cpu().numpy(), eager[1], f"replay {rep} status")
        del g
