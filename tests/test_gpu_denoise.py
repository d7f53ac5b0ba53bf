"""GPU tests of temporal denoising (run on an MI355X: python -m pytest tests/test_gpu_denoise.py -m gpu -q).

oflk_denoise_frames_host must equal the NumPy statement of tests/denoise_model.py byte for byte, out and count, float32 and
uint8, at every radius, on shapes around the kernel's 64 x 4 block, on sequences short enough that chains end at both ends, on
flows that leave the frame and on flows and pixels with NaN and infinities planted in them.  oflk_denoise_sequence must equal
oflk_pyramidal_sequence_fb_median followed by the host form, whatever the chunk cut.
"""
import functools

import numpy as np
import pytest

import denoise_model as M
from test_gpu_fb import _same
from test_gpu_sequence import _video

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (5, 7), (4, 64), (9, 65), (33, 130)]   # around the block of 4 rows x 64 columns
RADII = [1, 2, 3, 4]
BAD = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)


def _frame_counts(R):
    return [2, 2 * R, 2 * R + 1, 2 * R + 3]


def _frames(T, H, W, seed, u8, planted=True):
    """random frames that keep some likeness from frame to frame (so that weights of every size occur); float32 frames carry
    a few NaN, infinities and zeros of both signs"""
    rng = np.random.default_rng(seed)
    f = rng.random((1, H, W)) * 255.0 + rng.normal(0.0, 25.0, (T, H, W))
    if u8:
        return np.rint(np.clip(f, 0, 255)).astype(np.uint8)
    f = f.astype(np.float32)
    if planted:
        idx = rng.choice(f.size, size=min(7, f.size // 2), replace=False)
        f.reshape(-1)[idx] = rng.permutation(np.concatenate([BAD[:3], np.array([0.0, -0.0, 0.0, -0.0], np.float32)]))[:len(idx)]
    return f


def _flows(B, H, W, seed, planted=True):
    """per pair one forward vector of up to 2.5 px (an eighth of the axis at most) with a jitter of 0.3 px a pixel, and backward
    flows that undo the vector with a jitter of their own, so that most steps pass the test and some do not; 2 % of the values
    wild (up to 2 W px: they leave the frame or fail the test), and NaN, infinities and 1e30 at a few pixels of every plane"""
    rng = np.random.default_rng(seed)
    amp = np.array([min(2.5, (W - 1) / 8), min(2.5, (H - 1) / 8)]).reshape(2, 1, 1, 1)
    vec = (rng.random((2, B, 1, 1)) * 2 - 1) * amp
    f = np.concatenate([vec, -vec]) + (rng.random((4, B, H, W)) * 2 - 1) * 0.3
    wild = rng.random((4, B, H, W)) < 0.02
    f[wild] = ((rng.random((4, B, H, W)) * 2 - 1) * 2 * W)[wild]
    f = f.astype(np.float32)
    for p in range(4 if planted else 0):
        idx = rng.choice(B * H * W, size=min(3, B * H * W // 2), replace=False)
        f[p].reshape(-1)[idx] = rng.permutation(BAD)[:len(idx)]
    return [np.ascontiguousarray(a) for a in f]


def _check(frames, flows, R, what, strength=60.0, alpha=0.01, beta=4.0, count=True):
    """the host form against the statement; returns the statement's (out, count)"""
    import lucas_kanade_pyramidal as P

    want = M.denoise(frames, *flows, strength, R, alpha, beta)
    got = P.denoise_frames(frames, *flows, strength, R, alpha, beta, return_count=count)
    _same(got[0] if count else got, want[0], f"{what}: frames")
    if count:
        _same(got[1], want[1], f"{what}: count")
    return want


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda s: str(s))
def test_host_form_equals_statement(H, W, u8):
    seen = {R: set() for R in RADII}
    for R in RADII:
        for i, T in enumerate(_frame_counts(R)):
            frames = _frames(T, H, W, seed=H * 100 + W + 10 * R + i, u8=u8)
            flows = _flows(T - 1, H, W, seed=H * 7 + W + 10 * R + i)
            alpha, beta = ((0.01, 4.0), (0.05, 0.5))[i % 2]
            want = _check(frames, flows, R, f"{H}x{W} R={R} T={T}", alpha=alpha, beta=beta, count=i != 1)
            seen[R] |= set(np.unique(want[1]).tolist())
    if H * W > 500:   # chains of every length: ended at once, ended on the way, and run to the end on both sides
        for R in RADII:
            assert seen[R] == set(range(2 * R + 1)), (R, seen[R])


def test_signed_zeros_come_out_as_the_statement_has_them():
    """frames of +0 and -0 only and flows that are +0, -0 or whole pixels: a centre of -0 with no neighbour stays -0, any
    neighbour makes it +0 (a sample's sum starts at +0), and the kernel agrees bit for bit"""
    rng = np.random.default_rng(3)
    T, H, W = 5, 6, 70
    frames = np.where(rng.random((T, H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    flows = [np.where(rng.random((T - 1, H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32) for _ in range(4)]
    flows[0][:, :, ::5], flows[2][:, :, ::5] = 1.0, -1.0
    flows[1][:2], flows[3][:2] = np.float32(300.0), np.float32(-300.0)   # pairs 0 and 1 throw every point out: chains end there
    for R in (1, 2):
        want = _check(frames, flows, R, f"signed zeros R={R}", strength=1.0)
        signs = np.signbit(want[0])
        assert signs.any() and (~signs).any() and (want[0] == 0).all()
        assert not signs[want[1] > 0].any()


def test_more_frames_than_the_grid_z_limit():
    """T = 65540 frames of 2 x 3: 65540 slices, cut at 65535.  Frames and flows repeat with period 7 (7 does not divide 65535),
    so the statement is evaluated on the first and the last 28 frames: an inner frame equals the inner frame of the same
    phase, and a slice given another frame's data, or ends of the sequence that are not its own, shows"""
    import lucas_kanade_pyramidal as P

    T, H, W, P_, L, R = 65540, 2, 3, 7, 28, 4
    fbase = _flows(P_, H, W, seed=7, planted=False)
    for u8 in (False, True):
        base = _frames(P_, H, W, seed=5, u8=u8, planted=False)
        frames = base[np.arange(T) % P_]
        flows = [f[np.arange(T - 1) % P_] for f in fbase]
        out, count = P.denoise_frames(frames, *flows, 60.0, R, return_count=True)
        head = M.denoise(frames[:L], *(f[:L - 1] for f in flows), 60.0, R)
        tail = M.denoise(frames[T - L:], *(f[T - L:] for f in flows), 60.0, R)
        inner = np.arange(R, T - R)
        for got, h, t, name in ((out, head[0], tail[0], "frames"), (count, head[1], tail[1], "count")):
            _same(got[:L - R], h[:L - R], f"z limit u8={u8}: first {name}")
            _same(got[T - L + R:], t[R:], f"z limit u8={u8}: last {name}")
            _same(got[inner], h[R + (inner - R) % P_], f"z limit u8={u8}: inner {name}")
        assert len(np.unique(head[1])) > R   # chains of many lengths


def _fb_median(frames, flow_median, levels=3, window=5, iters=3):
    """oflk_pyramidal_sequence_fb_median[_u8]'s four flows (no errors, no masks) and what it resolved"""
    import _oflk

    T, H, W = frames.shape
    f = np.ascontiguousarray(frames)
    out = [np.empty((T - 1, H, W), np.float32) for _ in range(4)]
    src, fn = _oflk.pixels(f, "oflk_pyramidal_sequence_fb_median")
    _oflk.check(fn(src, T, H, W, levels, window, iters, 0.01, 0.5, flow_median, *(_oflk.ptr(o) for o in out), None, None, None, None))
    return out, int(_oflk.lib().oflk_last_resolved())


@pytest.mark.parametrize("flow_median", [0, 5])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_sequence_equals_fb_median_then_host_form(u8, flow_median):
    import _oflk
    import lucas_kanade_pyramidal as P

    T, H, W = 9, 48, 64
    frames = _video(T, H, W, seed=3, u8=u8)
    for arith in (0, 2):
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
        try:
            flows, n_fb = _fb_median(frames, flow_median)
            got = {R: P.lucas_kanade_pyramidal_sequence_denoise(frames, 12.0, radius=R, flow_median=flow_median, return_count=True)
                   for R in (2, 4)}
            n_seq = int(_oflk.lib().oflk_last_resolved())
        finally:
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
        assert n_seq == n_fb
        for R, (out, count) in got.items():
            want = P.denoise_frames(frames, *flows, 12.0, R, return_count=True)
            _same(out, want[0], f"arith {arith} R={R}: frames")
            _same(count, want[1], f"arith {arith} R={R}: count")
            if arith == 0:
                model = M.denoise(frames, *flows, 12.0, R)
                _same(out, model[0], f"statement R={R}: frames")
                _same(count, model[1], f"statement R={R}: count")
                assert count[R:T - R].mean() > R   # not a comparison of centres alone: most chains run to their end
    assert P.lucas_kanade_pyramidal_sequence_denoise(frames, 12.0, flow_median=flow_median).dtype == frames.dtype


@functools.lru_cache(maxsize=None)
def _video_1080p():
    return _video(18, 1080, 1920, seed=4, u8=True)


@functools.lru_cache(maxsize=None)
def _flows_1080p(T):
    return _fb_median(_video_1080p()[:T], 9)[0]


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("T", [14, 18])
def test_1080p_sequence_equals_host_form_on_the_downloaded_flows(T, R):
    """uint8 frames of 1080p through the 9 x 9 median.  The chunk rule (chunk_pairs) runs the 13 pairs of T = 14 in one piece
    and cuts the 17 pairs of T = 18 into chunks of 4, 4, 4, 4 and 1: there the flows carried from chunk to chunk (2 R pairs)
    are fewer than a chunk's at R = 1 and twice a chunk's at R = 4, and the first frames come out only with the third chunk"""
    import lucas_kanade_pyramidal as P

    frames = _video_1080p()[:T]
    out, count = P.lucas_kanade_pyramidal_sequence_denoise(frames, 12.0, radius=R, return_count=True)
    want = P.denoise_frames(frames, *_flows_1080p(T), 12.0, R, return_count=True)
    _same(out, want[0], f"1080p T={T} R={R}: frames")
    _same(count, want[1], f"1080p T={T} R={R}: count")
    assert count[R:T - R].mean() > R
