"""GPU tests of the median filter of dense flows (run on an MI355X: python -m pytest tests/test_gpu_flow_median.py -m gpu -q).

oflk_flow_median and its host form must equal the NumPy statement of tests/flow_median_model.py byte for byte, a NaN equal to
a NaN, at every size, on the shapes at which a tiled median can go wrong, on heavy ties and on planes seeded with NaNs of both
signs, infinities and zeros of both signs.  The _median sequence calls must equal the unfiltered call's flows put through the
host form and then through the host forms of what follows.
"""
import numpy as np
import pytest

import flow_median_model as FMM
import nv12_model as NM
from test_gpu_fb import _host_fb, _same
from test_gpu_interp_colour import _colour_video, _nv12_video
from test_gpu_sequence import _dev, _video

pytestmark = pytest.mark.gpu

SIZES = FMM.SIZES


def _tile():
    import _oflk

    return _oflk.flow_median_tile()   # (rows, columns) of a block's output pixels: the kernel's constants


def _shapes():
    """smaller than every halo, one below / on / one above the tile, two tiles plus one"""
    th, tw = _tile()
    return [(1, 1), (1, 5), (3, 2), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 1, 2 * tw + 1)]


def _device(planes, size):
    import torch

    import _oflk

    P, H, W = planes.shape
    d_in = _dev(planes)
    out = torch.full((P, H, W), 77.0, dtype=torch.float32, device=d_in.device)
    _oflk.flow_median(d_in.data_ptr(), out.data_ptr(), P, H, W, size, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(d_in.cpu().numpy(), planes, "the input is left as it was")
    return out.cpu().numpy()


def _planes(kind, P, H, W, seed):
    if kind == "random":
        return ((np.random.default_rng(seed).random((P, H, W)) * 2 - 1) * 4).astype(np.float32)
    return FMM.quantised_planes(P, H, W, seed) if kind == "ties" else FMM.special_planes(P, H, W, seed)


@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_statement(size):
    import lucas_kanade_pyramidal as P_

    assert _tile()[0] * _tile()[1] == 256
    for H, W in _shapes():
        for i, (kind, P) in enumerate((("random", 2), ("ties", 1), ("specials", 5), ("ties", 2), ("specials", 1))):
            planes = _planes(kind, P, H, W, seed=H * 100 + W + size + i)
            want = FMM.median(planes, size)
            _same(_device(planes, size), want, f"{size} x {size} on {P} x {H} x {W} {kind}: device")
            _same(P_.median_filter_flow(planes, size), want, f"{size} x {size} on {P} x {H} x {W} {kind}: host")


def test_more_planes_than_the_grid_z_limit():
    """65540 planes of 4 x 4, cut at 65535.  The planes repeat with period 7 (7 does not divide 65535), so the statement is
    evaluated on 7 planes; a plane given another plane's data shows"""
    P, H, W, period = 65540, 4, 4, 7
    base = np.concatenate([FMM.special_planes(3, H, W, seed=1), _planes("random", 4, H, W, seed=2)])
    idx = np.arange(P) % period
    planes = np.ascontiguousarray(base[idx])
    for size in (3, 9):
        _same(_device(planes, size), FMM.median(base, size)[idx], f"z limit, size {size}")


def test_host_form_does_not_depend_on_its_chunks():
    """a chunk is min(64, 2^27 / (4 H W)) planes.  70 planes of 5 x 9 go as 64 + 6; 17 planes of 1080p as 16 + 1, and equal
    the device form, which has them in one launch"""
    import lucas_kanade_pyramidal as P_

    planes = np.concatenate([FMM.special_planes(35, 5, 9, seed=3), _planes("random", 35, 5, 9, seed=4)])
    for size in (3, 7):
        whole = P_.median_filter_flow(planes, size)
        _same(whole, FMM.median(planes, size), f"70 planes, size {size}: statement")
        _same(whole, np.concatenate([P_.median_filter_flow(planes[:64], size), P_.median_filter_flow(planes[64:], size)]),
              f"70 planes, size {size}: the chunks on their own")
    H, W = 1080, 1920
    small = _planes("random", 17, 27, 40, seed=5)
    big = np.ascontiguousarray(np.tile(small, (1, H // 27, W // 40)))
    assert big.shape == (17, H, W)
    whole = P_.median_filter_flow(big, 3)
    _same(whole, _device(big, 3), "17 planes of 1080p: host against device")
    _same(whole[16], P_.median_filter_flow(big[16], 3), "17 planes of 1080p: the last chunk on its own")
    _same(whole[3, :60, :90], FMM.median_plane(big[3, :64, :94], 3)[:60, :90], "17 planes of 1080p: a corner against the statement")


def _fb_host(flows, alpha=0.01, beta=0.5):
    import _oflk

    B, H, W = flows[0].shape
    err = [np.empty((B, H, W), np.float32) for _ in range(2)]
    valid = [np.empty((B, H, W), np.uint8) for _ in range(2)]
    _oflk.check(_oflk.lib().oflk_fb_consistency_host(*(_oflk.ptr(f) for f in flows), B, H, W, alpha, beta, _oflk.ptr(err[0]),
                                                     _oflk.ptr(err[1]), valid[0].ctypes.data, valid[1].ctypes.data))
    return err, valid


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_fb_sequence_equals_fb_then_median_then_check(u8):
    import _oflk
    import lucas_kanade_pyramidal as P_

    T, H, W = 4, 64, 80
    frames = _video(T, H, W, seed=3, u8=u8)
    for arith, sizes in ((0, SIZES), (2, (5,))):
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
        try:
            fb, n_fb = _host_fb(frames, 3, 5, 3)
            got = {}
            for k in sizes:
                got[k] = (P_.lucas_kanade_pyramidal_sequence_fb(frames, flow_median=k), int(_oflk.lib().oflk_last_resolved()))
        finally:
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
        for k, (r, n_seq) in got.items():
            assert n_seq == n_fb
            flows = [P_.median_filter_flow(f, k) for f in fb[:4]]
            err, valid = _fb_host(flows)
            for name, a, b in zip(r._fields, r, flows + err + [v.astype(bool) for v in valid]):
                _same(a, b, f"arith {arith}, median {k}: {name}")
            if arith == 0:
                _same(flows[0], FMM.median(fb[0], k), f"median {k}: the host form against the statement")
                assert any((f != g).any() for f, g in zip(flows, fb[:4]))   # the filter changed something
                assert r.valid_fwd.mean() > 0.5                           # not a comparison of empty masks


def _chain(kind, frames, k, taus, arg=None):
    """(the _median sequence call's result, (new, status) of the unfiltered flows filtered and interpolated by the host forms)"""
    import _oflk
    import lucas_kanade_pyramidal as P_

    if kind == "grey":
        r = P_.lucas_kanade_pyramidal_sequence_interpolate(frames, taus=taus, flow_median=k)
        grey = frames
    elif kind == "packed":
        r = P_.lucas_kanade_pyramidal_sequence_interpolate(frames, taus=taus, order=arg, flow_median=k)
        grey = _oflk.luma_host(frames, _oflk.COLOUR_ORDERS[arg])
    else:
        r = P_.lucas_kanade_pyramidal_sequence_interpolate_nv12(frames, taus=taus, siting=arg, flow_median=k)
        grey = np.ascontiguousarray(NM.planes(frames)[0])
    n_seq = int(_oflk.lib().oflk_last_resolved())
    fb, n_fb = _host_fb(grey, 3, 5, 3)
    assert n_seq == n_fb
    flows = [P_.median_filter_flow(f, k) if k else f for f in fb[:4]]
    if kind == "nv12":
        return r, P_.interpolate_frames_nv12(frames, *flows, taus=taus, siting=arg, return_status=True)
    return r, P_.interpolate_frames(frames, *flows, taus=taus, return_status=True)


@pytest.mark.parametrize("kind,arg", [("grey", "f32"), ("grey", "u8"), ("packed", "bgr"), ("nv12", "center")])
def test_interpolation_sequence_equals_the_chain_on_filtered_flows(kind, arg):
    T, H, W = 4, 64, 80
    if kind == "grey":
        frames = _video(T, H, W, seed=3, u8=arg == "u8")
    else:
        frames = _colour_video(T, H, W, 3, seed=3) if kind == "packed" else _nv12_video(T, H, W, seed=3)
    taus = [0.25, 0.5, 0.75]
    plain, _ = _chain(kind, frames, 0, taus, arg)
    for k in (5, 9):
        r, (new, status) = _chain(kind, frames, k, taus, arg)
        _same(r.new, new, f"{kind} {arg}, median {k}: new frames")
        _same(r.status, status, f"{kind} {arg}, median {k}: status")
        assert (r.status != plain.status).any()   # the filter reached the interpolation
        assert (status == 3).mean() > 0.5         # not a comparison of fallbacks


def test_chunked_1080p_equals_the_chain_on_filtered_flows():
    """T = 18 at 1080p: the chunk rule (chunk_pairs) cuts the 17 pairs into chunks of 4, 4, 4, 4 and 1, each filtered through
    the one spare buffer"""
    frames = _video(18, 1080, 1920, seed=4, u8=True)
    r, (new, status) = _chain("grey", frames, 5, [0.5])
    _same(r.new, new, "1080p: new frames")
    _same(r.status, status, "1080p: status")
    assert (status == 3).mean() > 0.5


def test_flow_median_0_is_the_call_without_the_keyword():
    import lucas_kanade_pyramidal as P_

    T, H, W = 4, 64, 80
    for u8 in (False, True):
        frames = _video(T, H, W, seed=5, u8=u8)
        a, b = P_.lucas_kanade_pyramidal_sequence_fb(frames), P_.lucas_kanade_pyramidal_sequence_fb(frames, flow_median=0)
        for name, x, y in zip(a._fields, a, b):
            _same(x, y, f"fb u8={u8}: {name}")
        a = P_.lucas_kanade_pyramidal_sequence_interpolate(frames, factor=3)
        b = P_.lucas_kanade_pyramidal_sequence_interpolate(frames, factor=3, flow_median=0)
        for name, x, y in zip(a._fields, a, b):
            _same(x, y, f"interpolate u8={u8}: {name}")


def test_device_form_replays_from_a_graph():
    """one eager call, then the same call captured on a side stream: replays give the eager bytes"""
    import torch

    import _oflk

    th, tw = _tile()
    P, H, W = 3, 3 * th + 2, 2 * tw + 5
    planes = np.concatenate([FMM.special_planes(1, H, W, seed=6), _planes("random", 2, H, W, seed=7)])
    for size in SIZES:
        eager = _device(planes, size)
        _same(eager, FMM.median(planes, size), f"size {size}: eager")
        d_in = _dev(planes)
        out = torch.zeros((P, H, W), dtype=torch.float32, device=d_in.device)
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            _oflk.flow_median(d_in.data_ptr(), out.data_ptr(), P, H, W, size, stream=torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            _same(out.cpu().numpy(), eager, f"size {size}: replay {rep}")
        del g
