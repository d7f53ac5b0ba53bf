"""GPU tests of frame interpolation on colour and NV12 video (run on an MI355X: python -m pytest
tests/test_gpu_interp_colour.py -m gpu -q).

oflk_interpolate_frames_packed, oflk_interpolate_frames_nv12 and their host forms must equal the NumPy statement of
tests/interp_colour_model.py byte for byte, frames and status, on every shape form, on flows that throw points out of the frame
and on flows with NaN, infinities and 1e30 planted in them; every packed channel and the Y plane must also equal the existing
grey device call.  The sequence calls must equal the chain of existing calls that include/oflk.h names.
"""
import numpy as np
import pytest

import fb_model as FM
import interp_colour_model as CM
import interp_model as M
import nv12_model as NM
from test_gpu_fb import _host_fb, _same
from test_gpu_interp import CONFIGS, SHAPES, TAUS, _device, _planted_flows, _wild_flows
from test_gpu_sequence import _dev, _video

pytestmark = pytest.mark.gpu

NV12_SHAPES = [(4, 4), (4, 6), (6, 4), (38, 54)] + [(h, w) for h in (6, 8, 10) for w in (126, 128, 130)]


def _layout(kind, arg):
    import _oflk

    return _oflk.FrameLayout("_" + kind, (arg,))


def _offset_tensor(shape, fill, misalign):
    """a uint8 device tensor of `shape`; with misalign its first byte lies 1 byte behind a 256-byte boundary"""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 512,), fill, dtype=torch.uint8, device=torch.device("cuda", 0))
    off = (-buf.data_ptr()) % 256 + (1 if misalign else 0)
    view = buf[off:off + n].view(*shape)
    assert view.data_ptr() % 256 == (1 if misalign else 0)
    return view


def _device_layout(kind, arg, frames, flows, taus, alpha=0.01, beta=0.5, refine=2, status=True, misalign=False):
    """the device form on torch tensors: (new, status or None); an output that was not asked for must stay as it was"""
    import torch

    import _oflk

    B, H, W = flows[0].shape
    n = len(taus)
    d_fr = _offset_tensor(frames.shape, 0, misalign)
    d_fr.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
    d = [_dev(f) for f in flows]
    out = _offset_tensor((B, n) + frames.shape[1:], 77, misalign)
    st = _offset_tensor((B, n, H, W), 9, misalign)
    _oflk.interpolate_frames_layout(_layout(kind, arg), d_fr.data_ptr(), B, H, W, *(x.data_ptr() for x in d), taus, out.data_ptr(),
                                    st.data_ptr() if status else 0, alpha, beta, refine, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if not status:
        assert (st == 9).all()
    return out.cpu().numpy(), st.cpu().numpy() if status else None


def _host_layout(kind, arg, frames, flows, taus, alpha, beta, refine, status):
    import lucas_kanade_pyramidal as P

    if kind == "packed":
        return P.interpolate_frames(frames, *flows, taus=taus, alpha=alpha, beta=beta, refine=refine, return_status=status)
    return P.interpolate_frames_nv12(frames, *flows, taus=taus, siting=arg, alpha=alpha, beta=beta, refine=refine, return_status=status)


def _model(kind, arg, frames, flows, taus, alpha=0.01, beta=0.5, refine=2):
    if kind == "packed":
        return CM.interpolate_packed(frames, *flows, taus, alpha, beta, refine)
    return CM.interpolate_nv12(frames, *flows, taus, arg, alpha, beta, refine)


def _check_all_forms(kind, arg, frames, flows, taus, refine, status, what):
    """the device form and the host form against the statement, and the planes that the grey call covers against the
    existing grey device call; returns the statement's (new, status)"""
    want = _model(kind, arg, frames, flows, taus, refine=refine)
    code = NM.SITING_CODES[arg] if kind == "nv12" else arg
    got = _device_layout(kind, code, frames, flows, taus, refine=refine, status=status)
    _same(got[0], want[0], f"{what}: device frames")
    if status:
        _same(got[1], want[1], f"{what}: device status")
    host = _host_layout(kind, arg, frames, flows, taus, 0.01, 0.5, refine, status)
    _same(host[0] if status else host, want[0], f"{what}: host frames")
    if status:
        _same(host[1], want[1], f"{what}: host status")
    H = flows[0].shape[1]
    planes = [np.ascontiguousarray(frames[..., c]) for c in range(arg)] if kind == "packed" else [np.ascontiguousarray(frames[:, :H])]
    for c, plane in enumerate(planes):
        grey = _device(plane, flows, taus, refine=refine, status=status)
        _same(got[0][..., c] if kind == "packed" else got[0][:, :, :H], grey[0], f"{what}: plane {c} vs the grey device call")
        if status:
            _same(got[1], grey[1], f"{what}: status vs the grey device call")
    return want


def _colour(F, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W, C), dtype=np.uint8)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda s: str(s))
def test_packed_kernel_equals_statement(H, W, C):
    """frames of one row or one column are refused, as every packed call refuses them (a tap is a dword of its frame):
    there the device and the host form must answer OFLK_ERR_INVALID and write nothing"""
    import _oflk

    codes = set()
    for i, (B, taus, refine, status) in enumerate(CONFIGS):
        frames = _colour(B + 1, H, W, C, seed=H * 100 + W + i)
        for kind, make in (("wild", _wild_flows), ("planted", _planted_flows)):
            flows = make(B, H, W, seed=H * 7 + W + i)
            if H < 2 or W < 2:
                for form in (lambda: _device_layout("packed", C, frames, flows, taus, refine=refine, status=False),
                             lambda: _host_layout("packed", C, frames, flows, taus, 0.01, 0.5, refine, status)):
                    with pytest.raises((_oflk.OflkError, ValueError), match="H and W must be >= 2|at least 2 x 2"):
                        form()
                continue
            want = _check_all_forms("packed", C, frames, flows, taus, refine, status, f"{H}x{W}x{C} {kind} config {i}")
            codes |= set(np.unique(want[1]).tolist())
    if H * W > 100:
        assert codes == {0, 1, 2, 3}


@pytest.mark.parametrize("siting", ["left", "center"])
@pytest.mark.parametrize("H,W", NV12_SHAPES, ids=lambda s: str(s))
def test_nv12_kernel_equals_statement(H, W, siting):
    codes = set()
    for i, (B, taus, refine, status) in enumerate(CONFIGS):
        frames = NM.random_frames(B + 1, H, W, seed=H * 100 + W + i)
        for kind, make in (("wild", _wild_flows), ("planted", _planted_flows)):
            flows = make(B, H, W, seed=H * 7 + W + i)
            want = _check_all_forms("nv12", siting, frames, flows, taus, refine, status, f"{H}x{W} {siting} {kind} config {i}")
            codes |= set(np.unique(want[1]).tolist())
    if H * W > 100:
        assert codes == {0, 1, 2, 3}


@pytest.mark.parametrize("kind,arg,H,W", [("packed", 4, 37, 52), ("packed", 3, 37, 53), ("nv12", 0, 38, 54), ("nv12", 1, 8, 128)])
def test_arrays_one_byte_off_a_256_byte_boundary_give_the_same_bytes(kind, arg, H, W):
    """the packed C = 4 lane stores a dword and an NV12 chroma lane 2 bytes where the output is aligned: frames, out and
    status 1 byte behind a 256-byte boundary take the byte-wise stores and must give the aligned call's bytes"""
    B, taus = 2, TAUS[:3]
    frames = _colour(B + 1, H, W, arg, seed=1) if kind == "packed" else NM.random_frames(B + 1, H, W, seed=1)
    flows = _wild_flows(B, H, W, seed=2)
    for k in range(4):
        flows[k][:, :, ::2] *= 0.01
    want = _model(kind, "center" if arg else "left", frames, flows, taus) if kind == "nv12" else _model(kind, arg, frames, flows, taus)
    for misalign in (False, True):
        got = _device_layout(kind, arg, frames, flows, taus, misalign=misalign)
        _same(got[0], want[0], f"misalign={misalign}: frames")
        _same(got[1], want[1], f"misalign={misalign}: status")


@pytest.mark.parametrize("kind,arg,H,W", [("packed", 3, 2, 3), ("nv12", 0, 4, 4)])
def test_more_slices_than_the_grid_z_limit(kind, arg, H, W):
    """B = 4100 pairs at n = 16: 65600 slices, cut at 65535.  Frames and flows repeat with period 7 (7 divides neither 16 nor
    65535), so the statement is evaluated on 7 pairs; a slice given another pair's data or time shows"""
    B, P_ = 4100, 7
    taus = TAUS + list(np.linspace(0.05, 0.95, 11))
    base = _colour(P_, H, W, arg, seed=5) if kind == "packed" else NM.random_frames(P_, H, W, seed=5)
    fbase = _planted_flows(P_, H, W, seed=7)
    for k in range(4):
        fbase[k][::3] = _wild_flows(P_, H, W, seed=6)[k][::3]
        fbase[k][1] *= np.float32(0.125)   # a pair whose points stay inside
    want = _model(kind, "left" if kind == "nv12" else arg, np.concatenate([base, base[:1]]), fbase, taus)
    frames = base[np.arange(B + 1) % P_]
    flows = [f[np.arange(B) % P_] for f in fbase]
    got = _device_layout(kind, arg, frames, flows, taus)
    idx = np.arange(B) % P_
    _same(got[0], want[0][idx], "z limit: frames")
    _same(got[1], want[1][idx], "z limit: status")


def _colour_video(T, H, W, C, seed):
    return np.ascontiguousarray(np.stack([_video(T, H, W, seed=seed + c, u8=True) for c in range(C)], axis=-1))


def _nv12_video(T, H, W, seed):
    return NM.from_grey(_video(T, H, W, seed=seed, u8=True))


def _sequence_and_chain(kind, frames, arg, taus=None, factor=2):
    """(the sequence call's result and resolved count, the chain's (new, status) and its fb call's resolved count)"""
    import _oflk
    import lucas_kanade_pyramidal as P

    if kind == "packed":
        r = P.lucas_kanade_pyramidal_sequence_interpolate(frames, factor=factor, taus=taus, order=arg)
        n_seq = int(_oflk.lib().oflk_last_resolved())
        grey = _oflk.luma_host(frames, _oflk.COLOUR_ORDERS[arg])
    else:
        r = P.lucas_kanade_pyramidal_sequence_interpolate_nv12(frames, factor=factor, taus=taus, siting=arg)
        n_seq = int(_oflk.lib().oflk_last_resolved())
        grey = np.ascontiguousarray(NM.planes(frames)[0])
    fb, n_fb = _host_fb(grey, 3, 5, 3)
    cfg_taus = r.new.shape[1]
    taus = taus if taus is not None else [(j + 1) / factor for j in range(cfg_taus)]
    chain = _host_layout(kind, arg if kind == "nv12" else frames.shape[-1], frames, fb[:4], taus, 0.01, 0.5, 2, True)
    return r, n_seq, chain, n_fb, fb


@pytest.mark.parametrize("kind,arg,C", [("packed", "rgb", 3), ("packed", "bgr", 3), ("packed", "rgb", 4), ("packed", "bgr", 4),
                                        ("nv12", "left", 0), ("nv12", "center", 0)])
def test_sequence_equals_the_chain_of_existing_calls(kind, arg, C):
    import _oflk

    T, H, W = 4, 64, 80
    frames = _colour_video(T, H, W, C, seed=3) if kind == "packed" else _nv12_video(T, H, W, seed=3)
    taus = [0.25, 0.5, 0.75]
    for arith in (0, 2):
        _oflk.check(_oflk.lib().oflk_set_host_arithmetic(arith))
        try:
            r, n_seq, chain, n_fb, fb = _sequence_and_chain(kind, frames, arg, taus)
        finally:
            _oflk.check(_oflk.lib().oflk_set_host_arithmetic(0))
        assert n_seq == n_fb
        _same(r.new, chain[0], f"arith {arith}: new frames")
        _same(r.status, chain[1], f"arith {arith}: status")
        if arith == 0:
            want = _model(kind, arg if kind == "nv12" else C, frames, fb[:4], taus)
            _same(r.new, want[0], "statement: frames")
            _same(r.status, want[1], "statement: status")
            assert (r.status == 3).mean() > 0.5   # not a comparison of fallbacks: most pixels pass on both sides


@pytest.mark.parametrize("kind,arg,C", [("packed", "rgb", 3), ("nv12", "left", 0)])
def test_chunked_1080p_equals_host_form_on_the_downloaded_flows(kind, arg, C):
    """T = 18 at 1080p: the chunk rule (chunk_pairs) cuts the 17 pairs into chunks of 4, 4, 4, 4 and 1"""
    T, H, W = 18, 1080, 1920
    grey = _video(T, H, W, seed=4, u8=True)
    if kind == "packed":   # three channels that differ, from one scene: the luma keeps its texture
        frames = np.ascontiguousarray(np.stack([grey, grey // 2 + 40, 255 - grey], axis=-1))
    else:
        frames = NM.from_grey(grey)
    r, n_seq, chain, n_fb, _ = _sequence_and_chain(kind, frames, arg)
    assert n_seq == n_fb
    _same(r.new, chain[0], "1080p pipeline vs host form: frames")
    _same(r.status, chain[1], "1080p pipeline vs host form: status")
    assert (r.status == 3).mean() > 0.5


@pytest.mark.parametrize("factor", [2, 4])
def test_python_wrappers_interleave_in_time_order(factor):
    import lucas_kanade_pyramidal as P

    T, H, W = 3, 38, 54
    n = factor - 1
    cases = [(_colour_video(T, H, W, 3, seed=factor), (H, W, 3), lambda f, **kw: P.lucas_kanade_pyramidal_sequence_interpolate(f, **kw)),
             (_colour_video(T, H, W, 4, seed=factor), (H, W, 4), lambda f, **kw: P.lucas_kanade_pyramidal_sequence_interpolate(f, order="bgr", **kw)),
             (_nv12_video(T, H, W, seed=factor), (3 * H // 2, W), lambda f, **kw: P.lucas_kanade_pyramidal_sequence_interpolate_nv12(f, siting="center", **kw))]
    for frames, shape, call in cases:
        r = call(frames, factor=factor)
        assert r.frames.shape == ((T - 1) * n + T,) + shape and r.frames.dtype == np.uint8
        assert r.new.shape == (T - 1, n) + shape and r.new.dtype == np.uint8
        assert r.status.shape == (T - 1, n, H, W) and r.status.dtype == np.uint8
        for t in range(T):
            _same(r.frames[t * factor], frames[t], f"original {t}")
        for t in range(T - 1):
            for j in range(n):
                _same(r.frames[t * factor + 1 + j], r.new[t, j], f"new frame {t}, {j}")
        explicit = call(frames, factor=9, taus=[(j + 1) / factor for j in range(n)])
        _same(explicit.frames, r.frames, "explicit taus")


@pytest.mark.parametrize("kind,arg", [("packed", 3), ("packed", 4), ("nv12", 0), ("nv12", 1)])
def test_device_forms_replay_from_a_graph(kind, arg):
    """one eager call, then the same call captured on a side stream: replays give the eager bytes"""
    import torch

    import _oflk

    B, H, W = 2, 96, 128
    grey, _ = FM.occluder_scene(T=B + 1)
    grey = np.rint(grey).astype(np.uint8)
    frames = np.ascontiguousarray(np.stack([grey, 255 - grey, grey // 2, grey][:arg], axis=-1)) if kind == "packed" else NM.from_grey(grey)
    flows = _wild_flows(B, H, W, seed=1)
    for k in range(4):
        flows[k][:, :, ::2] *= 0.01
    taus = TAUS[:3]
    eager = _device_layout(kind, arg, frames, flows, taus)
    want = _model(kind, ("left", "center")[arg] if kind == "nv12" else arg, frames, flows, taus)
    _same(eager[0], want[0], "eager frames")
    _same(eager[1], want[1], "eager status")
    d_fr, d = _dev(frames), [_dev(f) for f in flows]
    out = torch.zeros((B, len(taus)) + frames.shape[1:], dtype=torch.uint8, device=d_fr.device)
    st = torch.zeros((B, len(taus), H, W), dtype=torch.uint8, device=d_fr.device)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _oflk.interpolate_frames_layout(_layout(kind, arg), d_fr.data_ptr(), B, H, W, *(x.data_ptr() for x in d), taus, out.data_ptr(),
                                        st.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        out.zero_()
        st.zero_()
        g.replay()
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), eager[0], f"replay {rep} frames")
        _same(st.cpu().numpy(), eager[1], f"replay {rep} status")
    del g
