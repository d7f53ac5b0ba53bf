"""Writes stay inside the caller's buffers (run on an MI355X: python -m pytest tests/test_gpu_guard_bands.py -m gpu -q).

Every device entry point that writes a caller's array runs here with ALL of its caller-owned arrays -- outputs, workspaces,
state and inputs -- laid out by tests/guard_bands.py as front band | payload | back band, under both band fills, at a
256-aligned base (the vector instantiations) and at bases skewed by one element (the element-wise ones), and with one and
three frames.  After the call every band byte is compared, every input must still hold its bytes, and the values are
asserted against the statement the family already has, so that a call which wrote nothing cannot pass.  Shapes are the
smallest that reach each store path; the table of what is covered is guard_bands.COVERAGE.
"""
import numpy as np
import pytest

import colour_model as CM
import fb_model as FBM
import flow_median_model as FMM
import guard_bands as GB
import homography_model as HM
import interp_colour_model as ICM
import interp_model as IM
import mosaic_exposure_model as MEM
import mosaic_median_model as MMM
import mosaic_model as M
import motion_model as MM
import nv12_model as NM
import stabilize_model as SM

pytestmark = pytest.mark.gpu


def _sync():
    import torch

    torch.cuda.synchronize()


def _runs(*skews):
    """(fill, skew) of every run of a call: both fills at the aligned base and at each skewed one"""
    return [(fill, skew) for skew in (0,) + skews for fill in GB.FILLS]


def _bands(fill, skew):
    return GB.Bands(fill, "cuda:0", skew)


# ---------------------------------------------------------------------------------------------------------------------
# warps: planar float32 and uint8, packed 3 and 4, NV12 with both sitings
# ---------------------------------------------------------------------------------------------------------------------
def _maps6(F, H, W):
    """F affine maps under each of which some pixels are inside and some outside"""
    return np.stack([CM.rotation(H, W, 7.0, 1.1), np.array([1.0, 0, 1.5, 0, 1, -0.5]), CM.rotation(H, W, -20.0, 0.8)])[:F]


def _maps(kind, F, H, W):
    m = _maps6(F, H, W)
    if kind == "affine":
        return m
    return np.stack([CM.as_homography(x) + [0, 0, 0, 0, 0, 0, 2e-3 / W, -1e-3 / H, 0] for x in m])


def _check_warp(call, model, frames, maps, pixel_bytes, row_bytes, inside_shape, skews, what):
    want, want_in = model(frames, maps)
    assert want_in.any() and not want_in.all(), "some pixels inside and some outside"
    for fill, skew in _runs(*skews):
        b = _bands(fill, skew)
        g_in = b.inp("d_frames", frames, row_bytes)
        g_map = b.inp("d_map", maps, skew=0)
        g_out = b.out("d_out", frames.nbytes, row_bytes, pixel_bytes)
        g_ins = b.out("d_inside", want_in.size, inside_shape[-1])
        call(g_in.ptr, g_map.ptr, g_out.ptr, g_ins.ptr)
        _sync()
        b.check(what)
        SM.same(g_out.numpy(frames.dtype, frames.shape), want, f"{what} skew {skew}: out")
        SM.same(g_ins.numpy(np.uint8, inside_shape), want_in, f"{what} skew {skew}: inside")


@pytest.mark.parametrize("H", [5, 6])
@pytest.mark.parametrize("W", [8, 9, 11, 12])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_warp_planar(kind, dtype, W, H):
    import _oflk

    u8 = dtype == np.uint8
    fn = _oflk.warp_affine if kind == "affine" else _oflk.warp_perspective
    model = SM.warp if kind == "affine" else HM.warp
    for F in (1, 3):
        rng = np.random.default_rng(H * W + F)
        frames = rng.integers(0, 256, (F, H, W), dtype=np.uint8) if u8 else (rng.random((F, H, W)) * 255).astype(np.float32)
        maps = _maps(kind, F, H, W)
        _check_warp(lambda i, m, o, s: fn(i, F, H, W, m, o, s, u8), model, frames, maps, frames.itemsize, W * frames.itemsize,
                    (F, H, W), (1, 2) if u8 else (4,), f"warp {kind} planar F={F} {H}x{W}")


@pytest.mark.parametrize("H", [5, 6])
@pytest.mark.parametrize("W", [8, 9, 11, 12])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_warp_packed(kind, C, W, H):
    import _oflk

    fn = _oflk.warp_affine_packed if kind == "affine" else _oflk.warp_perspective_packed
    model = CM.warp_affine if kind == "affine" else CM.warp_perspective
    for F in (1, 3):
        frames = CM.random_frames(F, H, W, C, H * W + F + C)
        _check_warp(lambda i, m, o, s: fn(i, F, H, W, C, m, o, s), model, frames, _maps(kind, F, H, W), 1, W * C, (F, H, W),
                    (1, 2), f"warp {kind} packed C={C} F={F} {H}x{W}")


@pytest.mark.parametrize("H", [4, 6])
@pytest.mark.parametrize("W", [8, 10, 12, 16])
@pytest.mark.parametrize("siting", ["left", "center"])
@pytest.mark.parametrize("kind", ["affine", "perspective"])
def test_warp_nv12(kind, siting, W, H):
    import _oflk

    fn = _oflk.warp_affine_nv12 if kind == "affine" else _oflk.warp_perspective_nv12
    model = NM.warp_affine if kind == "affine" else NM.warp_perspective
    for F in (1, 3):
        frames = NM.random_frames(F, H, W, H * W + F)
        _check_warp(lambda i, m, o, s: fn(i, F, H, W, m, o, s, NM.SITING_CODES[siting]),
                    lambda f, m: model(f, m, siting), frames, _maps(kind, F, H, W), 1, W, (F, H, W), (1, 2),
                    f"warp {kind} nv12 {siting} F={F} {H}x{W}")


# ---------------------------------------------------------------------------------------------------------------------
# luma
# ---------------------------------------------------------------------------------------------------------------------
# k_luma<C, VEC> is chosen by W % 4 == 0 and the alignment of both bases: W = 4 and 8 at the aligned base store dwords, the
# same shapes at skews 1 and 2 and every other width store bytes.  F H W % 4 takes 0, 1 and 3 (a frame has at least two rows)
LUMA_SHAPES = [(1, 2, 4), (3, 3, 4), (1, 5, 8), (3, 2, 8), (1, 2, 6), (1, 3, 3), (3, 3, 5), (1, 3, 5)]


@pytest.mark.parametrize("shape", LUMA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}-W%4={s[2] % 4}-n%4={s[0] * s[1] * s[2] % 4}")
@pytest.mark.parametrize("C", [3, 4])
def test_luma(C, shape):
    import _oflk

    F, H, W = shape
    frames = CM.random_frames(F, H, W, C, sum(shape) + C)
    for order in ("rgb", "bgr"):
        want = CM.luma(frames, order)
        for fill, skew in _runs(1, 2):
            b = _bands(fill, skew)
            g_in = b.inp("d_frames", frames, W * C)
            g_out = b.out("d_luma", F * H * W, W)
            _oflk.luma(g_in.ptr, F, H, W, C, g_out.ptr, CM.ORDERS[order])
            _sync()
            b.check(f"luma C={C} {shape}")
            SM.same(g_out.numpy(np.uint8, (F, H, W)), want, f"luma C={C} {shape} {order} skew {skew}")


# ---------------------------------------------------------------------------------------------------------------------
# the forward-backward check and the flow median
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 5, 8), (3, 5, 9), (1, 6, 11), (3, 17, 66)], ids=lambda v: str(v))
def test_fb_consistency(B, H, W):
    import _oflk
    from test_gpu_fb import _random_flows

    flows = _random_flows(B, H, W, seed=B + H + W)
    want = FBM.fb_check(*flows, 0.01, 0.5)
    masks = [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)]
    names = ("d_err_f", "d_err_b", "d_valid_f", "d_valid_b")
    for mask in masks:
        for fill, skew in _runs(4):
            b = _bands(fill, skew)
            ins = [b.inp(n, f, 4 * W) for n, f in zip(("d_uf", "d_vf", "d_ub", "d_vb"), flows)]
            outs = [b.out(n, B * H * W * (4 if i < 2 else 1), W * (4 if i < 2 else 1), 4 if i < 2 else 1,
                          skew=None if i < 2 else skew // 4) for i, n in enumerate(names)]
            _oflk.fb_consistency(*(g.ptr for g in ins), B, H, W, 0.01, 0.5, *(g.ptr if m else 0 for g, m in zip(outs, mask)))
            _sync()
            b.check(f"fb_consistency {mask}")
            for i, (g, m) in enumerate(zip(outs, mask)):
                if m:
                    SM.same(g.numpy(np.float32 if i < 2 else np.uint8, (B, H, W)), want[i], f"fb_consistency {mask} skew {skew}: {names[i]}")
                else:
                    assert (g.numpy() == GB.PREFILL).all(), f"{names[i]} was not asked for"


def _median_shapes():
    import _oflk

    th, tw = _oflk.flow_median_tile()
    return [(th - 1, tw - 1), (th + 1, tw + 1), (1, 1)]


@pytest.mark.parametrize("size", [3, 9])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["tile-1", "tile+1", "1x1"])
def test_flow_median(which, size):
    import _oflk

    H, W = _median_shapes()[which]
    for P in (1, 3):
        planes = FMM.special_planes(P, H, W, seed=H + W + P)
        want = FMM.median(planes, size)
        for fill, skew in _runs(4):
            b = _bands(fill, skew)
            g_in = b.inp("d_in", planes, 4 * W)
            g_out = b.out("d_out", planes.nbytes, 4 * W, 4)
            _oflk.flow_median(g_in.ptr, g_out.ptr, P, H, W, size)
            _sync()
            b.check(f"flow_median {size} P={P} {H}x{W}")
            SM.same(g_out.numpy(np.float32, planes.shape), want, f"flow_median {size} P={P} {H}x{W} skew {skew}")


# ---------------------------------------------------------------------------------------------------------------------
# frame interpolation: planar, packed, NV12
# ---------------------------------------------------------------------------------------------------------------------
def _interp_flows(B, H, W, seed):
    from test_gpu_interp import _planted_flows, _wild_flows

    f = _planted_flows(B, H, W, seed)
    w = _wild_flows(B, H, W, seed + 1)
    for k in range(4):
        f[k][:, ::3] = w[k][:, ::3]
    return f


def _check_interp(call, model, frames, flows, n, elem, row_bytes, skews, what):
    B, H, W = flows[0].shape
    taus = (np.arange(1, n + 1) / (n + 1.0)).tolist()
    want, want_st = model(frames, *flows, taus)
    for fill, skew in _runs(*skews):
        b = _bands(fill, skew)
        g_fr = b.inp("d_frames", frames, row_bytes)
        g_fl = [b.inp(nm, f, 4 * W) for nm, f in zip(("d_uf", "d_vf", "d_ub", "d_vb"), flows)]
        g_out = b.out("d_out", want.nbytes, row_bytes, elem)
        g_st = b.out("d_status", B * n * H * W, W)
        call(g_fr.ptr, [g.ptr for g in g_fl], taus, g_out.ptr, g_st.ptr)
        _sync()
        b.check(what)
        SM.same(g_out.numpy(want.dtype, want.shape), want, f"{what} skew {skew}: out")
        SM.same(g_st.numpy(np.uint8, (B, n, H, W)), want_st, f"{what} skew {skew}: status")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W", [1, 5, 8])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_interpolate_planar(u8, W, n):
    import _oflk
    from test_gpu_interp import _frames

    for B, H in ((1, 5), (3, 6)):
        frames = _frames(B, H, W, B + H + W, u8)
        flows = _interp_flows(B, H, W, seed=W + n)
        _check_interp(lambda fr, fl, taus, o, s: _oflk.interpolate_frames(fr, B, H, W, *fl, taus, o, s, u8=u8), IM.interpolate, frames,
                      flows, n, frames.itemsize, W * frames.itemsize, (1, 2) if u8 else (4,), f"interpolate planar B={B} n={n} {H}x{W}")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W", [2, 5, 8])   # packed frames are at least 2 x 2: W = 1 is refused
@pytest.mark.parametrize("C", [3, 4])
def test_interpolate_packed(C, W, n):
    import _oflk

    layout = _oflk.FrameLayout("_packed", (C,))
    for B, H in ((1, 5), (3, 6)):
        frames = CM.random_frames(B + 1, H, W, C, B + H + W + C)
        flows = _interp_flows(B, H, W, seed=W + n + C)
        _check_interp(lambda fr, fl, taus, o, s: _oflk.interpolate_frames_layout(layout, fr, B, H, W, *fl, taus, o, s),
                      ICM.interpolate_packed, frames, flows, n, 1, W * C, (1, 2), f"interpolate packed C={C} B={B} n={n} {H}x{W}")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(4, 4), (6, 6), (6, 12)])
@pytest.mark.parametrize("siting", ["left", "center"])
def test_interpolate_nv12(siting, H, W, n):
    import _oflk

    layout = _oflk.FrameLayout("_nv12", (NM.SITING_CODES[siting],))
    for B in (1, 3):
        frames = NM.random_frames(B + 1, H, W, B + H + W)
        flows = _interp_flows(B, H, W, seed=W + n)
        _check_interp(lambda fr, fl, taus, o, s: _oflk.interpolate_frames_layout(layout, fr, B, H, W, *fl, taus, o, s),
                      lambda f, *a: ICM.interpolate_nv12(f, *a, siting), frames, flows, n, 1, W, (1, 2),
                      f"interpolate nv12 {siting} B={B} n={n} {H}x{W}")


# ---------------------------------------------------------------------------------------------------------------------
# trajectories and chains
# ---------------------------------------------------------------------------------------------------------------------
def _spoiled(T, fam, seed):
    from test_gpu_stabilize import _spoil

    model = SM.noisy_models(T - 1, fam, seed)
    counts = np.tile(np.int32([30, 40, 1]), (T - 1, 1))
    return _spoil(model, counts, seed) if T > 2 else (model, counts)


@pytest.mark.parametrize("T", [2, 3, 9])
def test_stabilize_trajectory(T):
    import _oflk

    w = SM.weights(3)
    model, counts = _spoiled(T, MM.AFFINE, T)
    want = SM.trajectory(model, counts, T, w)
    for fill, skew in _runs(4):
        b = _bands(fill, skew)
        g_m, g_c = b.inp("d_model", model), b.inp("d_counts", counts)
        g_corr = b.out("d_correction", T * 24, itemsize=4)
        g_map = b.out("d_map", T * 48, itemsize=8, skew=2 * skew)
        g_held = b.out("d_held", T - 1, skew=skew // 4)
        _oflk.stabilize_trajectory(g_m.ptr, g_c.ptr, T, w, g_corr.ptr, g_map.ptr, g_held.ptr)
        _sync()
        b.check(f"trajectory T={T}")
        SM.same(g_corr.numpy(np.float32, (T, 6)), want[0], f"T={T} skew {skew}: correction")
        SM.same(g_map.numpy(np.float64, (T, 6)), want[1], f"T={T} skew {skew}: map")
        SM.same(g_held.numpy(np.uint8), want[2], f"T={T} skew {skew}: held")


@pytest.mark.parametrize("T", [2, 3, 9])
def test_stabilize_trajectory_ring(T):
    """the ring form on a ring of exactly cap slots that holds the steps in order: the closed stream's T frames"""
    import _oflk

    w = SM.weights(3)
    steps, step_counts = _spoiled(T, MM.SIMILARITY, T + 1)
    want = SM.trajectory(steps, step_counts, T, w)
    cap = max(T - 1, 6)   # cap >= 2 r; the slots past the last step are never read
    model, counts = np.full((cap, 6), np.nan, np.float32), np.zeros((cap, 3), np.int32)
    model[:T - 1], counts[:T - 1] = steps, step_counts
    for n, f0 in ((T, 0), (1, T - 1)):
        for fill, skew in _runs(4):
            b = _bands(fill, skew)
            g_m, g_c = b.inp("d_model_ring", model), b.inp("d_counts_ring", counts)
            g_corr = b.out("d_correction", n * 24, itemsize=4)
            g_map = b.out("d_map", n * 48, itemsize=8, skew=2 * skew)
            _oflk.stabilize_trajectory_ring(g_m.ptr, g_c.ptr, cap, f0, n, T, w, g_corr.ptr, g_map.ptr)
            _sync()
            b.check(f"trajectory ring T={T} n={n}")
            SM.same(g_corr.numpy(np.float32, (n, 6)), want[0][f0:f0 + n], f"T={T} n={n} skew {skew}: correction")
            SM.same(g_map.numpy(np.float64, (n, 6)), want[1][f0:f0 + n], f"T={T} n={n} skew {skew}: map")


@pytest.mark.parametrize("T", [2, 3, 9])
def test_mosaic_chain(T):
    import _oflk
    from test_gpu_mosaic import _chain_scene

    H, W = 120, 160
    model, counts = _chain_scene(T, T)
    for anchor in (0, T - 1):
        want = M.chain(model, counts, T, anchor, H, W, 8.0 * W)
        for fill, skew in _runs(4):
            b = _bands(fill, skew)
            g_m, g_c = b.inp("d_model", np.float32(model).reshape(T - 1, 9)), b.inp("d_counts", np.int32(counts))
            outs = [b.out("d_from_anchor", T * 72, skew=2 * skew), b.out("d_to_anchor", T * 72, skew=2 * skew),
                    b.out("d_box", T * 32, skew=2 * skew), b.out("d_held", T - 1, skew=skew // 4), b.out("d_dropped", T, skew=skew // 4)]
            _oflk.mosaic_chain(g_m.ptr, g_c.ptr, T, anchor, H, W, 8.0 * W, *(g.ptr for g in outs))
            _sync()
            b.check(f"mosaic chain T={T}")
            shapes = [(np.float64, (T, 9)), (np.float64, (T, 9)), (np.float64, (T, 4)), (np.uint8, (T - 1,)), (np.uint8, (T,))]
            for g, (dt, sh), x in zip(outs, shapes, want):
                SM.same(g.numpy(dt, sh), x, f"mosaic chain T={T} anchor {anchor} skew {skew}: {g.name}")


# ---------------------------------------------------------------------------------------------------------------------
# the mosaic: the state at exactly its promised bytes, resolve and median outputs
# ---------------------------------------------------------------------------------------------------------------------
def _mosaic_scene(F, H, W, Hc, Wc, u8, seed):
    rng = np.random.default_rng(seed)
    f = rng.random((F, H, W)) * 255
    frames = np.rint(f).astype(np.uint8) if u8 else f.astype(np.float32)
    maps = np.stack([M.translation(-0.4 * j, 0.3 * j) + [0, 0, 0, 0, 0, 0, 1e-3 * j, 0, 0] for j in range(F)]).astype(np.float64)
    skip = np.zeros(F, np.uint8)
    if F > 2:
        skip[1] = 1
    exposure = np.stack([rng.uniform(0.6, 1.5, F), rng.uniform(-20, 20, F)], 1)
    return frames, maps, skip, exposure


@pytest.mark.parametrize("Hc", [5, 6])
@pytest.mark.parametrize("Wc", [8, 9, 11])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("blend", ["mean", "feather", "first", "last"])
def test_mosaic_accumulate_and_resolve(blend, u8, Wc, Hc):
    import _oflk

    H, W, x0, y0 = 5, 7, -1, -1
    code = M.BLENDS[blend]
    nbytes = _oflk.mosaic_state_bytes(Hc, Wc)
    assert nbytes > 0
    esz = 1 if u8 else 4
    for F in (1, 3):
        frames, maps, skip, exposure = _mosaic_scene(F, H, W, Hc, Wc, u8, Hc * Wc + F)
        for ex in (None, exposure):
            want = M.composite(frames, maps, skip, x0, y0, Hc, Wc, code) if ex is None else \
                MEM.composite(frames, maps, skip, ex, x0, y0, Hc, Wc, code)
            assert want[1].any()
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                b = _bands(fill, skew)
                g_fr, g_map, g_skip = b.inp("d_frames", frames, W * esz), b.inp("d_map", maps, skew=0), b.inp("d_skip", skip)
                g_ex = None if ex is None else b.inp("d_exposure", ex, skew=0)
                g_state = b.out("d_state", nbytes, skew=0)
                g_state.payload.zero_()
                g_out = b.out("d_out", Hc * Wc * esz, Wc * esz, esz)
                g_cnt = b.out("d_count", Hc * Wc * 4, Wc * 4, 4, skew=4 if skew else 0)
                _oflk.mosaic_accumulate(g_fr.ptr, F, H, W, g_map.ptr, g_skip.ptr, x0, y0, Hc, Wc, code, g_state.ptr, nbytes, u8,
                                        d_exposure=None if ex is None else g_ex.ptr)
                _oflk.mosaic_resolve(g_state.ptr, Hc, Wc, g_out.ptr, g_cnt.ptr, u8)
                _sync()
                what = f"mosaic {blend} exposure={ex is not None} F={F} {Hc}x{Wc}"
                b.check(what)
                SM.same(g_out.numpy(frames.dtype, (Hc, Wc)), want[0], f"{what} skew {skew}: canvas")
                SM.same(g_cnt.numpy(np.int32, (Hc, Wc)), want[1], f"{what} skew {skew}: count")


@pytest.mark.parametrize("Hc", [5, 6])
@pytest.mark.parametrize("Wc", [8, 9, 11])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_mosaic_median(u8, Wc, Hc):
    import _oflk

    H, W, x0, y0 = 5, 7, -1, -1
    esz = 1 if u8 else 4
    for F in (1, 3):
        frames, maps, skip, exposure = _mosaic_scene(F, H, W, Hc, Wc, u8, Hc * Wc + F + 7)
        for ex in (None, exposure):
            want = MMM.median(frames, maps, skip, x0, y0, Hc, Wc, ex)
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                b = _bands(fill, skew)
                g_fr, g_map, g_skip = b.inp("d_frames", frames, W * esz), b.inp("d_map", maps, skew=0), b.inp("d_skip", skip)
                g_ex = None if ex is None else b.inp("d_exposure", ex, skew=0)
                g_out = b.out("d_out", Hc * Wc * esz, Wc * esz, esz)
                g_cnt = b.out("d_count", Hc * Wc * 4, Wc * 4, 4, skew=4 if skew else 0)
                _oflk.mosaic_median(g_fr.ptr, F, H, W, g_map.ptr, g_skip.ptr, 0 if ex is None else g_ex.ptr, x0, y0, Hc, Wc,
                                    g_out.ptr, g_cnt.ptr, u8)
                _sync()
                what = f"mosaic median exposure={ex is not None} F={F} {Hc}x{Wc}"
                b.check(what)
                SM.same(g_out.numpy(frames.dtype, (Hc, Wc)), want[0], f"{what} skew {skew}: canvas")
                SM.same(g_cnt.numpy(np.int32, (Hc, Wc)), want[1], f"{what} skew {skew}: count")


# ---------------------------------------------------------------------------------------------------------------------
# dense flow through a plan
# ---------------------------------------------------------------------------------------------------------------------
DENSE = [(H, W) for H in (24, 25, 37) for W in (64, 66, 53)]   # W % 4 == 0, W % 4 == 2, odd; a partial last tile row


def _flow_outs(b, names, B, H, W, skew):
    return [b.out(n, B * H * W * 4, 4 * W, 4, skew=4 if skew else 0) for n in names]


def _same_flow(g_u, g_v, shape, b_index, want, what):
    u, v = g_u.numpy(np.float32, shape)[b_index], g_v.numpy(np.float32, shape)[b_index]
    assert np.array_equal(u, want[0]) and np.array_equal(v, want[1]), f"{what}: pair {b_index} differs from its reference"


@pytest.mark.parametrize("H,W", DENSE, ids=lambda v: str(v))
@pytest.mark.parametrize("win", [5, 7])
def test_dense_single_scale(oracle, win, H, W):
    """oflk_plan_single_scale and _u8 through the tile kernel and the streaming kernel against the oracle, value for value;
    oflk_plan_single_scale_fp16 against its model within the ulp bound of tests/test_gpu_fp16.py"""
    import oflk_fp16_model as M16

    import _oflk
    from oflk_synth import synth_pair
    from test_gpu_fp16 import MODEL_ULP

    for B in (1, 3):
        pairs = [synth_pair(H, W, H + W + b) for b in range(B)]
        p, c = np.stack([x[0] for x in pairs]).astype(np.float32), np.stack([x[1] for x in pairs]).astype(np.float32)
        want = [oracle.lucas_kanade_single_scale(p[b], c[b], win) for b in range(B)]
        want16 = [M16.fp16_flow(p[b], c[b], win) for b in range(B)]
        plan = _oflk.Plan(0, B, H, W, 1, win, 0)
        try:
            for kernels, u8 in ((1, False), (2, False), (1, True), (2, True), (0, "fp16")):
                plan.set_kernels(kernels)
                call = {False: plan.single_scale, True: plan.single_scale_u8, "fp16": plan.single_scale_fp16}[u8]
                fp, fc = (p.astype(np.uint8), c.astype(np.uint8)) if u8 is True else (p, c)
                for fill, skew in _runs(*((1, 2) if u8 is True else (4,))):
                    b = _bands(fill, skew)
                    g_p, g_c = b.inp("d_prev", fp, W * fp.itemsize), b.inp("d_curr", fc, W * fp.itemsize)
                    g_u, g_v = _flow_outs(b, ("d_u", "d_v"), B, H, W, skew)
                    call(g_p.ptr, g_c.ptr, g_u.ptr, g_v.ptr)
                    _sync()
                    what = f"single scale {win}x{win} kernels={kernels} {u8} B={B} {H}x{W} skew {skew}"
                    b.check(what)
                    for i in range(B):
                        if u8 == "fp16":
                            u, v = g_u.numpy(np.float32, (B, H, W))[i], g_v.numpy(np.float32, (B, H, W))[i]
                            zeros, d = M16.compare(u, v, *want16[i])
                            assert zeros and d <= MODEL_ULP, (what, i, zeros, d)
                        else:
                            _same_flow(g_u, g_v, (B, H, W), i, want[i], what)
        finally:
            plan.close()


def _dense_forms(plan, frames, exact, ref, what0, flagged_first=False):
    """the pair, sequence and two-direction passes of `plan` on guarded frames and flows, each followed by its resolve call.
    Before the resolve an unflagged pair equals ref, after it a flagged one equals exact (both {"f": [...], "b": [...]} of
    (u, v) per pair).  flagged_first: pair 0 must be flagged, so that the resolve call has something to write"""
    B, H, W = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
    u8, esz = frames.dtype == np.uint8, frames.itemsize
    for form in ("pairs", "sequence", "sequence_fb"):
        for fill, skew in _runs(*((1, 2) if u8 else (4,))):
            b = _bands(fill, skew)
            what = f"{what0} {form} u8={u8} B={B} {H}x{W} skew {skew}"
            if form == "pairs":
                g_p = b.inp("d_prev", frames[:-1], W * esz)
                g_c = b.inp("d_curr", frames[1:], W * esz)
                prev, curr = g_p.ptr, g_c.ptr
            else:
                g_f = b.inp("d_frames", frames, W * esz)
                prev, curr = g_f.ptr, g_f.ptr + H * W * esz
            dirs = ("f", "b") if form == "sequence_fb" else ("f",)
            outs = _flow_outs(b, [f"d_{x}{d}" for d in dirs for x in "uv"], B, H, W, skew)
            ptrs = [g.ptr for g in outs]
            if form == "pairs":
                (plan.pyramidal_u8 if u8 else plan.pyramidal)(prev, curr, *ptrs)
            elif form == "sequence":
                plan.pyramidal_sequence(prev, *ptrs, u8=u8)
            else:
                plan.pyramidal_sequence_fb(prev, *ptrs, u8=u8)
            flags = {"f": plan.read_uncertain()}
            if form == "sequence_fb":
                flags["b"] = plan.read_uncertain_backward()
            _sync()
            b.check(what)
            for k, d in enumerate(dirs):
                for i in range(B):
                    if not flags[d][i].any():
                        _same_flow(outs[2 * k], outs[2 * k + 1], (B, H, W), i, ref[d][i], f"{what} direction {d}")
            if flagged_first:
                assert flags["f"][0].any(), f"{what}: pair 0 is not flagged"
            if form == "sequence_fb":
                n = plan.resolve_uncertain_sequence_fb(prev, *ptrs, u8=u8)
            else:
                n = plan.resolve_uncertain(prev, curr, *ptrs, u8=u8)
            _sync()
            assert n == sum(int(flags[d][i].any()) for d in dirs for i in range(B)), what
            b.check(what + ", resolved")
            for k, d in enumerate(dirs):
                for i in range(B):
                    want = exact[d][i] if flags[d][i].any() else ref[d][i]
                    _same_flow(outs[2 * k], outs[2 * k + 1], (B, H, W), i, want, f"{what} direction {d}, resolved")


def _both_directions(frames, fn):
    f = frames.astype(np.float32)
    B = len(f) - 1
    return {"f": [fn(f[t], f[t + 1]) for t in range(B)], "b": [fn(f[t + 1], f[t]) for t in range(B)]}


@pytest.mark.parametrize("H,W", DENSE, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", ["exact", "tolerant"])
def test_dense_pyramidal(oracle, mode, H, W):
    """oflk_plan_pyramidal, _u8, _sequence and _sequence_fb at (3, 3): every pair equals the mode's reference (the oracle, or
    the CPU model of the tolerant arithmetic).  No pair of these scenes is flagged: the resolve calls are held to their
    stores by test_dense_resolve_uncertain"""
    import _oflk
    from test_gpu_exit_band import ARITH, _reference
    from test_gpu_sequence import _video

    L = K = 3
    for B in (1, 3):
        for u8 in (False, True):
            frames = _video(B + 1, H, W, seed=H + W + B, u8=u8)
            exact = _both_directions(frames, lambda a, c: oracle.lucas_kanade_pyramidal_ex(a, c, L, 5, K)[:2])
            ref = exact if mode == "exact" else _both_directions(frames, lambda a, c: _reference(oracle, mode, a, c, L, K, 5)[:2])
            plan = _oflk.Plan(0, B, H, W, L, 5, K)
            try:
                plan.set_arithmetic(ARITH[mode])
                _dense_forms(plan, frames, exact, ref, f"pyramidal {mode}")
            finally:
                plan.close()


FLAGGED = [(48, 64, True), (37, 66, False), (37, 53, False)]   # (H, W, byte-valued frames: they also run as uint8)
_flagged_pairs = {}


def _flagged_pair(oracle, H, W, bytes_only):
    """(prev, curr) float32 whose first exit decision (level 0 of 2, iteration 0) has its EXACT mean within half the
    library's decision band of the threshold, so that the device flags the pair: the placement of
    test_gpu_exit_band.test_near_threshold_decisions_flagged_as_the_bounds_say, curr = prev + t (shifted - prev) with t
    bisected on the CPU.  bytes_only: both frames rounded to bytes (t then moves the mean in steps, and a seed is taken
    only if a step lands inside); computed once"""
    import _oflk
    from oflk_synth import synth_pair
    from test_gpu_exit_band import THR, _reference
    from test_tolerant_model import level_sum_path

    if (H, W) in _flagged_pairs:
        return _flagged_pairs[H, W]
    L = K = 2
    dims = oracle.pyramid_dims(H, W, L)
    g = float(_oflk.lib().oflk_decision_guard(level_sum_path(0, L, K, 5, dims, 0), *dims[0]))
    for seed in range(16):
        prev, shifted = synth_pair(H, W, seed, dx=0.75, dy=-0.5)
        prev = np.rint(prev).astype(np.float32) if bytes_only else prev
        delta = (shifted - prev).astype(np.float64)

        def curr(t):
            c = prev + t * delta
            return np.clip(np.rint(c), 0, 255).astype(np.float32) if bytes_only else c.astype(np.float32)

        def mean(t):
            return float(max(_reference(oracle, "exact", prev, curr(t), L, K, 5)[4][0, 0]))

        lo, hi = 0.0, 1.0
        if not mean(lo) < THR < mean(hi):
            continue
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean(mid) < THR else (lo, mid)
        t = min((lo, hi), key=lambda e: abs(mean(e) - THR))
        if abs(mean(t) / THR - 1.0) < 0.5 * g:
            _flagged_pairs[H, W] = (prev, curr(t))
            return _flagged_pairs[H, W]
    raise AssertionError(f"{H}x{W}: no seed puts the first decision's mean within half the band {g:.1e} of the threshold")


@pytest.mark.parametrize("H,W,bytes_only", FLAGGED, ids=lambda v: str(v))
def test_dense_resolve_uncertain(oracle, H, W, bytes_only):
    """oflk_plan_resolve_uncertain, _u8, _sequence_fb and _sequence_fb_u8 with something to write: pair 0 (and every other
    pair of the alternating sequence that repeats it) is flagged by construction, the resolve call redoes it into the guarded
    flows, and every pair then equals the oracle.  Exact arithmetic, 2 levels, 2 iterations"""
    import _oflk

    L = K = 2
    prev, curr = _flagged_pair(oracle, H, W, bytes_only)
    for B in (1, 3):
        f32 = np.ascontiguousarray(np.stack([prev, curr, prev, curr][:B + 1]))
        exact = _both_directions(f32, lambda a, c: oracle.lucas_kanade_pyramidal_ex(a, c, L, 5, K)[:2])
        plan = _oflk.Plan(0, B, H, W, L, 5, K)
        try:
            for frames in (f32, f32.astype(np.uint8)) if bytes_only else (f32,):
                _dense_forms(plan, frames, exact, exact, "resolve", flagged_first=True)
        finally:
            plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# points: oflk_track_points, oflk_plan_sparse_tracks, oflk_plan_sparse_klt_replenish (the blocks are one wave)
# ---------------------------------------------------------------------------------------------------------------------
POINTS = [1, 63, 65]


def _point_queries(H, W, seed):
    """65 queries of frames 0 and 1: points inside, and a few on the edges, outside and not finite"""
    rng = np.random.default_rng(seed)
    xy = (rng.random((65, 2)) * [W - 1, H - 1]).astype(np.float32)
    xy[5], xy[20], xy[40], xy[62], xy[64] = (W - 1, H - 1), (-1, 2), (np.nan, 1), (0, 0), (W - 1 + 2.0 ** -18, 1)
    qt = rng.integers(0, 2, 65).astype(np.int32)
    qt[0] = 0
    return qt, xy


def _point_rows(b, B, N, skew, pair=8):
    """d_tracks skewed by one (x, y) pair where the call wants it 8-byte aligned (pair=4: by one float), d_visible by a byte"""
    return (b.out("d_tracks", (B + 1) * N * 8, N * 8, skew=pair if skew else 0), b.out("d_visible", (B + 1) * N, N, skew=1 if skew else 0))


@pytest.mark.parametrize("N", POINTS)
def test_track_points(N):
    import track_model as TM

    import _oflk
    from test_gpu_tracks import _same_tracks

    H, W = 17, 23
    flows = TM.smooth_flows(3, H, W, seed=4, scale=2.5)
    qt, xy = _point_queries(H, W, 2)
    want = TM.track(*flows, qt, xy)
    assert want[1][-1].any() and not want[1][-1].all()
    for B in (1, 3):
        for fill, skew in _runs(4):
            b = _bands(fill, skew)
            g_fl = [b.inp(n, f[:B], 4 * W) for n, f in zip(("d_uf", "d_vf", "d_ub", "d_vb"), flows)]
            g_q, g_qt = b.inp("d_qxy", xy[:N]), b.inp("d_qt", qt[:N])
            g_tr, g_vis = _point_rows(b, B, N, skew)
            _oflk.track_points(*(g.ptr for g in g_fl), B, H, W, g_q.ptr, N, g_tr.ptr, g_vis.ptr, d_qt=g_qt.ptr)
            _sync()
            b.check(f"track_points N={N} B={B}")
            _same_tracks((g_tr.numpy(np.float32, (B + 1, N, 2)), g_vis.numpy(np.uint8, (B + 1, N))),
                         (want[0][:B + 1, :N], want[1][:B + 1, :N]), f"track_points N={N} B={B} skew {skew}")


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("N", POINTS)
def test_sparse_tracks(N, u8):
    import sparse_model as S

    import _oflk
    from test_gpu_tracks import _same_tracks
    from test_sparse_cpu import _drifting

    H, W = 40, 52
    frames = _drifting(4, H, W, 3)
    frames = np.rint(frames).astype(np.uint8) if u8 else frames
    qt, xy = _point_queries(H, W, 3)
    want = S.track(frames, qt, xy, 3, 5, 3)
    assert want[1][-1].any() and not want[1][-1].all()
    for B in (1, 3):
        plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
        try:
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                b = _bands(fill, skew)
                g_f = b.inp("d_frames", frames[:B + 1], W * frames.itemsize)
                g_q, g_qt = b.inp("d_qxy", xy[:N], skew=4 if skew else 0), b.inp("d_qt", qt[:N], skew=4 if skew else 0)
                g_tr, g_vis = _point_rows(b, B, N, skew, pair=4)   # this call's rows may lie at any float
                _oflk.sparse_tracks(plan, g_f.ptr, g_q.ptr, N, g_tr.ptr, g_vis.ptr, d_qt=g_qt.ptr, u8=u8)
                _sync()
                b.check(f"sparse_tracks N={N} B={B}")
                _same_tracks((g_tr.numpy(np.float32, (B + 1, N, 2)), g_vis.numpy(np.uint8, (B + 1, N))),
                             (want[0][:B + 1, :N], want[1][:B + 1, :N]), f"sparse_tracks N={N} B={B} u8={u8} skew {skew}")
        finally:
            plan.close()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("K", POINTS)
def test_sparse_klt_replenish(K, u8):
    """every row array, the slots and the workspace at exactly its promised bytes, over the prefill's garbage"""
    import sparse_replenish_model as SRM

    import _oflk
    from test_gpu_sequence import _video

    H, W, D, q, md = 48, 64, 2, 0.01, 3.0
    video = _video(4, H, W, seed=5, u8=u8)
    nbytes = _oflk.replenish_features_workspace(H, W, 5, md, K)
    for B in (1, 3):
        frames = video[:B + 1]
        want = SRM.sequence(frames, K, D, q, md)
        assert want[3][0] > 0
        plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
        try:
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                s4, s1 = (4 if skew else 0), (skew if u8 else skew // 4)
                b = _bands(fill, skew)
                g_f = b.inp("d_frames", frames, W * frames.itemsize)
                g_ws = b.out("d_workspace", nbytes, skew=0)
                g_qt, g_qxy = b.out("d_qt", K * 4, skew=s4), b.out("d_qxy", K * 8, skew=2 * s4)
                g_tr, g_vis = _point_rows(b, B, K, skew)
                g_born = b.out("d_born", (B + 1) * K, K, skew=s1)
                g_det = b.out("d_detected", (B + 1) * 4, skew=s4)
                g_res = b.out("d_residual", (B + 1) * K * 4, K * 4, skew=s4)
                _oflk.sparse_klt_replenish(plan, g_f.ptr, g_ws.ptr, nbytes, g_qt.ptr, g_qxy.ptr, g_tr.ptr, g_vis.ptr, g_born.ptr,
                                           g_det.ptr, K, D, q, md, d_residual=g_res.ptr, u8=u8)
                _sync()
                b.check(f"sparse_klt_replenish K={K} B={B}")
                got = (g_tr.numpy(np.float32, (B + 1, K, 2)), g_vis.numpy(np.uint8, (B + 1, K)), g_born.numpy(np.uint8, (B + 1, K)),
                       g_det.numpy(np.int32), g_res.numpy(np.float32, (B + 1, K)))
                SRM.same(got, want, f"sparse_klt_replenish K={K} B={B} u8={u8} skew {skew}")
        finally:
            plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------------------------------
FEATURE_SHAPES = [(17, 65), (15, 63)]   # one more and one less than the score kernel's 16 x 64 tile


def _feature_frames(F, H, W, u8):
    from test_gpu_features import _frame

    return np.stack([_frame(H, W, seed=H + W + f, u8=u8) for f in range(F)])


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("H,W", FEATURE_SHAPES, ids=lambda v: str(v))
def test_corner_score(H, W, u8):
    import feature_model as FM

    import _oflk

    for F in (1, 3):
        frames = _feature_frames(F, H, W, u8)
        for win in (3, 11):
            want = np.stack([FM.score(f, win) for f in frames])
            assert (want > 0).any()
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                b = _bands(fill, skew)
                g_f = b.inp("d_frames", frames, W * frames.itemsize)
                g_s = b.out("d_score", F * H * W * 4, 4 * W, 4, skew=4 if skew else 0)
                _oflk.corner_score(g_f.ptr, F, H, W, g_s.ptr, win, u8=u8)
                _sync()
                b.check(f"corner_score F={F} {H}x{W} window {win}")
                SM.same(g_s.numpy(np.float32, (F, H, W)), want, f"corner_score F={F} {H}x{W} window {win} skew {skew}")


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("H,W", FEATURE_SHAPES, ids=lambda v: str(v))
def test_good_features(H, W, K):
    import feature_model as FM

    import _oflk
    from test_gpu_features import _same_features

    q, md = 0.01, 3.0
    for u8 in (False, True):
        for F in (1, 3):
            frames = _feature_frames(F, H, W, u8)
            want = [FM.good_features(f, 5, q, md, K) for f in frames]
            assert all(w[0] == K for w in want)
            nbytes = _oflk.good_features_workspace(F, H, W, 5, md, K)
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                s4 = 4 if skew else 0
                b = _bands(fill, skew)
                g_f = b.inp("d_frames", frames, W * frames.itemsize)
                g_ws = b.out("d_workspace", nbytes, skew=0)
                g_cnt, g_xy, g_sc = b.out("d_count", F * 4, skew=s4), b.out("d_xy", F * K * 8, skew=2 * s4), b.out("d_score", F * K * 4, skew=s4)
                _oflk.good_features(g_f.ptr, F, H, W, g_ws.ptr, nbytes, g_cnt.ptr, g_xy.ptr, g_sc.ptr, K, q, md, 5, u8=u8)
                _sync()
                b.check(f"good_features F={F} K={K} {H}x{W}")
                _same_features((g_xy.numpy(np.float32, (F, K, 2)), g_sc.numpy(np.float32, (F, K)), g_cnt.numpy(np.int32)), want,
                               f"good_features F={F} K={K} {H}x{W} u8={u8} skew {skew}")


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("H,W", FEATURE_SHAPES, ids=lambda v: str(v))
def test_replenish_features(H, W, K):
    import feature_model as FM

    import _oflk
    from test_gpu_replenish import _garbage, _same_detection, _state, _want

    q, md, t = 0.01, 3.0, 4
    for u8 in (False, True):
        frame = _feature_frames(1, H, W, u8)[0]
        S = FM.score(frame, 5)
        nbytes = _oflk.replenish_features_workspace(H, W, 5, md, K)
        for free in sorted({1, K}):
            xy, vis = _state(S, K, md, seed=K + free, free=free)
            qt, qxy = _garbage(K, K)
            want = _want(S, xy, vis, q, md, t, qt, qxy)
            assert want[3] >= 1
            for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                s4, s1 = (4 if skew else 0), (skew if u8 else skew // 4)
                b = _bands(fill, skew)
                g_f = b.inp("d_frame", frame, W * frame.itemsize)
                g_xy, g_vis = b.inp("d_xy", xy, skew=2 * s4), b.inp("d_visible", np.asarray(vis, np.uint8), skew=s1)
                g_ws = b.out("d_workspace", nbytes, skew=0)
                g_qt, g_qxy = b.inout("d_qt", qt, skew=s4), b.inout("d_qxy", qxy, skew=2 * s4)
                g_born, g_det = b.out("d_born", K, skew=s1), b.out("d_detected", 4, skew=s4)
                _oflk.replenish_features(g_f.ptr, H, W, t, g_xy.ptr, g_vis.ptr, g_ws.ptr, nbytes, g_qt.ptr, g_qxy.ptr, g_born.ptr,
                                         g_det.ptr, K, q, md, 5, u8=u8)
                _sync()
                b.check(f"replenish_features K={K} free={free} {H}x{W}")
                got = (g_qt.numpy(np.int32), g_qxy.numpy(np.float32, (K, 2)), g_born.numpy(np.uint8), int(g_det.numpy(np.int32)[0]))
                _same_detection(got, want, f"replenish_features K={K} free={free} {H}x{W} u8={u8} skew {skew}")


# ---------------------------------------------------------------------------------------------------------------------
# fits
# ---------------------------------------------------------------------------------------------------------------------
FIT_N = [4, 63, 65, 257]


def _fit_scene(kind, S, N):
    """S steps of N correspondences (src, dst, valid) and the same as rows of tracks: row t + 1 is step t's dst of row t"""
    planted = MM.planted_scene if kind == "motion" else HM.planted_scene
    src, dst, _ = planted(N, 0.0 if N == 4 else 0.3, N + S)
    rows = np.stack([src, dst, src, dst][:S + 1])
    rng = np.random.default_rng(N)
    vis = np.ones((S + 1, N), np.uint8)
    born = np.zeros((S + 1, N), np.uint8)
    if N > 8:
        vis[rng.integers(0, S + 1, 3), rng.integers(0, N, 3)] = 0
        born[S, 1] = 1
    valid = MM.tracks_valid(vis, born).astype(np.uint8)
    return np.ascontiguousarray(rows[:-1]), np.ascontiguousarray(rows[1:]), valid, rows, vis, born


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", FIT_N)
@pytest.mark.parametrize("kind", ["motion", "homography"])
def test_fits(kind, N, S):
    """oflk_estimate_* and oflk_tracks_*: model, inlier mask and counts, and the workspace at exactly its promised bytes"""
    import _oflk

    hyps, thr, seed, nc = 64, 1.0, 3, (6 if kind == "motion" else 9)
    src, dst, valid, rows, vis, born = _fit_scene(kind, S, N)
    if kind == "motion":
        families = [MM.SIMILARITY, MM.AFFINE] if N > 4 else [MM.TRANSLATION]
        nbytes = _oflk.motion_workspace(S, N, hyps)
    else:
        families = [None]
        nbytes = _oflk.homography_workspace(S, N, hyps)
    for fam in families:
        args = (hyps, thr, seed, 5) if fam is None else (fam, hyps, thr, seed, 5)
        model = HM if fam is None else MM
        want = model.estimate_batch(src, dst, valid, *args)
        assert want[2][:, 2].any(), "a step is fitted"
        for form in ("estimate", "tracks"):
            fn = getattr(_oflk, f"{form}_{kind}")
            for fill, skew in _runs(4):
                s1 = skew // 4
                b = _bands(fill, skew)
                if form == "estimate":
                    ins = [b.inp("d_src", src, skew=2 * skew), b.inp("d_dst", dst, skew=2 * skew), b.inp("d_valid", valid, skew=s1)]
                    head = (S, N)
                else:
                    ins = [b.inp("d_tracks", rows, skew=2 * skew), b.inp("d_visible", vis, skew=s1), b.inp("d_born", born, skew=s1)]
                    head = (S + 1, N)
                g_ws = b.out("d_workspace", nbytes, skew=0)
                g_m, g_i, g_c = b.out("d_model", S * nc * 4, itemsize=4), b.out("d_inlier", S * N, N, skew=s1), b.out("d_counts", S * 12, itemsize=4)
                fn(*(g.ptr for g in ins), *head, g_ws.ptr, nbytes, g_m.ptr, g_i.ptr, g_c.ptr, *args)
                _sync()
                what = f"{form}_{kind} family {fam} N={N} S={S}"
                b.check(what)
                MM.same((g_m.numpy(np.float32, (S, nc)), g_i.numpy(np.uint8, (S, N)), g_c.numpy(np.int32, (S, 3))), want,
                        f"{what} skew {skew}")


# ---------------------------------------------------------------------------------------------------------------------
# direct alignment: the plain, photometric and robust forms, pairs and sequences, and the weight map
# ---------------------------------------------------------------------------------------------------------------------
def _align_scene(S, code, u8, photometric):
    """S + 1 frames that alternate between a planted pair's two views (b re-exposed with photometric), the step models
    pushed off the planted ones, the last of three steps held"""
    import align_model as AM
    import align_photo_model as APM

    H, W = 33, 47
    A, B, planted = AM.planted_pair(H, W, 5 + S, code, move=2.0)
    if u8:
        A, B = np.float32(40.0) + np.float32(0.5) * A, np.float32(40.0) + np.float32(0.5) * B
    if photometric:
        B = APM.exposed(B, 0.8, 12.0)
    frames = np.stack([A, B, A, B][:S + 1])
    frames = np.rint(frames).astype(np.uint8) if u8 else np.ascontiguousarray(frames, np.float32)
    push = AM.pushed(planted, H, W, code, 0.5)
    model = np.stack([push, AM.IDENTITY[code], push][:S]).astype(np.float32)
    return frames, model, np.int32([1, 1, 0][:S])


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("form", ["plain", "photo", "robust", "robust-photo"])
@pytest.mark.parametrize("kind", ["homography", "affine"])
def test_align(oracle, kind, form, u8, S):
    import align_model as AM
    import align_photo_model as APM
    import align_robust_model as ARM

    import _oflk

    code = AM.KINDS[kind]
    photometric, robust = form.endswith("photo"), form.startswith("robust")
    L, n, delta = 2, 2, 4.0
    frames, model, status = _align_scene(S, code, u8, photometric)
    T, H, W = frames.shape
    a, bb = np.ascontiguousarray(frames[:-1]), np.ascontiguousarray(frames[1:])
    if robust:
        want = ARM.refine(a, bb, model, delta, status, code, L, n, 0.25, photometric)
        same = ARM.same
    elif photometric:
        want, same = APM.refine(a, bb, model, status, code, L, n), APM.same
    else:
        want, same = AM.refine(a, bb, model, status, code, L, n), AM.same
    assert want[1][0] == 1, "the first step is refined"
    nbytes = _oflk.align_workspace(S, H, W, L, code, photometric, robust)
    ns = 8 if robust else 4
    for sequence in (False, True):
        for fill, skew in _runs(*((1, 2) if u8 else (4,))):
            s4 = 4 if skew else 0
            b = _bands(fill, skew)
            if sequence:
                heads = (b.inp("d_frames", frames, W * frames.itemsize).ptr, T)
            else:
                heads = (b.inp("d_a", a, W * frames.itemsize).ptr, b.inp("d_b", bb, W * frames.itemsize).ptr, S)
            g_mi, g_si = b.inp("d_model_in", model, skew=s4), b.inp("d_status_in", status, skew=s4)
            g_ws = b.out("d_workspace", nbytes, skew=0)
            g_mo, g_so = b.out("d_model_out", model.nbytes, skew=s4), b.out("d_status_out", S * 4, skew=s4)
            g_st = b.out("d_stats", S * ns * 8, skew=2 * s4)
            g_ph = b.out("d_photo_out", S * 8, skew=s4)
            fn = _oflk.align_sequence if sequence else _oflk.align_refine
            fn(*heads, H, W, L, n, code, 0.25, g_mi.ptr, g_si.ptr, g_ws.ptr, nbytes, g_mo.ptr, g_so.ptr, g_st.ptr, u8, 0,
               g_ph.ptr if photometric else None, delta if robust else None)
            _sync()
            what = f"align {kind} {form} {'sequence' if sequence else 'pairs'} S={S} u8={u8}"
            b.check(what)
            got = (g_mo.numpy(np.float32, model.shape), g_so.numpy(np.int32), g_st.numpy(np.float64, (S, ns)))
            if photometric:
                got += (g_ph.numpy(np.float32, (S, 2)),)
            else:
                assert (g_ph.numpy() == GB.PREFILL).all(), "d_photo_out is not written without photometric"
                if robust:
                    got += (np.stack([ARM.ONE] * S),)
            same(got, want, f"{what} skew {skew}")


@pytest.mark.parametrize("W", [7, 8])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_align_weights(oracle, u8, W):
    import align_model as AM
    import align_robust_model as ARM

    import _oflk
    from test_gpu_align_robust import _same_map

    H, delta = 9, 4.0
    for kind, code in AM.KINDS.items():
        for S in (1, 3):
            A, B, planted = AM.planted_pair(H, W, W + S, code, move=1.0)
            a, bb = np.stack([A, B, A][:S]), np.stack([B, A, B][:S])
            a, bb = (np.rint(a).astype(np.uint8), np.rint(bb).astype(np.uint8)) if u8 else (a.astype(np.float32), bb.astype(np.float32))
            model = np.stack([AM.IDENTITY[code], AM.pushed(planted, H, W, code, 0.5), AM.IDENTITY[code]][:S]).astype(np.float32)
            for photo in (None, np.stack([np.float32([0.8 + 0.01 * s, 12.0 - s]) for s in range(S)])):
                want = np.stack([ARM.weights(a[s], bb[s], model[s], code, delta, *(() if photo is None else photo[s])) for s in range(S)])
                assert want.any()
                for fill, skew in _runs(*((1, 2) if u8 else (4,))):
                    s4 = 4 if skew else 0
                    b = _bands(fill, skew)
                    g_a, g_b = b.inp("d_a", a, W * a.itemsize), b.inp("d_b", bb, W * a.itemsize)
                    g_m = b.inp("d_model", model, skew=s4)
                    g_p = None if photo is None else b.inp("d_photo", photo, skew=s4)
                    g_w = b.out("d_weights", S * H * W * 4, 4 * W, skew=s4)
                    _oflk.align_weights(g_a.ptr, g_b.ptr, S, H, W, code, delta, g_m.ptr, 0 if photo is None else g_p.ptr, g_w.ptr, u8)
                    _sync()
                    what = f"align_weights {kind} S={S} {H}x{W} u8={u8} photo={photo is not None}"
                    b.check(what)
                    _same_map(g_w.numpy(np.float32, (S, H, W)), want, f"{what} skew {skew}")


# ---------------------------------------------------------------------------------------------------------------------
# the rest of the header
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 1027])
def test_u8_to_f32(n):
    import _oflk

    src = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    for fill, skew in _runs(1, 2, 4):
        b = _bands(fill, skew)
        g_in = b.inp("d_in", src)
        g_out = b.out("d_out", 4 * n, skew=4 if skew else 0)
        _oflk.check(_oflk.lib().oflk_u8_to_f32(g_in.ptr, g_out.ptr, n, None))
        _sync()
        b.check(f"u8_to_f32 n={n}")
        assert np.array_equal(g_out.numpy(np.float32), src.astype(np.float32)), f"u8_to_f32 n={n} skew {skew}"


def test_the_helper_sees_a_stray_byte_on_the_device():
    """the band comparison itself, on device memory: one byte behind, one ahead, and an input changed"""
    for fill in GB.FILLS:
        g = GB.guarded(100, fill=fill, device="cuda:0", name="out")
        g.check()
        g.raw[g.end] ^= 1
        with pytest.raises(AssertionError, match=r"BEHIND the payload, offsets 0 \.\. 0 "):
            g.check()
        g = GB.guarded_input(np.arange(25, dtype=np.float32), fill=fill, skew=4, device="cuda:0")
        g.raw[g.start - 1] ^= 0x80
        with pytest.raises(AssertionError, match=r"AHEAD of the payload, offsets -1 \.\. -1 "):
            g.check()
        g.raw[g.start - 1] ^= 0x80
        g.raw[g.start + 3] ^= 1
        with pytest.raises(AssertionError, match=r"an input was written, payload offsets 3 \.\. 3 "):
            g.check()


@pytest.mark.parametrize("H,W", [(5, 5), (6, 9), (12, 17)], ids=lambda v: str(v))
def test_rtl_flow_device(H, W):
    import rtl_model as RM

    import _oflk

    M = (H - 4) * (W - 4)
    for B in (1, 3):
        rng = np.random.default_rng(H + W + B)
        p, c = rng.integers(0, 256, (B, H, W), dtype=np.uint8), rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        want = []
        for i in range(B):
            gx, gy, gt, _ = RM.gradient_stream(p[i], c[i])
            want.append(RM.flow_states(gx, gy, gt, W)[3:])
        for fill, skew in _runs(1, 2):
            b = _bands(fill, skew)
            g_p, g_c = b.inp("d_prev", p, W), b.inp("d_curr", c, W)
            g_u, g_v = b.out("d_u", B * M * 2, M * 2, skew=2 if skew else 0), b.out("d_v", B * M * 2, M * 2, skew=2 if skew else 0)
            _oflk.check(_oflk.lib().oflk_rtl_flow_u8_device(g_p.ptr, g_c.ptr, B, H, W, g_u.ptr, g_v.ptr, None))
            _sync()
            b.check(f"rtl flow B={B} {H}x{W}")
            u, v = g_u.numpy(np.int16, (B, M)).astype(np.int64), g_v.numpy(np.int16, (B, M)).astype(np.int64)
            for i in range(B):
                assert np.array_equal(u[i], want[i][0]) and np.array_equal(v[i], want[i][1]), f"rtl flow B={B} {H}x{W} pair {i} skew {skew}"


@pytest.mark.parametrize("W", [32, 33])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_stabilizer_push_and_flush_device(u8, W):
    """every emission of oflk_stabilizer_push_device and the r frames of oflk_stabilizer_flush_device into guarded d_out and
    d_inside: the frames are the sequence call's, the masks the warp statement's under the map of correction_device"""
    from test_gpu_stabilize import _sequence
    from test_gpu_stabilize_online import _stabilizer
    from test_gpu_tracker import _from_device

    T, H, r = 10, 24, 2
    frames, _ = SM.jitter_scene(4, T=T, H=H, W=W)
    frames = np.ascontiguousarray(frames if u8 else frames.astype(np.float32))
    assert frames.dtype == (np.uint8 if u8 else np.float32)
    args = (16, 4, 0.05, 3.0, MM.TRANSLATION, 32, 1.0, 1, SM.weights(r))
    want = _sequence(frames, *args, levels=2)[0]
    assert (want != frames).any()
    esz = frames.itemsize
    for fill, skew in _runs(*((1, 2) if u8 else (4,))):
        st = _stabilizer(frames, *args, levels=2)
        try:
            for t in range(T + 1):
                n = 1 if t < T else r
                b = _bands(fill, skew)
                g_out = b.out("d_out", n * H * W * esz, W * esz, esz)
                g_ins = b.out("d_inside", n * H * W, W)
                if t < T:
                    g_f = b.inp("d_frame", frames[t], W * esz)
                    e = st.push_device(g_f.ptr, g_out.ptr, g_ins.ptr)
                    assert e == (t - r if t >= r else -1)
                else:
                    e, count = st.flush_device(g_out.ptr, g_ins.ptr)
                    assert (e, count) == (T - r, r)
                _sync()
                what = f"stabilizer {'push' if t < T else 'flush'} {t} u8={u8} W={W} skew {skew}"
                b.check(what)
                if e < 0:
                    assert (g_out.numpy() == GB.PREFILL).all() and (g_ins.numpy() == GB.PREFILL).all(), f"{what}: nothing is emitted"
                    continue
                pm = st.correction_device()[1]
                mp = _from_device(pm, (n, 6), "<f8")
                model_out, model_in = SM.warp(frames[e:e + n], mp)
                SM.same(g_out.numpy(frames.dtype, (n, H, W)), want[e:e + n], f"{what}: out")
                SM.same(g_out.numpy(frames.dtype, (n, H, W)), model_out, f"{what}: out against the warp statement")
                SM.same(g_ins.numpy(np.uint8, (n, H, W)), model_in, f"{what}: inside")
        finally:
            st.close()
