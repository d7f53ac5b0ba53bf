"""GPU tests of the uint8 outputs at and beyond the byte range (run on an MI355X: python -m pytest tests/test_gpu_byte_range.py
-m gpu -q).  The scenes are tests/byte_range_scenes.py; tests/test_byte_range_cpu.py shows on the statements that they go where
they claim.

oflk_mosaic_resolve with u8 = 1 saturates: 0 for a NaN, otherwise rint, half to even, held to [0, 255].  It is held to the
statement (tests/mosaic_model.py) byte for byte on values from -1e30 to +inf; to itself, the uint8 resolve of a state against
the float32 resolve of the same state, with no model in between; and through the Python calls, uint8 frames against their
float32 copies.  The warps, the interpolation and the plain mosaic, which keep the bare conversion, equal their statements on
frames of 0 and 255.
"""
import numpy as np
import pytest

import byte_range_scenes as S
import mosaic_model as MM
import stabilize_model as SM

pytestmark = pytest.mark.gpu

BLENDS = list(MM.BLENDS.items())


def _saturate(v):
    """the rule, written here and not taken from the statement"""
    v = np.asarray(v)
    assert v.dtype == np.float32
    out = np.zeros(v.shape, np.uint8)
    ok = ~np.isnan(v)
    out[ok] = np.clip(np.rint(v[ok]), 0.0, 255.0).astype(np.uint8)
    return out


def _device(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend, cuts=()):
    """the device form on a cleared state, accumulated in the calls that `cuts` makes (exposure None: the plain accumulate),
    then resolved twice from that one state: ((uint8 canvas, count), (float32 canvas, count))"""
    import torch

    import _oflk

    d = "cuda:0"
    u8 = frames.dtype == np.uint8
    F, H, W = frames.shape
    nbytes = _oflk.mosaic_state_bytes(Hc, Wc)
    state = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=d)
    state[:nbytes].zero_()
    t_in = torch.from_numpy(np.ascontiguousarray(frames)).to(d)
    t_map = torch.from_numpy(np.ascontiguousarray(maps, np.float64).reshape(F, 9)).to(d)
    t_skip = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, np.uint8)).to(d)
    t_exp = None if exposure is None else torch.from_numpy(np.ascontiguousarray(exposure, np.float64).reshape(F, 2)).to(d)
    edges = [0, *cuts, F]
    for lo, hi in zip(edges[:-1], edges[1:]):
        _oflk.mosaic_accumulate(t_in.data_ptr() + lo * H * W * t_in.element_size(), hi - lo, H, W, t_map.data_ptr() + 72 * lo,
                                0 if t_skip is None else t_skip.data_ptr() + lo, x0, y0, Hc, Wc, blend, state.data_ptr(), nbytes, u8, 0,
                                None if t_exp is None else t_exp.data_ptr() + 16 * lo)
    got = []
    for flag, dtype in ((True, torch.uint8), (False, torch.float32)):
        out = torch.full((Hc * Wc + 64,), 77, dtype=dtype, device=d)
        count = torch.full((Hc * Wc + 64,), -3, dtype=torch.int32, device=d)
        _oflk.mosaic_resolve(state.data_ptr(), Hc, Wc, out.data_ptr(), count.data_ptr(), flag, 0)
        torch.cuda.synchronize()
        assert (out[Hc * Wc:] == 77).all().item() and (count[Hc * Wc:] == -3).all().item(), "nothing is written past the outputs"
        got.append((out[:Hc * Wc].cpu().numpy().reshape(Hc, Wc), count[:Hc * Wc].cpu().numpy().reshape(Hc, Wc)))
    assert (state[nbytes:] == 0xA5).all().item(), "nothing is written past the state"
    return got


def _scene(kind, key):
    """(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend code) of one cell"""
    if kind == "ladder":
        case, blend = key
        (_, _), (Hc, Wc), (x0, y0), _, _ = S.CASES[case]
        fr, maps, ex, code, _ = S.ladder(case, blend)
        return fr, maps, None, ex, x0, y0, Hc, Wc, code
    if kind == "wide":
        case, blend, dtype = key
        (_, _), (Hc, Wc), (x0, y0), _, _ = S.CASES[case]
        fr, maps, skip, ex = S.wide(case, dtype)
        return fr, maps, skip, ex, x0, y0, Hc, Wc, MM.BLENDS[blend]
    (name, projective, extra), blend = key
    fr, maps, (x0, y0), (Hc, Wc) = S.float_state(name, projective, extra)
    return fr, maps, None, None, x0, y0, Hc, Wc, MM.BLENDS[blend]


CELLS = ([("ladder", (c, b)) for c in range(2) for b in ("last", "first")] +
         [("wide", (c, b, t)) for c in range(2) for b in MM.BLENDS for t in (np.uint8, np.float32)] +
         [("float_state", (fs, b)) for fs in S.FLOAT_STATES for b in MM.BLENDS])


def _id(cell):
    kind, key = cell
    flat = [x for k in key for x in (k if isinstance(k, tuple) else (k,))]
    return kind + "-" + "-".join(np.dtype(x).name if isinstance(x, type) else str(x) for x in flat)


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_the_mosaic_equals_the_statement_beyond_the_byte_range(cell):
    """canvas and count, uint8 and float32 output: the device form in one call and cut into two, and the host form (which
    writes the frames' type: uint8 frames go in again as their float32 copies, whose state is the same; float_state has no
    uint8 host form)"""
    import _oflk

    fr, maps, skip, ex, x0, y0, Hc, Wc, code = _scene(*cell)
    st = S.state_of(fr, maps, skip, ex, x0, y0, Hc, Wc, code)
    want = [MM.resolve(st, True), MM.resolve(st, False)]
    assert (want[0][1] > 0).any() and want[0][0].dtype == np.uint8 and want[1][0].dtype == np.float32
    forms = [("one call", _device(fr, maps, skip, ex, x0, y0, Hc, Wc, code)),
             ("two calls", _device(fr, maps, skip, ex, x0, y0, Hc, Wc, code, cuts=(2,)))]
    host = [None, None]
    for f in ([fr, fr.astype(np.float32)] if fr.dtype == np.uint8 else [fr]):
        host[0 if f.dtype == np.uint8 else 1] = _oflk.mosaic_composite_host(np.ascontiguousarray(f), maps, skip, x0, y0, Hc, Wc, code, True,
                                                                            ex)
    forms.append(("host form", host))
    for name, got in forms:
        for g, w, out in zip(got, want, ("uint8", "float32")):
            if g is not None:
                SM.same(g[0], w[0], f"{_id(cell)} {name} {out}: canvas")
                SM.same(g[1], w[1], f"{_id(cell)} {name} {out}: count")


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_one_state_resolved_twice(cell):
    """out_u8 == saturate(out_f32) at every pixel of one accumulated state: no NumPy statement of the mosaic takes part"""
    fr, maps, skip, ex, x0, y0, Hc, Wc, code = _scene(*cell)
    (u8, c8), (f32, c32) = _device(fr, maps, skip, ex, x0, y0, Hc, Wc, code)
    assert np.array_equal(c8, c32) and (c8 > 0).any()
    SM.same(u8, _saturate(f32), f"{_id(cell)}: the uint8 resolve against the float32 resolve")
    assert not u8[c8 == 0].any() and not f32[c8 == 0].any()
    if cell[0] != "float_state" or cell[1][0][0] == "u16":
        assert (f32 > 255.5).any(), "the state goes above the byte range"
    if cell[0] != "float_state" or cell[1][0][0] == "signed":
        assert (f32 < -0.5).any(), "the state goes below the byte range"


def test_uint8_frames_against_their_float32_copies():
    """through lucas_kanade_core.mosaic_composite: a byte widens exactly, so the state is the same and the uint8 canvas is the
    saturated rounding of the float32 one"""
    import lucas_kanade_core as K

    for case in range(len(S.CASES)):
        (_, _), shape, origin, _, _ = S.CASES[case]
        fr, maps, skip, ex = S.wide(case)
        for blend in MM.BLENDS:
            cu, nu = K.mosaic_composite(fr, maps, shape, origin, skip, blend, True, exposure=ex)
            cf, nf = K.mosaic_composite(fr.astype(np.float32), maps, shape, origin, skip, blend, True, exposure=ex)
            assert cu.dtype == np.uint8 and cf.dtype == np.float32 and np.array_equal(nu, nf)
            SM.same(cu, _saturate(cf), f"wide {case} {blend}")
        fr, maps, ex, _, band = S.ladder(case, "last")
        cu = K.mosaic_composite(fr, maps, shape, origin, None, "last", exposure=ex)
        SM.same(cu, _saturate(K.mosaic_composite(fr.astype(np.float32), maps, shape, origin, None, "last", exposure=ex)), f"ladder {case}")
        for k, want in enumerate(S.RULE):
            assert (cu[band == k] == want).all(), f"ladder {case}: {S.TARGETS[k]} -> {want}, got {np.unique(cu[band == k])}"


def test_the_highlights_of_a_compensated_pan_read_255():
    """highlight_pan, grey and colour, under its planted exposures.  The bound on the uint8 canvas's error is derived: clipping
    to [0, 255] is 1-Lipschitz and rounding moves a value by at most 0.5, so |u8 - clip(truth)| <= |f32 - truth| + 0.5"""
    import lucas_kanade_core as K

    pan = S.highlight_pan()
    fr, maps, ex, origin, shape = pan["frames"], pan["maps"], pan["exposure"], pan["origin"], pan["shape"]
    for blend in ("mean", "feather"):
        cu, nu = K.mosaic_composite(fr, maps, shape, origin, None, blend, True, exposure=ex)
        cf, nf = K.mosaic_composite(fr.astype(np.float32), maps, shape, origin, None, blend, True, exposure=ex)
        assert np.array_equal(nu, nf) and (nu > 0).all()
        SM.same(cu, _saturate(cf), f"highlight_pan {blend}")
        high = cf >= 255.5
        print(f"{blend}: {int(high.sum())} canvas pixels at 255.5 or above, the largest {cf.max():.2f}")
        assert high.sum() > 100 and (cu[high] == 255).all()
        ok = (nu > 0) & ~pan["clipped"]
        err_u8 = np.abs(cu.astype(np.float64) - np.clip(pan["truth"], 0.0, 255.0))
        err_f32 = np.abs(cf.astype(np.float64) - pan["truth"])
        print(f"{blend}: over {int(ok.sum())} pixels the uint8 error is at most {err_u8[ok].max():.3f}, the float32 error {err_f32[ok].max():.3f}")
        assert ok.sum() > 10000 and (err_u8[ok] <= err_f32[ok] + 0.5 + 1e-9).all()
    colour = np.ascontiguousarray(np.stack([fr, 255 - fr, fr[:, ::-1]], -1))
    got = K.mosaic_composite(colour, maps, shape, origin, None, "feather", exposure=ex)
    assert got.dtype == np.uint8 and got.shape == shape + (3,)
    for c in range(3):
        cf = K.mosaic_composite(np.ascontiguousarray(colour[..., c], np.float32), maps, shape, origin, None, "feather", exposure=ex)
        SM.same(got[..., c], _saturate(cf), f"highlight_pan colour plane {c}")
        assert c > 0 or (cf >= 255.5).sum() > 100, "plane 0 is the grey pan"


def test_the_sequence_call_on_the_highlight_pan_is_the_chain_of_its_parts():
    """refine_photometric=True on frames whose highlights clip: the call equals the chain of the public parts, and the parts'
    float32 composite, saturated, is the call's canvas.  Nothing is asserted about how many pixels saturate: the exposures are
    estimated on the device"""
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    frames = S.highlight_pan()["frames"]
    T = len(frames)
    got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, anchor=T - 1, refine_iterations=3, refine_photometric=True)
    assert type(got) is P.PhotometricMosaic
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, 1000, 4, 0.01, 10.0, 3, 5, 3, 0.01, 0.5, 4.0)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born, 256, 1.0, 0)
    al = K.sequence_refine_alignment(frames, fit.model, fit.status, "homography", 3, 3, photometric=True)
    chain = K.mosaic_chain(al.model, fit.status, frames.shape[1:], anchor=T - 1)
    ex = K.exposure_chain(al.gain, al.bias, al.status == 1, anchor=T - 1)
    args = (chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", True)
    canvas, count = K.mosaic_composite(frames, *args, exposure=ex)
    assert got.origin == chain.origin
    for g, w, name in ((got.canvas, canvas, "canvas"), (got.count, count, "count"), (got.to_anchor, chain.to_anchor, "to_anchor"),
                       (got.model, al.model, "model"), (got.status, fit.status, "status"), (got.held, chain.held, "held"),
                       (got.dropped, chain.dropped, "dropped"), (got.exposure, ex, "exposure")):
        SM.same(np.asarray(g), np.asarray(w), f"sequence mosaic on the highlight pan: {name}")
    cf, nf = K.mosaic_composite(frames.astype(np.float32), *args, exposure=ex)
    assert np.array_equal(nf, count)
    SM.same(got.canvas, _saturate(cf), "the parts' float32 composite, saturated")
    print(f"{int((cf >= 255.5).sum())} canvas pixels at 255.5 or above, {int((cf < -0.5).sum())} below -0.5")


@pytest.mark.parametrize("name", S.EXTREMES)
def test_the_warps_equal_their_statements_on_the_extremes(name):
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    for what, layout, arg, frames, maps in S.warp_cells(name):
        want = S.warp_statement(layout, arg, frames, maps)
        affine = maps.shape[1] == 6
        if layout == "nv12":
            got = (P.warp_affine_nv12 if affine else P.warp_perspective_nv12)(frames, maps, arg)
        else:
            got = (K.warp_affine if affine else K.warp_perspective)(frames, maps)
        SM.same(got, want, what)
        if name in ("zeros", "full") and layout != "nv12":
            assert set(np.unique(got).tolist()) <= {0, 255 if name == "full" else 0}, f"{what}: 0 stays 0 and 255 stays 255"


@pytest.mark.parametrize("name", S.EXTREMES)
def test_the_interpolation_equals_its_statement_on_the_extremes(name):
    import lucas_kanade_pyramidal as P

    for what, layout, arg, frames, flows, taus in S.interp_cells(name):
        want = S.interp_statement(layout, arg, frames, flows, taus)
        if layout == "nv12":
            got = P.interpolate_frames_nv12(frames, *flows, taus=taus, siting=arg)
        else:
            got = P.interpolate_frames(frames, *flows, taus=taus)
        SM.same(got, want, what)
        if name in ("zeros", "full"):
            assert (got == (255 if name == "full" else 0)).all(), f"{what}: 0 stays 0 and 255 stays 255"


@pytest.mark.parametrize("name", S.EXTREMES)
def test_the_plain_mosaic_equals_its_statement_on_the_extremes(name):
    import lucas_kanade_core as K

    for what, frames, maps, skip, x0, y0, Hc, Wc in S.mosaic_cells(name):
        for blend, code in BLENDS:
            want = MM.composite(frames, maps, skip, x0, y0, Hc, Wc, code)
            got = K.mosaic_composite(frames, maps, (Hc, Wc), (x0, y0), skip, blend, True)
            SM.same(got[0], want[0], f"{what} {blend}: canvas")
            SM.same(got[1], want[1], f"{what} {blend}: count")
            if name == "full":
                assert (got[0][got[1] > 0] == 255).all()
