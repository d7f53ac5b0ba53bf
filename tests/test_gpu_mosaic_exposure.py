"""GPU tests of the exposure-compensated mosaic (run on an MI355X: python -m pytest tests/test_gpu_mosaic_exposure.py -m gpu -q).

oflk_mosaic_accumulate_exposure and the composite calls made of it must equal the statement (tests/mosaic_exposure_model.py)
byte for byte, a NaN equal to a NaN: the four blends, float32 and uint8, a canvas whose width is a multiple of 4 and one whose
width is not, frames added in two calls, and the unit exposure against the plain accumulate.  The pan under a changing
exposure goes through the public Python parts and through the mosaic call, whose refine_photometric=True must be the chain of
those parts.
"""
import numpy as np
import pytest

import align_photo_model as APM
import mosaic_exposure_model as MEM
import mosaic_model as MM
import stabilize_model as SM

pytestmark = pytest.mark.gpu

BLENDS = [("mean", MM.MEAN), ("feather", MM.FEATHER), ("first", MM.FIRST), ("last", MM.LAST)]
ANCHOR = 3


def _device(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend, cuts=()):
    """the device form on a cleared state, in the calls that `cuts` makes; exposure None: the plain accumulate"""
    import torch

    import _oflk

    d = "cuda:0"
    u8 = frames.dtype == np.uint8
    F, H, W = frames.shape
    nbytes = _oflk.mosaic_state_bytes(Hc, Wc)
    state = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=d)
    state[:nbytes].zero_()
    out = torch.full((Hc * Wc,), 77, dtype=torch.uint8 if u8 else torch.float32, device=d)
    count = torch.full((Hc * Wc,), -3, dtype=torch.int32, device=d)
    t_in = torch.from_numpy(np.ascontiguousarray(frames)).to(d)
    t_map = torch.from_numpy(np.ascontiguousarray(maps, np.float64).reshape(F, 9)).to(d)
    t_skip = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, np.uint8)).to(d)
    t_exp = None if exposure is None else torch.from_numpy(np.ascontiguousarray(exposure, np.float64).reshape(F, 2)).to(d)
    edges = [0, *cuts, F]
    for lo, hi in zip(edges[:-1], edges[1:]):
        _oflk.mosaic_accumulate(t_in.data_ptr() + lo * H * W * t_in.element_size(), hi - lo, H, W, t_map.data_ptr() + 72 * lo,
                                0 if t_skip is None else t_skip.data_ptr() + lo, x0, y0, Hc, Wc, blend, state.data_ptr(), nbytes, u8, 0,
                                None if t_exp is None else t_exp.data_ptr() + 16 * lo)
    _oflk.mosaic_resolve(state.data_ptr(), Hc, Wc, out.data_ptr(), count.data_ptr(), u8, 0)
    torch.cuda.synchronize()
    assert (state[nbytes:] == 0xA5).all().item(), "nothing is written past the state"
    return out.cpu().numpy().reshape(Hc, Wc), count.cpu().numpy().reshape(Hc, Wc)


def _scene(F, H, W, x0, y0, Hc, Wc, dtype, seed):
    rng = np.random.default_rng(seed)
    f = 40.0 + 100.0 * rng.random((F, H, W))
    frames = np.rint(f).astype(np.uint8) if dtype == np.uint8 else f.astype(np.float32)
    maps = np.stack([MM.translation(-(x0 - 2.25 + 3.37 * k), -(y0 - 1.5 + 1.21 * k)) for k in range(F)])
    maps[F // 2] = [0.9, 0.05, -0.9 * x0 + 1, -0.04, 1.1, -1.1 * y0 + 2, 1e-3, -1e-3, 1.0]   # a perspective frame
    maps[F - 1] = MM.translation(1e6, -3e5)                                                  # a frame that is culled
    skip = np.zeros(F, np.uint8)
    skip[1] = 1
    exposure = np.stack([rng.uniform(0.6, 1.5, F), rng.uniform(-20, 20, F)], 1)
    return frames, maps, skip, exposure


# frame, canvas (a width that is a multiple of 4 and one that is not; more than one block both ways), origin, frames
CASES = [((9, 13), (19, 68), (-7, 3), 6), ((17, 40), (21, 71), (5, -4), 7)]


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("blend", BLENDS, ids=[b[0] for b in BLENDS])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_compensated_accumulate_equals_the_model(case, blend, dtype):
    import _oflk

    (H, W), (Hc, Wc), (x0, y0), F = CASES[case]
    frames, maps, skip, exposure = _scene(F, H, W, x0, y0, Hc, Wc, dtype, case)
    what = f"case {case} {blend[0]} {np.dtype(dtype).name}"
    want = MEM.composite(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend[1])
    assert want[1].max() >= 3 and (want[1] == 0).any()
    one = _device(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend[1])
    two = _device(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend[1], cuts=(2,))
    host = _oflk.mosaic_composite_host(frames, maps, skip, x0, y0, Hc, Wc, blend[1], True, exposure)
    for got, name in ((one, "one call"), (two, "two calls"), (host, "host form")):
        SM.same(got[0], want[0], f"{what} {name}: canvas")
        SM.same(got[1], want[1], f"{what} {name}: count")
    unit = np.tile([1.0, 0.0], (F, 1))
    plain = _device(frames, maps, skip, None, x0, y0, Hc, Wc, blend[1])
    got = _device(frames, maps, skip, unit, x0, y0, Hc, Wc, blend[1])
    SM.same(got[0], plain[0], f"{what} unit exposure: canvas")
    SM.same(got[1], plain[1], f"{what} unit exposure: count")
    SM.same(plain[0], MM.composite(frames, maps, skip, x0, y0, Hc, Wc, blend[1])[0], f"{what} plain accumulate")


def test_the_refusals_and_the_colour_composite():
    import torch

    import _oflk
    import lucas_kanade_core as K

    frames, maps, skip, exposure = _scene(4, 9, 13, 0, 0, 12, 20, np.uint8, 3)
    with pytest.raises(ValueError):
        K.mosaic_composite(frames, maps, (12, 20), exposure=exposure[:3])
    nbytes = _oflk.mosaic_state_bytes(12, 20)
    state = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    t = torch.from_numpy(frames).to("cuda:0")
    m = torch.from_numpy(maps).to("cuda:0")
    with pytest.raises(ValueError):   # a NULL d_exposure
        _oflk.mosaic_accumulate(t.data_ptr(), 4, 9, 13, m.data_ptr(), 0, 0, 0, 12, 20, 0, state.data_ptr(), nbytes, True, 0, 0)
    with pytest.raises(ValueError):   # one that is not 8-byte aligned
        _oflk.mosaic_accumulate(t.data_ptr(), 4, 9, 13, m.data_ptr(), 0, 0, 0, 12, 20, 0, state.data_ptr(), nbytes, True, 0, m.data_ptr() + 4)
    colour = np.ascontiguousarray(np.stack([frames, frames[::-1], frames], -1))
    got = K.mosaic_composite(colour, maps, (12, 20), (0, 0), skip, "feather", exposure=exposure)
    for c in range(3):
        want = MEM.composite(np.ascontiguousarray(colour[..., c]), maps, skip, exposure, 0, 0, 12, 20, MM.FEATHER)
        SM.same(got[..., c], want[0], f"colour plane {c}")


def test_the_pan_mosaic_through_the_public_parts_is_four_times_nearer_the_source():
    """sequence_refine_alignment(photometric=True) -> mosaic_chain + exposure_chain -> mosaic_composite(exposure=...) on the
    8-frame pan, from the step models (-5 + 0.3, -0.2): the mean absolute difference from the source at the anchor's exposure
    is at most a quarter of the uncompensated composite's under the same chain, for the mean and the feather blend"""
    import lucas_kanade_core as K

    frames, src, gains, biases = APM.pan_scene()
    truth = gains[ANCHOR] * src + biases[ANCHOR]
    model = np.stack([MM.translation(-5 + 0.3, -0.2).astype(np.float32)] * 7).reshape(7, 3, 3)
    al = K.sequence_refine_alignment(frames, model, None, "homography", 3, 4, photometric=True)
    assert (al.status == 1).all()
    ch = K.mosaic_chain(al.model, None, (96, 128), anchor=ANCHOR)
    ex = K.exposure_chain(al.gain, al.bias, al.status == 1, anchor=ANCHOR)
    assert np.abs(ex[:, 0] - gains[ANCHOR] / gains).max() < 0.01
    f32 = frames.astype(np.float32)
    at = (4 + 5 * ANCHOR, 4)
    for blend in ("mean", "feather"):
        comp = K.mosaic_composite(f32, ch.from_anchor, ch.canvas_shape, ch.origin, ch.dropped, blend, True, exposure=ex)
        unc = K.mosaic_composite(f32, ch.from_anchor, ch.canvas_shape, ch.origin, ch.dropped, blend, True)
        ec, eu = MEM.source_error(*comp, ch.origin, truth, at), MEM.source_error(*unc, ch.origin, truth, at)
        print(f"{blend}: mean |mosaic - source| {eu[0]:.3f} -> {ec[0]:.3f} grey levels, worst {eu[1]:.2f} -> {ec[1]:.2f}")
        assert ec[0] <= eu[0] / 4.0


def test_refine_photometric_is_the_chain_of_the_public_parts_and_false_is_todays_call():
    """the pan through the tracker.  max_residual=16: under the default of 4 grey levels the exposure steps of this pan (up to
    about 6 grey levels) end tracks before the refinement sees the step"""
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    frames, _, _, _ = APM.pan_scene()
    kw = dict(max_corners=300, detect_every=4, max_residual=16.0)
    got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=ANCHOR, refine_iterations=2, refine_levels=2,
                                                   refine_photometric=True, **kw)
    assert type(got) is P.PhotometricMosaic and got._fields[:-1] == P.Mosaic._fields and got._fields[-1] == "exposure"
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, **kw)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born, 128, 1.0, seed=5)
    al = K.sequence_refine_alignment(frames, fit.model, fit.status, "homography", 2, 2, photometric=True)
    chain = K.mosaic_chain(al.model, fit.status, (96, 128), anchor=ANCHOR)
    ex = K.exposure_chain(al.gain, al.bias, al.status == 1, anchor=ANCHOR)
    canvas, count = K.mosaic_composite(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", True, exposure=ex)
    assert fit.status.all() and (al.status == 1).any() and got.origin == chain.origin and not (ex == [1.0, 0.0]).all()
    for g, w, name in ((got.canvas, canvas, "canvas"), (got.count, count, "count"), (got.to_anchor, chain.to_anchor, "to_anchor"),
                       (got.model, al.model, "model"), (got.status, fit.status, "status"), (got.held, chain.held, "held"),
                       (got.dropped, chain.dropped, "dropped"), (got.exposure, ex, "exposure")):
        SM.same(np.asarray(g), np.asarray(w), f"mosaic refine_photometric: {name}")
    base = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=ANCHOR, refine_iterations=2, refine_levels=2, **kw)
    off = P.lucas_kanade_pyramidal_sequence_mosaic(frames, hypotheses=128, seed=5, anchor=ANCHOR, refine_iterations=2, refine_levels=2,
                                                   refine_photometric=False, **kw)
    assert type(off) is P.Mosaic
    for g, w, name in zip(off, base, base._fields):
        SM.same(np.asarray(g), np.asarray(w), f"mosaic refine_photometric=False: {name}")
    # the stabiliser only uses the better models
    st = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5, max_residual=16.0,
                                                     refine_iterations=2, refine_levels=2, refine_photometric=True)
    fa = K.tracks_motion(rows.tracks, rows.visible, rows.born, "affine", 256, 1.0, 5)
    aa = K.sequence_refine_alignment(frames, fa.model, fa.status, "affine", 2, 2, photometric=True)
    tr = K.stabilize_trajectory(aa.model, fa.status, 3)
    for g, w, name in ((st.frames, K.warp_affine(frames, tr.map), "frames"), (st.correction, tr.correction, "correction"),
                       (st.model, aa.model, "model"), (st.status, fa.status, "status"), (st.held, tr.held, "held")):
        SM.same(np.asarray(g), np.asarray(w), f"stabilize refine_photometric: {name}")
    sb = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5, max_residual=16.0, refine_iterations=2,
                                                     refine_levels=2)
    sf = P.lucas_kanade_pyramidal_sequence_stabilize(frames, 300, 4, model="affine", radius=3, seed=5, max_residual=16.0, refine_iterations=2,
                                                     refine_levels=2, refine_photometric=False)
    for g, w, name in zip(sf, sb, sb._fields):
        SM.same(np.asarray(g), np.asarray(w), f"stabilize refine_photometric=False: {name}")
    for fn in (P.lucas_kanade_pyramidal_sequence_mosaic, lambda f, **k: P.lucas_kanade_pyramidal_sequence_stabilize(f, 300, 4, **k)):
        with pytest.raises(ValueError):
            fn(frames, refine_photometric=True)
