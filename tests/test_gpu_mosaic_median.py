"""GPU tests of the temporal-median mosaic (run on an MI355X: python -m pytest tests/test_gpu_mosaic_median.py -m gpu -q).

oflk_mosaic_median, its host forms, mosaic_median and the sequence call must equal the statement (tests/mosaic_median_model.py)
byte for byte, a NaN equal to a NaN: coverage counts on both sides of the ballot group of 64 frames and of the capacity a pixel
keeps on chip, counts that differ between the lanes of a wave, the map kinds that matter to the cull, canvases around the
kernel's tile sizes, both pixel types, special values, and the agreement with the existing blends' calls.
"""
import numpy as np
import pytest

import mosaic_exposure_model as MEM
import mosaic_median_model as MD
import mosaic_model as MM
import stabilize_model as SM

pytestmark = pytest.mark.gpu

TILE_W, BLOCK_W = 16, 64   # k_mosaic_median's wave tile and block, a pixel a lane


def _device(frames, maps, skip, exposure, x0, y0, Hc, Wc, count=True, stream=0, offset=0, twice=False):
    """the device form into outputs that begin `offset` elements into guarded buffers: (canvas, count or None)"""
    import torch

    import _oflk

    d = "cuda:0"
    u8 = frames.dtype == np.uint8
    F, H, W = frames.shape
    n = Hc * Wc
    out = torch.full((n + offset + 64,), 77, dtype=torch.uint8 if u8 else torch.float32, device=d)
    cnt = torch.full((n + offset + 64,), -3, dtype=torch.int32, device=d)
    t_in = torch.from_numpy(np.ascontiguousarray(frames)).to(d)
    t_map = torch.from_numpy(np.ascontiguousarray(maps, np.float64).reshape(F, 9)).to(d)
    t_skip = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, np.uint8)).to(d)
    t_exp = None if exposure is None else torch.from_numpy(np.ascontiguousarray(exposure, np.float64).reshape(F, 2)).to(d)
    torch.cuda.synchronize()
    for _ in range(2 if twice else 1):
        _oflk.mosaic_median(t_in.data_ptr(), F, H, W, t_map.data_ptr(), 0 if t_skip is None else t_skip.data_ptr(),
                            0 if t_exp is None else t_exp.data_ptr(), x0, y0, Hc, Wc, out.data_ptr() + offset * out.element_size(),
                            cnt.data_ptr() + 4 * offset if count else 0, u8, stream)
    torch.cuda.synchronize()
    assert (out[:offset] == 77).all().item() and (out[offset + n:] == 77).all().item(), "nothing is written outside the canvas"
    assert (cnt[:offset] == -3).all().item() and (cnt[offset + n:] == -3).all().item(), "nothing is written outside the count"
    if not count:
        assert (cnt == -3).all().item()
    return (out[offset:offset + n].cpu().numpy().reshape(Hc, Wc), cnt[offset:offset + n].cpu().numpy().reshape(Hc, Wc) if count else None)


def _check(got, want, what):
    SM.same(got[0], want[0], f"{what}: canvas")
    if got[1] is not None:
        SM.same(got[1], want[1], f"{what}: count")


def _pixels(shape, dtype, seed):
    f = 20.0 + 200.0 * np.random.default_rng(seed).random(shape)
    return np.rint(f).astype(np.uint8) if dtype == np.uint8 else (f - 100.0).astype(np.float32)


HALVES = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]


def _covering(F, dtype, shifted, seed=0):
    """F frames of 20 x 69 that all cover the canvas of 19 x 68 at the origin under the identity and half-pixel translations;
    shifted: every third frame moved off the canvas's left half, so the count changes inside a wave's tile"""
    frames = _pixels((F, 20, 69), dtype, seed)
    maps = np.stack([MM.translation(*HALVES[k % 4]) for k in range(F)])
    if shifted:
        for k in range(2, F, 3):
            maps[k] = MM.translation(HALVES[k % 4][0] - 37.0, HALVES[k % 4][1])
    return frames, maps


def _counts():
    import _oflk

    cap = _oflk.mosaic_median_capacity()
    # 2 cap - 1 is the last count whose median is among the cap smallest samples; 4 cap + 1 takes three walks
    return sorted({1, 2, 3, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap + 1, 2 * cap - 1, 2 * cap, 4 * cap + 1} - {0})


@pytest.mark.parametrize("shifted", [False, True], ids=["whole", "shifted"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_coverage_counts_across_the_ballot_group_and_the_capacity(dtype, shifted):
    import _oflk

    cap = _oflk.mosaic_median_capacity()
    for F in _counts():
        frames, maps = _covering(F, dtype, shifted, F)
        want = MD.median(frames, maps, None, 0, 0, 19, 68)
        assert want[1].max() == F and (shifted and F >= 3) == bool((want[1] < F).any())
        assert not shifted or F < 3 or len(np.unique(want[1][:4, 32:48])) > 1, "the count differs inside one wave's tile"
        _check(_device(frames, maps, None, None, 0, 0, 19, 68), want, f"F = {F} (capacity {cap})")


def _kinds(F, H, W, x0, y0, dtype, seed):
    """frames of the kinds that matter to the cull: sub-pixel translations that walk over the canvas, a mild homography, a frame
    behind the camera on part of a tile, a NaN coefficient, a frame far away, a skipped frame"""
    frames = _pixels((F, H, W), dtype, seed)
    maps = np.stack([MM.translation(-(x0 - 2.25 + 3.37 * k), -(y0 - 1.5 + 1.21 * k)) for k in range(F)])
    maps[0] = MM.translation(-x0, -y0)                                                           # the identity on the canvas
    maps[2] = [0.9, 0.05, -0.9 * x0 + 1, -0.04, 1.1, -1.1 * y0 + 2, 1e-3, -1e-3, 1.0]          # a mild homography
    maps[3] = [1.0, 0.0, -x0 - 3.0, 0.0, 1.0, -y0 - 1.0, -1.0 / 9.0, 0.0, 1.0 + x0 / 9.0]       # w <= 0 from canvas column 9 on
    maps[4] = MM.translation(-x0 - 1.5, -y0 - 0.25)
    maps[4][1] = np.nan                                                                         # a NaN coefficient
    maps[5] = MM.translation(1e6, -3e5)                                                         # far away: culled
    skip = np.zeros(F, np.uint8)
    skip[6] = 1
    return frames, maps, skip


# frame, canvas, origin: the mosaic tests' smallest case; canvases of one pixel, one row and one column; widths one short of and
# one past a wave's tile and a block; a second block both ways
CANVASES = [((9, 13), (19, 68), (-7, 3)), ((9, 13), (1, 1), (0, 0)), ((9, 13), (1, 68), (5, -4)), ((9, 13), (19, 1), (-2, -3)),
            ((9, 13), (5, TILE_W - 1), (0, 0)), ((9, 13), (5, TILE_W + 1), (-1, 0)), ((9, 13), (6, BLOCK_W - 1), (0, -2)),
            ((9, 13), (3, 2), (1, 1)), ((17, 40), (21, BLOCK_W + 7), (5, -4))]


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("case", range(len(CANVASES)))
def test_the_map_kinds_and_the_canvas_shapes(case, dtype):
    (H, W), (Hc, Wc), (x0, y0) = CANVASES[case]
    frames, maps, skip = _kinds(12, H, W, x0, y0, dtype, case)
    exposure = np.stack([np.linspace(0.7, 1.4, 12), np.linspace(-15, 15, 12)], 1)
    for ex in (None, exposure):
        want = MD.median(frames, maps, skip, x0, y0, Hc, Wc, ex)
        what = f"case {case} {np.dtype(dtype).name} exposure {ex is not None}"
        _check(_device(frames, maps, skip, ex, x0, y0, Hc, Wc), want, what)
        _check(_device(frames, maps, skip, ex, x0, y0, Hc, Wc, count=False, offset=1), want, what + " no count, offset 1")
        _check(_device(frames, maps, skip, ex, x0, y0, Hc, Wc, offset=4, twice=True), want, what + " offset 4, launched twice")
    if case == 0:
        assert want[1].max() >= 4 and (want[1] == 0).any()
        part = MD.samples(frames, maps, skip, None, x0, y0, Hc, Wc)[1][3]
        assert part.any() and not part[:, 9:].any(), "the frame behind the camera covers the columns in front of it only"


SPECIALS = {"nan": 0x7FC00000, "-nan": 0xFFC00000, "inf": 0x7F800000, "-inf": 0xFF800000}
PLANTED = [["nan", 1.0], ["-nan", 1.0], ["nan", "-nan", 5.0], ["inf", "-inf"], ["inf", 3.0, "-inf"], ["-nan", "inf", "nan", 4.0],
           ["-inf", "-inf", 2.0], ["nan", "nan", "-nan"], ["inf", "inf"], ["-nan", "-inf", -3.0, "inf", "nan"]]


def test_planted_nans_and_infinities_of_both_signs():
    """pixel (0, 0) of frame f holds PLANTED[..][f]; under the identity and the half-pixel translations it is the first tap, with
    a positive weight, of canvas pixel (0, 0)'s sample from every frame, so that pixel's samples are the planted values"""
    for row, planted in enumerate(PLANTED):
        frames, maps = _covering(len(planted), np.float32, False, 100 + row)
        bits = frames.view(np.uint32)
        for f, v in enumerate(planted):
            if isinstance(v, str):
                bits[f, 0, 0] = SPECIALS[v]
            else:
                frames[f] = v   # a constant frame: the sample is v whatever the weights
        want = MD.median(frames, maps, None, 0, 0, 19, 68)
        got = _device(frames, maps, None, None, 0, 0, 19, 68)
        _check(got, want, f"planted {planted}")
        e, _ = MD.samples(frames, maps, None, None, 0, 0, 19, 68)
        for f, v in enumerate(planted):
            if isinstance(v, str):
                assert e[f, 0, 0].view(np.uint32) & 0xFF800000 == SPECIALS[v] & 0xFF800000, f"{planted}: the sample keeps {v}"


def test_signed_zeros_ties_and_the_byte_store():
    zeros = np.zeros((3, 20, 69), np.float32)
    maps = np.stack([MM.translation(*HALVES[k]) for k in range(3)])
    for eg, bits in (((1.0, -1.0, -1.0), 0x80000000), ((1.0, 1.0, -1.0), 0), ((-1.0, -1.0, -1.0), 0x80000000)):   # e = +-0
        ex = np.array([[g, -0.0] for g in eg])
        want = MD.median(zeros, maps, None, 0, 0, 19, 68, ex)
        assert (want[0].view(np.uint32) == bits).all()
        _check(_device(zeros, maps, None, ex, 0, 0, 19, 68), want, f"signed zeros {eg}")
    for F in (1, 2, 5, 33, 34):   # constant frames: every key ties
        frames, maps = _covering(F, np.float32, True)
        frames[:] = np.float32(7.25)
        want = MD.median(frames, maps, None, 0, 0, 19, 68)
        assert (want[0] == 7.25).all()
        _check(_device(frames, maps, None, None, 0, 0, 19, 68), want, f"ties, F = {F}")
    for F in (2, 4, 34):   # 254 and 255 at even n: v = 254.5 stores 254
        frames, maps = _covering(F, np.uint8, False)
        frames[: F // 2], frames[F // 2:] = 254, 255
        want = MD.median(frames, maps, None, 0, 0, 19, 68)
        assert (want[0] == 254).all()
        _check(_device(frames, maps, None, None, 0, 0, 19, 68), want, f"254.5, F = {F}")


def test_an_exposure_that_leaves_the_byte_range_or_yields_a_nan():
    frames, maps = _covering(5, np.uint8, True, 7)
    frames[:] = np.clip(frames, 90, 250)
    for name, ex in (("above", [[3.0, 0.0]] * 5), ("below", [[-1.0, 0.0]] * 5), ("both", [[3.0, 0.0], [-1.0, 0.0], [3.0, 10.0], [-2.0, 0.0], [1.0, 0.0]]),
                     ("a NaN", [[1.0, 0.0], [1.0, np.nan], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0]]),
                     ("two NaNs", [[1.0, 0.0], [1.0, np.nan], [1.0, np.nan], [1.0, 0.0], [1.0, np.nan]])):
        ex = np.array(ex)
        for F in (4, 5):
            want = MD.median(frames[:F], maps[:F], None, 0, 0, 19, 68, ex[:F])
            _check(_device(frames[:F], maps[:F], None, ex[:F], 0, 0, 19, 68), want, f"exposure {name}, F = {F}")
        if name == "above":
            assert (want[0] == 255).all()
        if name == "below":
            assert (want[0] == 0).all()
    f32 = frames.astype(np.float32)
    ex = np.array([[1.0, 0.0], [1.0, np.nan], [2.0, 1.0], [1.0, np.nan], [1.0, -4.0]])
    want = MD.median(f32, maps, None, 0, 0, 19, 68, ex)
    assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()
    _check(_device(f32, maps, None, ex, 0, 0, 19, 68), want, "float32 under a NaN exposure")


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_agreement_with_the_existing_calls_and_the_host_and_python_forms(dtype):
    import torch

    import _oflk
    import lucas_kanade_core as K

    (H, W), (Hc, Wc), (x0, y0) = CANVASES[0]
    F = 2 * _oflk.mosaic_median_capacity() + 3
    frames, maps, skip = _kinds(F, H, W, x0, y0, dtype, 11)
    maps[12:] = maps[[7, 8]][np.arange(12, F) % 2]   # many frames on one spot: pixels beyond the capacity beside pixels below it
    exposure = np.stack([np.linspace(0.7, 1.4, F), np.linspace(-15, 15, F)], 1)
    for ex in (None, exposure):
        want = MD.median(frames, maps, skip, x0, y0, Hc, Wc, ex)
        assert want[1].max() > _oflk.mosaic_median_capacity() and (want[1] == 0).any()
        dev = _device(frames, maps, skip, ex, x0, y0, Hc, Wc)
        _check(dev, want, "the device form")
        blend = _oflk.mosaic_composite_host(frames, maps, skip, x0, y0, Hc, Wc, MM.MEAN, True, ex)
        SM.same(dev[1], blend[1], "count against accumulate / resolve")
        p = np.random.default_rng(3).permutation(F)
        _check(_device(frames[p], maps[p], skip[p], None if ex is None else ex[p], x0, y0, Hc, Wc), dev, "a frame permutation")
        side = torch.cuda.Stream()
        _check(_device(frames, maps, skip, ex, x0, y0, Hc, Wc, stream=side.cuda_stream), dev, "a stream of its own")
        _check(_oflk.mosaic_median_host(frames, maps, skip, ex, x0, y0, Hc, Wc, True), dev, "the host form")
        assert _oflk.mosaic_median_host(frames, maps, skip, ex, x0, y0, Hc, Wc, False)[1] is None
        _check(K.mosaic_median(frames, maps.reshape(F, 3, 3), (Hc, Wc), (x0, y0), skip != 0, True, ex), dev, "mosaic_median")
        SM.same(K.mosaic_median(frames, maps, (Hc, Wc), (x0, y0), skip, exposure=ex), dev[0], "mosaic_median without the count")
    for f in (0, 2, 3):
        one = K.mosaic_median(frames[f:f + 1], maps[f:f + 1], (Hc, Wc), (x0, y0), return_count=True)
        _check(one, K.mosaic_composite(frames[f:f + 1], maps[f:f + 1], (Hc, Wc), (x0, y0), blend="last", return_count=True), f"F = 1, frame {f}")


def test_colour_is_each_channels_grey_bytes():
    import lucas_kanade_core as K

    (H, W), (Hc, Wc), (x0, y0) = CANVASES[0]
    frames, maps, skip = _kinds(9, H, W, x0, y0, np.uint8, 21)
    for C in (3, 4):
        colour = np.ascontiguousarray(np.stack([np.roll(frames, c, axis=0) for c in range(C)], -1))
        got, cnt = K.mosaic_median(colour, maps, (Hc, Wc), (x0, y0), skip, True)
        assert got.shape == (Hc, Wc, C)
        for c in range(C):
            want = MD.median(np.ascontiguousarray(colour[..., c]), maps, skip, x0, y0, Hc, Wc)
            SM.same(got[..., c], want[0], f"{C} channels, plane {c}")
            SM.same(cnt, want[1], f"{C} channels: count")


def _source_error(canvas, count, origin, img):
    """the mean absolute difference from the source over the pixels that at least 5 frames cover, and their number"""
    often = MEM.source_error(canvas.astype(np.float64), (count >= 5).astype(np.int32), origin, img.astype(np.float64), (0, 0))
    return often[0], int((count >= 5).sum())


def test_the_sequence_call_is_the_chain_of_its_public_parts():
    """12 frames of 96 x 128 panning over a smooth_field image with the mover pasted in: plain, refined, and refined with a
    gain and a bias.  The difference from the source where >= 5 frames cover is printed beside the feather mosaic's (DESIGN
    section 2 records it); it rests on tracks and fits made on the device, so it has no bar here -- the CPU test has"""
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    img, frames, _ = MD.mover_scene(F=12, H=96, W=128, dx=6, image_shape=(100, 200), step=(7, 2), start=(4, 20), patch=(24, 28))
    kw = dict(max_corners=300, detect_every=4)
    rows = P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames, **kw)
    fit = K.tracks_homography(rows.tracks, rows.visible, rows.born, 128, 1.0, seed=5)
    for name, extra in (("plain", {}), ("refined", dict(refine_iterations=3)), ("photometric", dict(refine_iterations=3, refine_photometric=True))):
        got = P.lucas_kanade_pyramidal_sequence_mosaic_median(frames, hypotheses=128, seed=5, **kw, **extra)
        model, ex = fit.model, None
        if extra:
            al = K.sequence_refine_alignment(frames, fit.model, fit.status, "homography", 3, 3, photometric=name == "photometric")
            model = al.model
            if name == "photometric":
                ex = K.exposure_chain(al.gain, al.bias, al.status == 1, 0)
        chain = K.mosaic_chain(model, fit.status, (96, 128), 0)
        canvas, count = K.mosaic_median(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, True, ex)
        assert type(got) is (P.PhotometricMosaic if name == "photometric" else P.Mosaic) and got.origin == chain.origin
        parts = [(got.canvas, canvas, "canvas"), (got.count, count, "count"), (got.to_anchor, chain.to_anchor, "to_anchor"),
                 (got.model, model, "model"), (got.status, fit.status, "status"), (got.held, chain.held, "held"),
                 (got.dropped, chain.dropped, "dropped")] + ([(got.exposure, ex, "exposure")] if ex is not None else [])
        for g, w, what in parts:
            SM.same(np.asarray(g), np.asarray(w), f"{name}: {what}")
        feather = K.mosaic_composite(frames, chain.from_anchor, chain.canvas_shape, chain.origin, chain.dropped, "feather", exposure=ex)
        em, n = _source_error(got.canvas, got.count, got.origin, img)
        ef, _ = _source_error(feather, got.count, got.origin, img)
        print(f"{name}: mean |mosaic - source| over the {n} pixels that >= 5 frames cover: median {em:.3f}, feather {ef:.3f} grey levels")
    colour = np.ascontiguousarray(np.stack([frames, 255 - frames, frames], -1))
    got = P.lucas_kanade_pyramidal_sequence_mosaic_median(colour, hypotheses=128, seed=5, **kw)
    grey = P.lucas_kanade_pyramidal_sequence_mosaic_median(K.rgb_to_luma(colour), hypotheses=128, seed=5, **kw)
    chain = K.mosaic_chain(grey.model, grey.status, (96, 128), 0)
    SM.same(got.canvas, K.mosaic_median(colour, chain.from_anchor, grey.canvas.shape, grey.origin, chain.dropped), "colour: canvas")
    SM.same(got.count, grey.count, "colour: count")
