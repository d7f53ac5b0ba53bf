"""CPU tests of the temporal-median mosaic: the statement (tests/mosaic_median_model.py) against np.median, its own order and
the existing blends' statement; the mover scene, where the median gives the clean plate and the mean and the feather do not; and
what the library and the Python wrappers export and refuse without a device.  No GPU is used."""
import ctypes

import numpy as np
import pytest

import mosaic_median_model as MD
import mosaic_model as MM
import stabilize_model as SM


def _scene(F, H, W, Hc, Wc, x0, y0, dtype, seed):
    """F frames of noise under sub-pixel translations that walk over the canvas, one perspective map among them"""
    rng = np.random.default_rng(seed)
    f = 20.0 + 200.0 * rng.random((F, H, W))
    frames = np.rint(f).astype(np.uint8) if dtype == np.uint8 else (f - 100.0).astype(np.float32)
    maps = np.stack([MM.translation(-(x0 - 2.25 + 2.37 * k), -(y0 - 1.5 + 0.71 * k)) for k in range(F)])
    maps[F // 2] = [0.9, 0.05, -0.9 * x0 + 1, -0.04, 1.1, -1.1 * y0 + 2, 1e-3, -1e-3, 1.0]
    skip = np.zeros(F, np.uint8)
    skip[1] = 1
    exposure = np.stack([rng.uniform(0.6, 1.5, F), rng.uniform(-20, 20, F)], 1)
    return frames, maps, skip, exposure


def test_the_model_is_np_median_on_finite_samples():
    frames, maps, skip, exposure = _scene(9, 9, 13, 19, 40, -3, 2, np.float32, 0)
    for ex in (None, exposure):
        out, count = MD.median(frames, maps, skip, -3, 2, 19, 40, ex)
        e, inside = MD.samples(frames, maps, skip, ex, -3, 2, 19, 40)
        assert count.max() >= 4 and (count == 0).any() and {0, 1} <= set((count % 2).ravel().tolist())
        assert not ((e == 0) & inside).any(), "no zeros, so no mixed signed zeros"
        want = np.zeros((19, 40), np.float32)
        for y, x in np.ndindex(19, 40):
            if count[y, x]:
                want[y, x] = np.float32(np.median(e[:, y, x][inside[:, y, x]].astype(np.float64)))
                assert MD.select(e[:, y, x][inside[:, y, x]]).tobytes() == out[y, x].tobytes()
        SM.same(out, want, "the model against np.median")


def test_the_key_order():
    v = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.0], np.float32)
    v[0], v[1] = np.uint32(0x7FC00000).view(np.float32), np.uint32(0xFFC00000).view(np.float32)   # the signs, whatever -nan parses to
    got = MD.unkey(np.sort(MD.key(v)))
    want = np.array([0xFFC00000, 0xFF800000, 0xC0000000, 0x80000000, 0x00000000, 0x3FC00000, 0x7F800000, 0x7FC00000], np.uint32)
    assert got.view(np.uint32).tolist() == want.tolist()   # -NaN < -inf < -2 < -0 < +0 < 1.5 < +inf < +NaN
    SM.same(MD.unkey(MD.key(v)), v, "the key is a bijection")
    assert np.isnan(MD.select(v[[2, 3]])) and MD.select(v[[3, 6, 2]]) == np.float32(1.5)   # inf + -inf;  -inf < 1.5 < inf
    assert MD.select(v[[4, 5]]).tobytes() == np.float32(0.0).tobytes() and MD.select(v[:0]) == 0
    assert MD.select(np.array([254, 255], np.float32)) == np.float32(254.5) and MM.saturate(np.float32(254.5)) == 254


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_a_frame_permutation_does_not_change_a_byte_and_the_count_is_the_blends(dtype):
    frames, maps, skip, exposure = _scene(8, 9, 13, 19, 40, -3, 2, dtype, 1)
    if dtype == np.float32:
        frames[2, 0, 0], frames[3, 0, 0], frames[4, 0, 0] = np.nan, -np.inf, -0.0
    for ex in (None, exposure):
        out, count = MD.median(frames, maps, skip, -3, 2, 19, 40, ex)
        p = np.random.default_rng(5).permutation(8)
        got = MD.median(frames[p], maps[p], skip[p], -3, 2, 19, 40, None if ex is None else ex[p])
        SM.same(got[0], out, "permuted: canvas")
        SM.same(got[1], count, "permuted: count")
        SM.same(count, MM.composite(frames, maps, skip, -3, 2, 19, 40, MM.MEAN)[1], "count against the blends'")
    for f in range(8):   # one frame: its own samples, which is the last blend's canvas
        one = MD.median(frames[f:f + 1], maps[f:f + 1], None, -3, 2, 19, 40)
        last = MM.composite(frames[f:f + 1], maps[f:f + 1], None, -3, 2, 19, 40, MM.LAST)
        SM.same(one[0], last[0], f"F = 1, frame {f}: canvas")
        SM.same(one[1], last[1], f"F = 1, frame {f}: count")


def test_the_median_of_the_mover_scene_is_the_source_where_five_frames_cover():
    img, frames, maps = MD.mover_scene()
    Hc, Wc = 48, 154
    med, count = MD.median(frames, maps, None, 0, 0, Hc, Wc)
    src = img[:Hc, :Wc]
    often = count >= 5
    print(f"covered by >= 5 frames: {often.sum()} of {often.size} ({often.mean():.3f})")
    assert often.mean() >= 0.68
    assert (med[often] == src[often]).all()
    for name, blend in (("median", None), ("mean", MM.MEAN), ("feather", MM.FEATHER)):
        out = med if blend is None else MM.composite(frames, maps, None, 0, 0, Hc, Wc, blend)[0]
        d = np.abs(out.astype(np.float64) - src)
        wrong = int((out[often] != src[often]).sum())
        print(f"{name}: mean |mosaic - source| {d.mean():.2f} grey levels, {d[often].mean():.2f} where >= 5 frames cover, {wrong} pixels differ there")
        assert blend is None or wrong > 1000
    assert (count[med != src] <= 4).all()


# ---------------------------------------------------------------------------------------------------------------------
# the C layer and the wrappers without a device
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ["oflk_mosaic_median_capacity", "oflk_mosaic_median", "oflk_mosaic_median_host", "oflk_mosaic_median_host_u8"]


def test_the_symbols_are_exported_declared_and_signed():
    import _oflk
    from test_abi import declared_functions

    L = _oflk.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _oflk.SIGNATURES and name in declared_functions(), name
    assert _oflk.mosaic_median_capacity() >= 1
    assert _oflk.SIGNATURES["oflk_mosaic_median_capacity"][1] == []


def test_refusals_come_before_any_device_call():
    """every refusal is decided on the host: this runs without a GPU, with pointers that are never dereferenced"""
    import _oflk

    L = _oflk.lib()
    P = 0x10000   # an 8-byte aligned address, never read
    INVALID, UNSUPPORTED = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED

    def device(frames=P, u8=0, F=3, H=8, W=8, m=P, skip=None, ex=None, x0=0, y0=0, Hc=20, Wc=30, out=P, count=None):
        return L.oflk_mosaic_median(frames, u8, F, H, W, m, skip, ex, x0, y0, Hc, Wc, out, count, None)

    def host(name):
        sig = _oflk.SIGNATURES[name][1]

        def cast(v, t):
            return v if v is None or t is ctypes.c_void_p else ctypes.cast(v, t)

        def call(frames=P, F=3, H=8, W=8, m=P, skip=None, ex=None, x0=0, y0=0, Hc=20, Wc=30, out=P, count=None):
            return getattr(L, name)(cast(frames, sig[0]), F, H, W, cast(m, sig[4]), skip, cast(ex, sig[6]), x0, y0, Hc, Wc,
                                    cast(out, sig[11]), count)
        return call

    cases = [(dict(F=0), INVALID), (dict(F=-1), INVALID), (dict(H=1), INVALID), (dict(W=1), INVALID), (dict(Hc=0), INVALID),
             (dict(Wc=0), INVALID), (dict(frames=None), INVALID), (dict(m=None), INVALID), (dict(out=None), INVALID),
             (dict(m=P + 4), INVALID), (dict(ex=P + 4), INVALID), (dict(Hc=1 << 15, Wc=1 << 15), UNSUPPORTED),
             (dict(H=1 << 15, W=1 << 15), UNSUPPORTED)]
    for fn in (device, host("oflk_mosaic_median_host"), host("oflk_mosaic_median_host_u8")):
        for kw, code in cases:
            assert fn(**kw) == code, kw
            assert L.oflk_last_error(), kw
    assert device(frames=P + 2) == INVALID and device(frames=P + 2, u8=1, Hc=0) == INVALID
    # the existing codes stay: the accumulate has no fifth blend
    assert L.oflk_mosaic_accumulate(P, 0, 3, 8, 8, P, None, 0, 0, 20, 30, 4, 0x20000, 1 << 30, None) == INVALID
    assert b"blend" in L.oflk_last_error()


def test_the_python_refusals_come_from_the_shared_helpers():
    import _oflk
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    assert P.mosaic_median is K.mosaic_median
    fr = np.zeros((2, 6, 7), np.float32)
    maps = np.tile(np.eye(3), (2, 1, 1))
    for kw in [dict(maps=maps[:1]), dict(maps=np.zeros((2, 5))), dict(maps=np.zeros((2, 2, 3))), dict(canvas_shape=(0, 7)),
               dict(canvas_shape=(6,)), dict(canvas_shape=(1 << 15, 1 << 15)), dict(origin=(0.5, 0)), dict(origin=(0,)),
               dict(origin=(True, 0)), dict(origin=(2 ** 31, 0)), dict(skip=np.zeros(3)), dict(exposure=np.zeros((3, 2))),
               dict(exposure=np.zeros(2)), dict(frames=fr[:, :1]), dict(frames=fr[:, :, :1]), dict(frames=np.zeros((2, 2, 6, 7))),
               dict(frames=np.zeros((2, 6, 7, 3), np.float32)), dict(frames=np.zeros((2, 6, 7, 2), np.uint8)),
               dict(frames=np.zeros((2, 2, 2, 6, 7)))]:
        args = dict(frames=fr, maps=maps, canvas_shape=(6, 7))
        args.update(kw)
        with pytest.raises(ValueError):
            K.mosaic_median(**args)
    with pytest.raises(TypeError):
        K.mosaic_median(fr, maps, (6, 7), blend="mean")   # the median is no blend
    # the same words as mosaic_composite's
    for kw in [dict(canvas_shape=(0, 7)), dict(origin=(0.5, 0)), dict(skip=np.zeros(3)), dict(exposure=np.zeros((3, 2))), dict(maps=maps[:1])]:
        said = []
        for fn in (K.mosaic_median, K.mosaic_composite):
            args = dict(frames=fr, maps=maps, canvas_shape=(6, 7))
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            said.append(str(e.value))
        assert said[0] == said[1], kw
    with pytest.raises(ValueError, match=r"blend must be one of \['feather', 'first', 'last', 'mean'\]"):
        K.mosaic_composite(fr, maps, (6, 7), blend="median")
    seq = np.zeros((3, 32, 32), np.uint8)
    for kw in [dict(anchor=3), dict(anchor=-1), dict(anchor=0.5), dict(extent=0), dict(max_pixels=0), dict(max_pixels=2.5),
               dict(refine_iterations=-1), dict(refine_photometric=True), dict(refine_robust_delta=4.0), dict(order="gbr"),
               dict(frames=seq[:1]), dict(frames=seq.astype(np.float64)[0]), dict(frames=seq[:, :1]), dict(num_levels=0),
               dict(hypotheses=0), dict(frames=np.zeros((3, 32, 32, 3), np.float32)), dict(frames=np.zeros((3, 32, 32, 2), np.uint8))]:
        args = dict(frames=seq)
        args.update(kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_mosaic_median(**args)
    with pytest.raises(ValueError, match="max_pixels must be an integer >= 1"):
        P.lucas_kanade_pyramidal_sequence_mosaic_median(seq, max_pixels=0)
    with pytest.raises(ValueError, match="refine_photometric needs refine_iterations > 0"):
        P.lucas_kanade_pyramidal_sequence_mosaic_median(seq, refine_photometric=True)
    import inspect

    a = inspect.signature(P.lucas_kanade_pyramidal_sequence_mosaic).parameters
    b = inspect.signature(P.lucas_kanade_pyramidal_sequence_mosaic_median).parameters
    assert [(n, p.default) for n, p in a.items() if n != "blend"] == [(n, p.default) for n, p in b.items()]
    assert _oflk.check_mosaic_canvas((6, 7), (-2, 3)) == (6, 7, -2, 3)
