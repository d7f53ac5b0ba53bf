"""CPU tests of the exposure chain and the exposure-compensated mosaic (tests/mosaic_exposure_model.py), and of the 8-frame pan
under a changing exposure through the statements alone: photometric refinement -> chains -> compensated composite.  No GPU is
used; oflk_exposure_chain_host is host code and is held to its statement here.
"""
import functools

import numpy as np
import pytest

import align_model as AM
import align_photo_model as APM
import mosaic_exposure_model as MEM
import mosaic_model as MM

ANCHOR = 3


def steps(seed, S):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.6, 1.5, S), rng.uniform(-20, 20, S)], 1).astype(np.float32)


@pytest.mark.parametrize("anchor", [0, 3, 6])
def test_the_chain_takes_every_frame_to_the_anchors_exposure(anchor):
    T = 7
    photo = steps(1, T - 1)
    E = MEM.exposure_chain(photo, None, T, anchor)
    assert E.shape == (T, 2) and E[anchor].tolist() == [1.0, 0.0]
    v = np.empty(T)   # one grey value seen by every frame: v_{t+1} = g_t v_t + b_t
    v[0] = 100.0
    for t in range(T - 1):
        v[t + 1] = np.float64(photo[t, 0]) * v[t] + np.float64(photo[t, 1])
    assert np.abs(E[:, 0] * v + E[:, 1] - v[anchor]).max() < 1e-10
    # forwards from frame 0 to the anchor, then backwards over the same steps: (1, 0) to within rounding
    fwd = MEM.exposure_chain(photo, None, T, 0)
    back = MEM.exposure_chain(photo, None, T, anchor)
    eg = back[0, 0] * fwd[anchor, 0]
    eb = back[0, 0] * fwd[anchor, 1] + back[0, 1]
    assert abs(eg - 1.0) < 1e-14 and abs(eb) < 1e-11


def test_held_steps_count_as_no_change():
    T = 6
    photo = steps(2, T - 1)
    status = np.array([1, 1, 0, 1, 1], np.int32)
    E = MEM.exposure_chain(photo, status, T, 1)
    assert E[3].tobytes() == E[2].tobytes()
    free = photo.copy()
    free[2] = (1.0, 0.0)
    assert E.tobytes() == MEM.exposure_chain(free, None, T, 1).tobytes()
    for bad in ((0.0, 3.0), (-0.5, 3.0), (np.nan, 3.0), (1.2, np.nan), (np.inf, 0.0), (1.1, -np.inf)):
        p = photo.copy()
        p[2] = bad
        for anchor in (0, 5):
            assert MEM.exposure_chain(p, None, T, anchor).tobytes() == MEM.exposure_chain(free, None, T, anchor).tobytes(), bad
    assert MEM.exposure_chain(np.zeros((0, 2), np.float32), None, 1, 0).tolist() == [[1.0, 0.0]]


def test_the_host_function_equals_the_statement():
    import _oflk

    for T, anchor in ((1, 0), (2, 0), (2, 1), (7, 0), (7, 3), (7, 6)):
        photo = steps(T, T - 1)
        status = None
        if T == 7:
            photo[1] = (-1.0, 2.0)
            photo[4, 1] = np.nan
            status = np.array([1, 1, 1, 0, 1, 1], np.int32)
        got = _oflk.exposure_chain_host(photo, status, T, anchor)
        assert got.tobytes() == MEM.exposure_chain(photo, status, T, anchor).tobytes(), (T, anchor)
    for T, anchor in ((0, 0), (3, 3), (3, -1)):
        with pytest.raises(ValueError):
            _oflk.exposure_chain_host(steps(0, 2), None, T, anchor)


def test_the_python_function_checks_its_arguments():
    import lucas_kanade_core as K

    photo = steps(3, 4)
    got = K.exposure_chain(photo[:, 0], photo[:, 1], [1, 0, 1, 1], anchor=2)
    assert got.tobytes() == MEM.exposure_chain(photo, [1, 0, 1, 1], 5, 2).tobytes()
    for bad in (dict(anchor=5), dict(anchor=-1), dict(anchor=True), dict(status=[1, 1])):
        with pytest.raises(ValueError):
            K.exposure_chain(photo[:, 0], photo[:, 1], **bad)
    with pytest.raises(ValueError):
        K.exposure_chain(photo[:, 0], photo[:3, 1])


def test_a_unit_exposure_is_the_plain_composite_and_a_gain_scales_it():
    frames, maps = MM.pan_frames(MM.smooth_field(30, 60, 4), 4, 20, 33, 5, 1, 2, 3)
    frames = frames.astype(np.float32)
    unit = np.tile([1.0, 0.0], (4, 1))
    for blend in (MM.MEAN, MM.FEATHER, MM.FIRST, MM.LAST):
        plain = MM.composite(frames, maps, None, 0, 0, 30, 60, blend)
        got = MEM.composite(frames, maps, None, unit, 0, 0, 30, 60, blend, cuts=(1,))
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
        # a power of two is exact at every step
        twice = MEM.composite(frames, maps, [0, 1, 0, 0], np.tile([2.0, 0.0], (4, 1)), 0, 0, 30, 60, blend)
        want = MM.composite(frames, maps, [0, 1, 0, 0], 0, 0, 30, 60, blend)
        assert twice[0].tobytes() == (2 * want[0]).tobytes() and twice[1].tobytes() == want[1].tobytes()


@functools.lru_cache(maxsize=None)
def pan():
    """the 8-frame pan refined by both statements from the step models (-5 + 0.3, -0.2)"""
    frames, src, gains, biases = APM.pan_scene()
    model = np.stack([MM.translation(-5 + 0.3, -0.2).astype(np.float32)] * 7)
    return frames, src, gains, biases, APM.sequence(frames, model, None, AM.HOMOGRAPHY, 3, 4), \
        AM.sequence(frames, model, None, AM.HOMOGRAPHY, 3, 4)


def test_the_pan_recovers_the_planted_steps_and_gains(oracle):
    frames, src, gains, biases, photo, plain = pan()
    assert frames.min() >= 30 and frames.max() <= 195   # nothing clips
    assert (photo[1] == 1).all()
    E = MEM.exposure_chain(photo[3], photo[1], 8, ANCHOR)
    want = gains[ANCHOR] / gains
    tp = np.abs(photo[0][:, [2, 5]] - np.array([-5.0, 0.0], np.float32)).max()
    tq = np.abs(plain[0][:, [2, 5]] - np.array([-5.0, 0.0], np.float32)).max()
    print(f"translations within {tp:.4f} px (photometric), {tq:.4f} px (plain); chained gains within {np.abs(E[:, 0] - want).max():.4f}")
    assert np.abs(E[:, 0] - want).max() < 0.01
    assert tp < 0.05


@pytest.mark.parametrize("blend", [MM.MEAN, MM.FEATHER], ids=["mean", "feather"])
def test_the_compensated_pan_mosaic_is_four_times_nearer_the_source(oracle, blend):
    frames, src, gains, biases, photo, plain = pan()
    truth = gains[ANCHOR] * src + biases[ANCHOR]
    P, Q, box, held, dropped = MM.chain(photo[0], None, 8, ANCHOR, 96, 128, 8.0 * 128)
    x0, y0, Wc, Hc = MM.canvas(box, dropped)
    E = MEM.exposure_chain(photo[3], photo[1], 8, ANCHOR)
    f32 = frames.astype(np.float32)
    at = (4 + 5 * ANCHOR, 4)
    comp = MEM.source_error(*MEM.composite(f32, P, dropped, E, x0, y0, Hc, Wc, blend), (x0, y0), truth, at)
    unc = MEM.source_error(*MM.composite(f32, P, dropped, x0, y0, Hc, Wc, blend), (x0, y0), truth, at)
    print(f"blend {blend}: mean |mosaic - source| {unc[0]:.3f} -> {comp[0]:.3f} grey levels, worst {unc[1]:.2f} -> {comp[1]:.2f}")
    assert not dropped.any() and comp[0] <= unc[0] / 4.0
