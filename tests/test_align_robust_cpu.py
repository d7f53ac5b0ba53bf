"""CPU tests of the robust alignment statement (tests/align_robust_model.py): a delta above every residual is the base
statement, what the Huber weights reach on scenes with an object that moves on its own, the weight map, and the refusals of
the statement, of the library (decided on the host: no GPU is needed) and of the Python wrappers."""
import numpy as np
import pytest

import align_model as AM
import align_photo_model as APM
import align_robust_model as ARM
import align_robust_scenes as RS

KINDS = [("homography", AM.HOMOGRAPHY), ("affine", AM.AFFINE)]
L, N = 3, 5


def _base(pa, pb, m0, kind, photometric, iterations=N):
    if photometric:
        return APM.refine_pyramids(pa, pb, m0, 1, kind, iterations)
    return AM.refine_pyramids(pa, pb, m0, 1, kind, iterations) + (ARM.ONE.copy(),)


@pytest.mark.parametrize("photometric", [False, True], ids=["plain", "photometric"])
@pytest.mark.parametrize("name,kind", KINDS)
@pytest.mark.parametrize("H,W", [(33, 47), (70, 257)])
def test_a_delta_above_every_residual_is_the_base_statement(oracle, H, W, name, kind, photometric):
    """robust_delta = 3.0e38: every weight is exactly 1.0, w c = c and (r r) 0.5 is exact, so model, status and photo are the
    base statement's bytes, the squared-residual stats are its stats, the Huber stats exactly half of them, the mean weights 1.0"""
    A, B, planted = AM.planted_pair(H, W, 4, kind, move=2.0)
    if photometric:
        B = APM.exposed(B, 0.8, 12.0)
    m0 = AM.pushed(planted, H, W, kind, 0.5)
    pa, pb = AM.pyramids(A, L), AM.pyramids(B, L)
    want = _base(pa, pb, m0, kind, photometric, 3)
    got = ARM.refine_pyramids(pa, pb, m0, RS.NO_DELTA, 1, kind, 3, 0.25, photometric)
    assert want[1] == 1 and got[1] == want[1]
    assert got[0].tobytes() == want[0].tobytes() and got[3].tobytes() == want[3].tobytes()
    assert got[2].shape == (8,) and got[2][2:4].tobytes() == want[2][2:4].tobytes()
    assert got[2][4:6].tobytes() == want[2][0:2].tobytes()
    assert got[2][0:2].tobytes() == (want[2][0:2] * 0.5).tobytes()
    assert got[2][6:8].tolist() == [1.0, 1.0]
    # and at the level of the sums: the base statement's, then rho = half of r r and sum(w) = the count
    lv = AM.Level(pa[-1], pb[-1])
    m = [np.float64(c) for c in m0] + ([np.float64(0.0), np.float64(0.0), np.float64(1.0)] if kind == AM.AFFINE else [])
    S = ARM.sums_robust(lv, m, kind, ARM.check_delta(RS.NO_DELTA), photometric, 0.9, 3.0)
    base = APM.sums_photo(lv, m, kind, 0.9, 3.0) if photometric else AM.sums(lv, m, kind)
    assert len(S) == ARM.n_sums(kind, photometric) == len(base) + 2 and S[:-2].tobytes() == base.tobytes()
    assert S[-2] == base[-2] * 0.5 and S[-1] == base[-1]


def test_the_numbers_of_sums():
    assert [ARM.n_sums(k, p) for p in (False, True) for k in (AM.AFFINE, AM.HOMOGRAPHY)] == [31, 48, 48, 69]


CASES = [(H, W, seed, name, kind, exposure) for (H, W) in RS.SIZES for seed in RS.SEEDS for name, kind in KINDS
         for exposure in [None] + RS.EXPOSURES]


@pytest.mark.parametrize("H,W,seed,name,kind,exposure", CASES,
                         ids=[f"{W}x{H}-seed{s}-{n}-{'plain' if e is None else f'{e[0]}_{e[1]:+g}'}" for H, W, s, n, _, e in CASES])
def test_huber_weights_hold_the_fit_against_a_moving_object(oracle, H, W, seed, name, kind, exposure):
    """AM.planted_pair with a textured rectangle of 12 % of the frame pasted into A and, 3 rows lower and 7 columns further
    right, into B; start AM.pushed(planted, 1.0) (corner error about 1.05 px), L = 3, n = 5, delta = 4 grey levels.  exposure
    None: the plain statement against align_model; otherwise B re-exposed after the paste and the photometric statement
    against align_photo_model.  Every robust result: status 1, corner error <= 0.15 px and <= a quarter of the base
    statement's on the same pair.

    Measured over these 48 cases: plain base 0.366 - 2.233 px, robust 0.014 - 0.092 px, worst ratio 0.113; photometric base
    0.329 - 1.883 px, robust 0.016 - 0.126 px, worst ratio 0.181 (the largest error at 130x96, seed 3, homography, (0.7, +20);
    the largest ratio at 130x96, seed 2, (0.7, +20)).  With seed k re-exposed by the k-th exposure only the photometric robust
    errors are 0.016 - 0.082 px and the worst ratio 0.094.  On the (0.7, +20) cases of seed 1 the photometric base statement
    estimates a gain of 0.56, the robust one 0.68."""
    A, B, planted = RS.moving_object_pair(H, W, seed, kind, exposure)
    m0 = AM.pushed(planted, H, W, kind, 1.0)
    pa, pb = AM.pyramids(A, L), AM.pyramids(B, L)
    photometric = exposure is not None
    base = _base(pa, pb, m0, kind, photometric)
    got = ARM.refine_pyramids(pa, pb, m0, RS.DELTA, 1, kind, N, 0.25, photometric)
    eb, er = AM.corner_error(base[0], planted, H, W), AM.corner_error(got[0], planted, H, W)
    print(f"{W}x{H} seed {seed} {name} exposure {exposure}: base status {base[1]} corner error {eb:.4f} px, robust status {got[1]} "
          f"{er:.4f} px (ratio {er / eb:.3f}), photo base {base[3]} robust {got[3]}, stats {got[2]}")
    assert base[1] == 1 and got[1] == 1
    assert er <= 0.15
    assert er <= 0.25 * eb
    assert got[2][1] <= got[2][0] and got[2][3] == L * N and 0.0 < got[2][7] < 1.0


@pytest.mark.parametrize("name,kind", KINDS)
def test_the_weight_map_marks_the_object(oracle, name, kind):
    """weights under the robustly refined model, delta = 4, 130 x 96, seed 1: the mean over the object's rectangle in A lies
    below the mean over the rest of the frame.  Measured: homography 0.223 against 0.957, affine 0.217 against 0.946; with
    B re-exposed by (0.7, +20) and the refined gain and bias, homography 0.296 against 0.959, affine 0.286 against 0.949.
    Over all 48 cases of the test above the object's mean is 0.153 - 0.331 and the rest's 0.912 - 0.961.  The bound: the
    object's mean below half of the rest's."""
    H, W = RS.SIZES[0]
    y, x, oh, ow = RS.object_box(H, W)
    mask = np.zeros((H, W), bool)
    mask[y:y + oh, x:x + ow] = True
    for exposure in (None, RS.EXPOSURES[0]):
        A, B, planted = RS.moving_object_pair(H, W, 1, kind, exposure)
        photometric = exposure is not None
        got = ARM.refine(A[None], B[None], AM.pushed(planted, H, W, kind, 1.0)[None], RS.DELTA, None, kind, L, N, 0.25, photometric)
        gb = (got[3][0, 0], got[3][0, 1]) if photometric else ()
        w = ARM.weights(A, B, got[0][0], kind, RS.DELTA, *gb)
        obj, rest = float(w[mask].mean()), float(w[~mask].mean())
        print(f"{name} exposure {exposure}: mean weight {obj:.3f} on the object, {rest:.3f} elsewhere")
        assert w.dtype == np.float32 and w.shape == (H, W) and w.min() >= 0.0 and w.max() == 1.0
        assert obj < 0.5 * rest
        # the map's mean over the counted pixels is stats[7], which sums the same weights in float64
        counted = w > 0
        assert abs(float(w[counted].astype(np.float64).mean()) - got[2][0, 7]) < 1e-6
    # a model that throws B off the frame: nothing is counted
    off = AM.IDENTITY[kind].copy()
    off[2] = 4.0 * W
    assert not ARM.weights(A, B, off, kind, RS.DELTA).any()


@pytest.mark.parametrize("photometric", [False, True], ids=["plain", "photometric"])
@pytest.mark.parametrize("name,kind", KINDS)
def test_refused_steps_come_back_as_they_went_in_with_eight_zeros(oracle, name, kind, photometric):
    H, W = 40, 56
    A, B, planted = AM.planted_pair(H, W, 2, kind, move=1.0)
    m0 = AM.pushed(planted, H, W, kind, 0.5)
    bad = m0.copy()
    bad[len(bad) - 2] = np.nan
    inf = m0.copy()
    inf[0] = np.inf
    a, b = np.stack([A] * 4), np.stack([B] * 4)
    model, status = np.stack([m0, m0, bad, inf]), np.array([1, 0, 1, 1], np.int32)
    out, st, stats, photo = ARM.refine(a, b, model, RS.DELTA, status, kind, 2, 2, 0.25, photometric)
    assert st.tolist() == [1, 0, 0, 0] and stats.shape == (4, 8) and photo.shape == (4, 2)
    for s in (1, 2, 3):
        assert out[s].tobytes() == model[s].tobytes() and not stats[s].any() and stats[s].tobytes() == np.zeros(8).tobytes()
        assert photo[s].tobytes() == ARM.ONE.tobytes()
    assert out[0].tobytes() != m0.tobytes() and stats[0, 3] == 4
    # a frozen step (a flat template) and a thrown one keep the model too, with stats that say why
    flat = np.full((H, W), 7.0, np.float32)
    off = AM.IDENTITY[kind].copy()
    off[2] = 4.0 * W
    out, st, stats, photo = ARM.refine(np.stack([flat, A]), np.stack([B, B]), np.stack([m0, off]), RS.DELTA, None, kind, 2, 2, 0.25,
                                       photometric)
    assert st.tolist() == [0, 0] and out[0].tobytes() == m0.tobytes() and out[1].tobytes() == off.tobytes()
    assert stats[0, 3] == 0 and stats[0, 2] > 0.9 and stats[1, 2] == 0 and np.isnan(stats[1, [0, 1, 4, 5, 6, 7]]).all()
    assert photo.tobytes() == np.stack([ARM.ONE, ARM.ONE]).tobytes()


def test_a_rejected_step_is_judged_on_the_huber_loss(oracle):
    """align_model.checker_pair: the refinement turns the checkerboard over.  The squared residual grows from 1 to above
    1000 and the Huber loss from 0.5 (every |r| = 1 <= delta) to above delta 0.5 of it: status 2 and the input model"""
    ca, cb = AM.checker_pair(40, 56)
    for kind in (AM.HOMOGRAPHY, AM.AFFINE):
        out, st, stats, photo = ARM.refine_pyramids(AM.pyramids(ca, 1), AM.pyramids(cb, 1), AM.IDENTITY[kind], RS.DELTA, 1, kind, 1)
        assert st == 2 and out.tobytes() == AM.IDENTITY[kind].tobytes() and photo.tobytes() == ARM.ONE.tobytes()
        assert stats[0] == 0.5 and stats[4] == 1.0 and stats[6] == 1.0 and stats[3] == 1
        assert stats[1] > stats[0] and stats[5] > 1000.0 and stats[7] < 1.0


def test_the_sequence_form_is_the_pair_form(oracle):
    frames = APM.pan_scene(5, 48, 70, 3, 11)[0]
    model = np.stack([AM.IDENTITY[AM.AFFINE]] * 4)
    model[:, 2] = -2.5
    status = np.array([1, 0, 1, 1], np.int32)
    for photometric in (False, True):
        seq = ARM.sequence(frames, model, RS.DELTA, status, AM.AFFINE, 2, 2, 0.25, photometric)
        ARM.same(ARM.refine(frames[:-1], frames[1:], model, RS.DELTA, status, AM.AFFINE, 2, 2, 0.25, photometric), seq, "pair form")
        assert seq[1].tolist() == [1, 0, 1, 1]


BAD_DELTAS = [0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e39, 1e-50]   # the last two: inf and 0 as float32


def test_the_statement_refuses_a_delta_that_is_not_finite_and_positive():
    for bad in BAD_DELTAS:
        with pytest.raises(ValueError):
            ARM.check_delta(bad)
    assert ARM.check_delta(4.0) == 4.0 and ARM.check_delta(0.1) == np.float64(np.float32(0.1))


def test_the_library_refuses_before_any_device_call():
    """every refusal is decided on the host: this runs without a GPU, with pointers that are never dereferenced"""
    import _oflk

    Lb = _oflk.lib()
    P, WS = 0x10000, 0x20000   # 8-byte and 256-byte aligned addresses, never read
    big = 1 << 40
    INVALID, UNSUPPORTED = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED
    c_bad = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]

    def refine(a=P, b=P, u8=0, S=2, H=16, W=16, levels=2, iterations=2, model=1, min_share=0.25, delta=4.0, photometric=0, m_in=P,
               s_in=None, ws=WS, nbytes=big, m_out=P, s_out=P, stats=P, photo=None):
        return Lb.oflk_align_refine_robust(a, b, u8, S, H, W, levels, iterations, model, min_share, delta, photometric, m_in, s_in, ws,
                                           nbytes, m_out, s_out, stats, photo, None)

    def sequence(frames=P, u8=0, T=3, H=16, W=16, levels=2, iterations=2, model=1, min_share=0.25, delta=4.0, photometric=0, m_in=P,
                 s_in=None, ws=WS, nbytes=big, m_out=P, s_out=P, stats=P, photo=None):
        return Lb.oflk_align_sequence_robust(frames, u8, T, H, W, levels, iterations, model, min_share, delta, photometric, m_in, s_in,
                                             ws, nbytes, m_out, s_out, stats, photo, None)

    for call in (refine, sequence):
        for d in c_bad:
            assert call(delta=d) == INVALID and b"robust_delta" in Lb.oflk_last_error(), d
            assert call(delta=d, photometric=1, photo=P) == INVALID
        assert call(photometric=1) == INVALID and b"d_photo_out" in Lb.oflk_last_error()
        assert call(photometric=1, photo=P + 2) == INVALID
        for kw in [dict(H=0), dict(W=0), dict(levels=0), dict(levels=99), dict(iterations=0), dict(model=2), dict(min_share=0.0),
                   dict(min_share=1.5), dict(m_in=None), dict(ws=None), dict(m_out=None), dict(s_out=None), dict(stats=None),
                   dict(ws=WS + 128), dict(stats=P + 4), dict(nbytes=0)]:
            assert call(**kw) == INVALID, kw
        assert call(levels=3) == UNSUPPORTED   # 16 x 16 at three levels: a level of 4 x 4
    assert refine(S=0) == INVALID and refine(a=None) == INVALID and refine(b=None) == INVALID and refine(a=P + 2) == INVALID
    assert sequence(T=1) == INVALID and sequence(frames=None) == INVALID

    # the workspace: larger than the base form's by the two sums and the first pass's two values
    for model in (0, 1):
        for photometric in (False, True):
            base = _oflk.align_workspace(3, 70, 257, 3, model, photometric)
            assert _oflk.align_workspace(3, 70, 257, 3, model, photometric, robust=True) > base
            need = _oflk.align_workspace(2, 16, 16, 2, model, photometric, robust=True)
            kw = dict(model=model, photometric=int(photometric), photo=P if photometric else None)
            assert refine(nbytes=need - 1, **kw) == INVALID and b"workspace" in Lb.oflk_last_error()
    n = _oflk.ctypes.c_size_t(7)
    assert Lb.oflk_align_robust_workspace(0, 16, 16, 2, 1, 0, _oflk.ctypes.byref(n)) == INVALID and n.value == 0
    assert Lb.oflk_align_robust_workspace(2, 16, 16, 2, 1, 0, None) == INVALID
    assert Lb.oflk_align_robust_workspace(2, 16, 16, 3, 1, 1, _oflk.ctypes.byref(n)) == UNSUPPORTED

    # the host forms
    fr = np.zeros((3, 16, 16), np.float32)
    f8 = np.zeros((3, 16, 16), np.uint8)
    m = np.zeros((2, 9), np.float32)
    st, stats, photo = np.zeros(2, np.int32), np.zeros((2, 8)), np.zeros((2, 2), np.float32)
    i32, f64 = st.ctypes.data_as(_oflk._i32p), _oflk._f64(stats)
    for fn, pa, seq in ((Lb.oflk_align_refine_robust_host, _oflk.ptr(fr), False), (Lb.oflk_align_refine_robust_host_u8, f8.ctypes.data, False),
                        (Lb.oflk_align_sequence_robust_host, _oflk.ptr(fr), True), (Lb.oflk_align_sequence_robust_host_u8, f8.ctypes.data, True)):
        def host(n=2, H=16, levels=2, iterations=2, delta=4.0, photometric=0, m_in=_oflk.ptr(m), out=_oflk.ptr(m), po=None):
            head = (pa, n + 1) if seq else (pa, pa, n)
            return fn(*head, H, 16, levels, iterations, 1, 0.25, delta, photometric, m_in, None, out, i32, f64, po)

        for d in c_bad:
            assert host(delta=d) == INVALID and b"robust_delta" in Lb.oflk_last_error(), d
        assert host(photometric=1) == INVALID
        for kw in [dict(n=0), dict(H=0), dict(levels=0), dict(iterations=0), dict(m_in=None), dict(out=None)]:
            assert host(**kw) == INVALID, kw
        assert host(levels=3) == UNSUPPORTED

    # the weight map
    def weights(a=P, b=P, u8=0, S=2, H=16, W=16, model=1, delta=4.0, m_in=P, photo=None, out=P):
        return Lb.oflk_align_weights(a, b, u8, S, H, W, model, delta, m_in, photo, out, None)

    for d in c_bad:
        assert weights(delta=d) == INVALID and b"robust_delta" in Lb.oflk_last_error(), d
    for kw in [dict(S=0), dict(H=0), dict(W=-1), dict(model=7), dict(a=None), dict(b=None), dict(m_in=None), dict(out=None),
               dict(a=P + 2), dict(out=P + 2), dict(photo=P + 2), dict(m_in=P + 1)]:
        assert weights(**kw) == INVALID, kw
    assert weights(H=1 << 15, W=1 << 15) == UNSUPPORTED
    w = np.zeros((2, 16, 16), np.float32)
    for fn, pa in ((Lb.oflk_align_weights_host, _oflk.ptr(fr)), (Lb.oflk_align_weights_host_u8, f8.ctypes.data)):
        for d in c_bad:
            assert fn(pa, pa, 2, 16, 16, 1, d, _oflk.ptr(m), None, _oflk.ptr(w)) == INVALID
        assert fn(pa, pa, 0, 16, 16, 1, 4.0, _oflk.ptr(m), None, _oflk.ptr(w)) == INVALID
        assert fn(pa, pa, 2, 16, 16, 3, 4.0, _oflk.ptr(m), None, _oflk.ptr(w)) == INVALID
        assert fn(None, pa, 2, 16, 16, 1, 4.0, _oflk.ptr(m), None, _oflk.ptr(w)) == INVALID
        assert fn(pa, pa, 2, 16, 16, 1, 4.0, None, None, _oflk.ptr(w)) == INVALID
        assert fn(pa, pa, 2, 16, 16, 1, 4.0, _oflk.ptr(m), None, None) == INVALID


def test_the_python_wrappers_refuse_before_any_device_call():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    a = np.zeros((16, 16), np.float32)
    eye = np.eye(3, dtype=np.float32)
    frames = np.zeros((3, 16, 16), np.float32)
    for bad in BAD_DELTAS + ["4", True, [4.0]]:
        with pytest.raises(ValueError, match="robust_delta"):
            K.refine_alignment(a, a, eye, robust_delta=bad)
        with pytest.raises(ValueError, match="robust_delta"):
            K.sequence_refine_alignment(frames, np.stack([eye] * 2), robust_delta=bad, photometric=True)
        with pytest.raises(ValueError, match="robust_delta"):
            K.alignment_weights(a, a, eye, robust_delta=bad)
    with pytest.raises(ValueError, match="gain and bias"):
        K.alignment_weights(a, a, eye, gain=1.0)
    with pytest.raises(ValueError, match="gain and bias"):
        K.alignment_weights(frames, frames, np.stack([eye] * 3), gain=[1.0, 1.0], bias=[0.0, 0.0])
    with pytest.raises(ValueError, match="kind"):
        K.alignment_weights(a, a, eye, kind="similarity")
    with pytest.raises(ValueError):
        K.alignment_weights(a, frames, eye)
    with pytest.raises(ValueError):
        K.alignment_weights(a, a, np.zeros((2, 3), np.float32))   # an affine model for kind "homography"
    u8 = np.zeros((3, 16, 16), np.uint8)
    nv12 = np.zeros((3, 24, 16), np.uint8)
    for call in (lambda: P.lucas_kanade_pyramidal_sequence_stabilize(u8, 10, 2, refine_robust_delta=4.0),
                 lambda: P.lucas_kanade_pyramidal_sequence_stabilize_nv12(nv12, 10, 2, refine_robust_delta=4.0),
                 lambda: P.lucas_kanade_pyramidal_sequence_mosaic(u8, refine_robust_delta=4.0)):
        with pytest.raises(ValueError, match="refine_robust_delta needs refine_iterations > 0"):
            call()
    assert K.RobustAlignment._fields == ("model", "status", "stats", "gain", "bias")
