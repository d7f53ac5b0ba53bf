"""CPU tests of video stabilisation: the statement (tests/stabilize_model.py) and its exact properties, the chain of CPU
statements end to end on jittered scenes, and what the product declares and refuses before any device call.  No GPU."""
import ctypes

import numpy as np
import pytest

import motion_model as MM
import stabilize_model as SM


def _bits_identity(corr):
    want = np.tile(SM.IDENTITY.astype(np.float32), (len(corr), 1))
    return corr.dtype == np.float32 and bool((corr.view(np.uint32) == want.view(np.uint32)).all())


def _is_identity(mp):
    return mp.dtype == np.float64 and np.array_equal(mp, np.tile(SM.IDENTITY, (len(mp), 1)))


# ---------------------------------------------------------------------------------------------------------------------
# the model's exact properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(3, -2), (1, 0), (-7, 5)])
def test_a_constant_integer_translation_is_left_alone_on_every_frame(shift):
    """forward then backward inside each i: w_i * (i s) + w_i * (-i s) cancels exactly, and acc00 and ws take the same sums.
    correction is the identity bit for bit; the stated inverse of the identity carries -0.0 (-a01 / det), so map equals it
    as values"""
    T = 12
    model = np.tile(np.float32([1, 0, shift[0], 0, 1, shift[1]]), (T - 1, 1))
    for r, sigma in [(3, None), (3, 0.8), (5, None), (64, None)]:
        corr, mp, held = SM.trajectory(model, None, T, SM.weights(r, sigma))
        assert _bits_identity(corr) and _is_identity(mp) and not held.any(), (r, sigma)


def test_radius_zero_is_the_identity_for_any_models():
    for fam in (MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE):
        model = SM.noisy_models(9, fam, 3)
        corr, mp, held = SM.trajectory(model, None, 10, SM.weights(0))
        assert _bits_identity(corr) and _is_identity(mp) and not held.any()


def test_a_held_step_behaves_exactly_as_an_identity_step():
    T = 9
    model = SM.noisy_models(T - 1, MM.AFFINE, 5)
    counts = np.tile(np.int32([10, 12, 1]), (T - 1, 1))
    ident = np.float32([1, 0, 0, 0, 1, 0])
    w = SM.weights(3)
    for s, how in [(0, "status"), (3, "nan"), (4, "inf"), (6, "zero"), (7, "singular")]:
        m, c = model.copy(), counts.copy()
        if how == "status":
            c[s, 2] = 0
        elif how == "nan":
            m[s, 2] = np.nan
        elif how == "inf":
            m[s, 0] = np.inf
        elif how == "zero":
            m[s] = 0
        else:
            m[s] = np.float32([2, 4, 1, 1, 2, 3])
        want_m = model.copy()
        want_m[s] = ident
        got, want = SM.trajectory(m, c, T, w), SM.trajectory(want_m, counts, T, w)
        SM.same(got[0], want[0], how)
        SM.same(got[1], want[1], how)
        assert got[2].tolist() == [int(i == s) for i in range(T - 1)] and not want[2].any(), how
    # without counts the status decides nothing
    c = counts.copy()
    c[2, 2] = 0
    assert SM.trajectory(model, c, T, w)[2][2] == 1 and not SM.trajectory(model, None, T, w)[2].any()


def test_one_and_two_frames():
    w = SM.weights(3)
    corr, mp, held = SM.trajectory(None, None, 1, w)
    assert corr.shape == (1, 6) and mp.shape == (1, 6) and held.shape == (0,) and _bits_identity(corr) and _is_identity(mp)
    corr, mp, held = SM.trajectory(SM.noisy_models(1, MM.SIMILARITY, 1), None, 2, w)
    assert corr.shape == (2, 6) and held.tolist() == [0] and _bits_identity(corr) and _is_identity(mp)


@pytest.mark.parametrize("T,r", [(3, 1), (7, 3), (8, 64), (20, 4)])
def test_the_window_is_clipped_symmetrically(T, r):
    model = SM.noisy_models(T - 1, MM.SIMILARITY, T)
    w = SM.weights(r)
    corr, mp, _ = SM.trajectory(model, None, T, w)
    assert _bits_identity(corr[[0, -1]]) and _is_identity(mp[[0, -1]]), "frames 0 and T-1 are never moved"
    assert not _bits_identity(corr[1:2]), "frame 1 is"
    # frame t sees the steps t - r_t .. t + r_t - 1 only: a cut of exactly that stretch gives the same frame
    for t in range(1, T - 1):
        rt = min(r, t, T - 1 - t)
        sub = SM.trajectory(model[t - rt:t + rt], None, 2 * rt + 1, w[:rt + 1])
        SM.same(sub[0][rt], corr[t], f"frame {t}")
        SM.same(sub[1][rt], mp[t], f"frame {t}")


def test_the_map_inverts_the_correction():
    for fam in (MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE):
        corr, mp, _ = SM.trajectory(SM.noisy_models(29, fam, 7), None, 30, SM.weights(8))
        for t in range(30):
            assert np.abs(SM.compose(mp[t], corr[t].astype(np.float64)) - SM.IDENTITY).max() <= 1e-12
            assert np.abs(SM.compose(corr[t].astype(np.float64), mp[t]) - SM.IDENTITY).max() <= 1e-12


def test_a_correction_that_cannot_be_inverted_is_the_identity():
    big = np.tile(np.float32([1, 0, 3e38, 0, 1, 0]), (4, 1))       # the mean's translation overflows float32 on frame 2
    big[:2, 2] = -3e38
    corr, mp, held = SM.trajectory(big, None, 5, np.array([1e-300, 1.0, 1.0]))
    assert not held.any() and _bits_identity(corr) and _is_identity(mp)


def test_the_warp_model_is_map_coordinates_and_rounds_half_to_even():
    from track_model import sample

    rng = np.random.default_rng(2)
    f = (rng.random((1, 9, 11)) * 255).astype(np.float32)
    th = np.deg2rad(30.0)
    m = np.array([np.cos(th), -np.sin(th), 2.0, np.sin(th), np.cos(th), -1.5])
    out, ins = SM.warp(f, m[None])
    xs, ys = SM.coordinates(m, 9, 11)
    assert np.array_equal(out[0], sample(f[0], xs.ravel(), ys.ravel()).reshape(9, 11)), "cval 0 outside is map_coordinates' own"
    assert 0 < ins.sum() < ins.size and (out[0][ins[0] == 0] == 0).all()
    b = np.uint8([[1, 2, 3, 2, 0], [1, 2, 3, 2, 0]])
    out, ins = SM.warp(b[None], np.array([[1, 0, 0.5, 0, 1, 0.0]]))
    assert out[0, 0].tolist() == [2, 2, 2, 1, 0] and ins[0, 0].tolist() == [1, 1, 1, 1, 0], "1.5 -> 2, 2.5 -> 2, 2.5 -> 2, 1.0"
    out, ins = SM.warp(b[None], np.array([[1, 0, np.nan, 0, 1, 0.0]]))
    assert not out.any() and not ins.any(), "a coordinate that is not a number is outside"


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the CPU statements
# ---------------------------------------------------------------------------------------------------------------------
SCENE = dict(K=48, D=4, q=0.05, md=5.0, family=MM.TRANSLATION, hyps=64, thr=1.0, seed=0, r=3, sigma=1.5)
_scenes = {}


def scene(seed):
    """(frames, path, (out, correction, model, counts, held)) of jittered scene `seed`, computed once per session"""
    if seed not in _scenes:
        frames, path = SM.jitter_scene(seed)
        s = SCENE
        _scenes[seed] = (frames, path, SM.sequence(frames, s["K"], s["D"], s["q"], s["md"], s["family"], s["hyps"], s["thr"], s["seed"],
                                                   SM.weights(s["r"], s["sigma"])))
    return _scenes[seed]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_chain_of_statements_steadies_a_jittered_pan(seed):
    """T = 14 uint8 frames of 64 x 80: a pan of 1 px per frame plus integer jitter in [-2, 2].  Every step must be fitted, and
    the steadied path's mean absolute second difference must be at most 0.25 of the true path's.  (Seeds 0 .. 3 give 0.131,
    0.110, 0.106, 0.150 with the step models within 0.0072 px of the truth.)"""
    frames, path, (out, corr, model, counts, held) = scene(seed)
    assert frames.shape == (14, 64, 80) and frames.dtype == np.uint8
    assert counts[:, 2].tolist() == [1] * 13 and not held.any(), "every step is fitted"
    err = float(np.abs(model[:, [2, 5]] - np.diff(path, axis=0)).max())
    steadied = path + corr[:, [2, 5]].astype(np.float64)
    d2 = lambda p: float(np.abs(np.diff(p, 2, axis=0)).mean())   # noqa: E731
    ratio = d2(steadied) / d2(path)
    print(f"seed {seed}: step models within {err:.4f} px, second difference {d2(steadied):.3f} / {d2(path):.3f} = {ratio:.3f}")
    assert ratio <= 0.25
    assert _bits_identity(corr[[0, -1]]) and np.array_equal(out[0], frames[0]) and np.array_equal(out[-1], frames[-1])
    assert out.dtype == np.uint8 and out.shape == frames.shape


# ---------------------------------------------------------------------------------------------------------------------
# the product's interface, without a device
# ---------------------------------------------------------------------------------------------------------------------
STABILIZE_SYMBOLS = ["oflk_stabilize_trajectory", "oflk_warp_affine", "oflk_stabilize_trajectory_host", "oflk_warp_affine_host",
                     "oflk_warp_affine_host_u8", "oflk_stabilize_sequence", "oflk_stabilize_sequence_u8"]


def test_header_exports_and_signatures_carry_the_new_names():
    import _oflk
    from test_abi import ROOT, declared_functions

    L = _oflk.lib()
    declared = declared_functions()
    for name in STABILIZE_SYMBOLS:
        assert name in declared and name in _oflk.SIGNATURES and hasattr(L, name), name
    header = (ROOT / "include" / "oflk.h").read_text()
    assert "#define OFLK_STABILIZE_MAX_RADIUS 64" in header
    assert _oflk.STABILIZE_MAX_RADIUS == SM.MAX_RADIUS == 64
    for r, sigma in [(0, None), (1, None), (15, None), (64, None), (7, 0.9)]:
        assert np.array_equal(_oflk.stabilize_weights(r, sigma), SM.weights(r, sigma))


def test_refusals_come_before_any_device_call():
    """every refusal is decided on the host: this runs without a GPU, with pointers that are never dereferenced"""
    import _oflk

    L = _oflk.lib()
    INV, UNS = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED
    P = 0x10000   # an aligned address, never read
    w = np.ones(65, np.float64)

    def weights(kind):
        v = w.copy()
        if kind is not None:
            v[2] = kind
        return v.ctypes.data_as(_oflk._f64p)

    def traj(model=P, counts=None, T=5, wt=None, radius=3, corr=P, mp=P, held=None, bad=None):
        return L.oflk_stabilize_trajectory(model, counts, T, weights(bad) if wt is None else wt, radius, corr, mp, held, None)

    def traj_host(model=P, T=5, radius=3, corr=P, mp=P, bad=None, wt=None):
        c = ctypes.cast
        return L.oflk_stabilize_trajectory_host(c(model, _oflk._f32p) if model else None, None, T, weights(bad) if wt is None else wt,
                                                radius, c(corr, _oflk._f32p) if corr else None, c(mp, _oflk._f64p) if mp else None,
                                                None)

    bad = [dict(T=0), dict(T=-3), dict(radius=-1), dict(radius=65), dict(bad=0.0), dict(bad=-1.0), dict(bad=float("nan")),
           dict(bad=float("inf")), dict(model=None), dict(corr=None), dict(mp=None)]
    for kw in bad + [dict(mp=P + 4)]:
        assert traj(**kw) == INV, kw
        assert L.oflk_last_error()
    for kw in bad:
        assert traj_host(**kw) == INV, kw
    null_w = ctypes.cast(None, _oflk._f64p)
    assert traj(wt=null_w) == INV and traj_host(wt=null_w) == INV

    def warp(frames=P, u8=0, F=2, H=8, W=8, mp=P, out=P, inside=None):
        return L.oflk_warp_affine(frames, u8, F, H, W, mp, out, inside, None)

    def warp_host(u8, frames=P, F=2, H=8, W=8, mp=P, out=P):
        c = ctypes.cast
        if u8:
            return L.oflk_warp_affine_host_u8(frames, F, H, W, c(mp, _oflk._f64p) if mp else None, out, None)
        return L.oflk_warp_affine_host(c(frames, _oflk._f32p) if frames else None, F, H, W, c(mp, _oflk._f64p) if mp else None,
                                       c(out, _oflk._f32p) if out else None, None)

    bad = [dict(F=0), dict(F=-1), dict(H=1), dict(W=1), dict(H=0), dict(W=-4), dict(frames=None), dict(mp=None), dict(out=None)]
    for u8 in (0, 1):
        for kw in bad + [dict(mp=P + 4)]:
            assert warp(u8=u8, **kw) == INV, (u8, kw)
        for kw in bad:
            assert warp_host(u8, **kw) == INV, (u8, kw)
        assert warp(u8=u8, H=1 << 15, W=1 << 15) == UNS and warp_host(u8, H=1 << 15, W=1 << 15) == UNS
    assert warp(u8=0, frames=P + 2) == INV and warp(u8=0, out=P + 1) == INV

    def seq(u8, frames=P, T=6, H=64, W=80, levels=3, win=5, iters=3, alpha=0.01, beta=0.5, mr=4.0, q=0.05, md=5.0, K=20, D=4, model=1,
            hyps=64, thr=1.0, seed=0, radius=3, out=P, bad=None, wt=None):
        c = ctypes.cast
        fn = L.oflk_stabilize_sequence_u8 if u8 else L.oflk_stabilize_sequence
        fr = frames if u8 else (c(frames, _oflk._f32p) if frames else None)
        o = out if u8 else (c(out, _oflk._f32p) if out else None)
        return fn(fr, T, H, W, levels, win, iters, alpha, beta, mr, q, md, K, D, model, hyps, thr, seed,
                  weights(bad) if wt is None else wt, radius, o, None, None, None, None)

    nan = float("nan")
    own = [dict(T=1), dict(T=0), dict(H=1), dict(W=1), dict(frames=None), dict(out=None), dict(radius=-1), dict(radius=65),
           dict(bad=0.0), dict(bad=nan), dict(bad=float("inf")), dict(bad=-2.0), dict(wt=null_w)]
    motion = [dict(model=3), dict(model=-1), dict(hyps=0), dict(hyps=MM.MAX_HYPOTHESES + 1), dict(thr=0.0), dict(thr=nan),
              dict(thr=float("inf"))]
    replenish = [dict(K=0), dict(D=0), dict(q=-0.1), dict(q=1.5), dict(q=nan), dict(md=-1.0), dict(md=nan), dict(alpha=-1.0),
                 dict(beta=nan), dict(mr=-1.0), dict(mr=nan), dict(levels=0), dict(iters=0)]
    for u8 in (0, 1):
        for kw in own + motion + replenish:
            assert seq(u8, **kw) == INV, (u8, kw)
            assert L.oflk_last_error()
        for kw in [dict(win=4), dict(win=13), dict(H=6, W=6), dict(H=1 << 15, W=1 << 15)]:
            assert seq(u8, **kw) == UNS, (u8, kw)


def test_python_arguments_are_checked_before_the_library_is_asked():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    m = np.tile(np.float32([[1, 0, 1], [0, 1, 0]]), (5, 1, 1))
    for kw in [dict(radius=-1), dict(radius=65), dict(radius=2.5), dict(radius=True), dict(sigma=0), dict(sigma=-1.0),
               dict(sigma=float("nan")), dict(sigma=float("inf")), dict(radius=64, sigma=0.5), dict(status=np.ones(4)),
               dict(status=np.ones((5, 2)))]:
        with pytest.raises(ValueError):
            K.stabilize_trajectory(m, **kw)
    for bad in (np.zeros((5, 5), np.float32), np.zeros((5, 3, 2), np.float32), np.zeros(7, np.float32)):
        with pytest.raises(ValueError):
            K.stabilize_trajectory(bad)
    f = np.zeros((3, 8, 8), np.float32)
    ident = np.tile(SM.IDENTITY, (3, 1))
    for frames, maps in [(f, ident[:2]), (f, np.zeros((3, 5))), (f[:, :1], ident), (f[:, :, :1], ident), (np.zeros((2, 3, 8, 8)), ident),
                         (f[:0], ident[:0]), (f[0], ident)]:
        with pytest.raises(ValueError):
            K.warp_affine(frames, maps)
    u8 = np.zeros((4, 64, 80), np.uint8)
    for kw in [dict(model="homography"), dict(radius=65), dict(radius=-1), dict(sigma=0.0), dict(hypotheses=0), dict(threshold=0),
               dict(seed=-1), dict(detect_every=0), dict(max_corners=0), dict(quality_level=2.0), dict(min_distance=-1),
               dict(num_levels=0), dict(window_size=4), dict(num_iterations=0), dict(alpha=-1), dict(max_residual=-1)]:
        args = dict(max_corners=20, detect_every=4)
        args.update(kw)
        with pytest.raises(ValueError):
            P.lucas_kanade_pyramidal_sequence_stabilize(u8, **args)
    with pytest.raises(ValueError):
        P.lucas_kanade_pyramidal_sequence_stabilize(u8[:1], 20, 4)
    assert P.stabilize_trajectory is K.stabilize_trajectory and P.warp_affine is K.warp_affine and P.Trajectory is K.Trajectory
