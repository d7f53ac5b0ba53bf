"""CPU tests of online video stabilisation: the ring and the schedule (tests/stabilize_online_model.py) against the offline
statement (tests/stabilize_model.py), and what the product declares and refuses before any device call.  No GPU."""
import ctypes

import numpy as np
import pytest

import motion_model as MM
import stabilize_model as SM
import stabilize_online_model as OM

FAMILIES = [MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE]


def spoiled(T, family, seed):
    """T-1 step models and counts with a held step (status 0) and a NaN coefficient planted where there is room"""
    model = SM.noisy_models(T - 1, family, seed)
    counts = np.tile(np.int32([30, 40, 1]), (T - 1, 1))
    if T > 2:
        counts[(T - 1) // 2, 2] = 0
    if T > 3:
        model[(T - 1) // 3, 2] = np.nan
    return model, counts


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_pushes_and_a_flush_equal_the_offline_trajectory(family):
    """a ring of 2r steps, emission at lag r and a flush with the true T give trajectory()'s corrections and maps bit for bit"""
    for T in (1, 2, 3, 4, 7, 8, 9, 20):
        for r in (0, 1, 3, 4, 8, 12):
            model, counts = spoiled(T, family, 100 * T + r)
            w = SM.weights(r)
            want = SM.trajectory(model, counts, T, w)
            if T > 3:
                assert want[2].sum() == len({(T - 1) // 2, (T - 1) // 3}), "a held step and a NaN step"
            for cap in (None, 2 * r + 3):
                idx, corr, mp = OM.run(model, counts, T, w, cap)
                assert idx == list(range(T)), (T, r, idx)
                SM.same(corr, want[0], f"T={T} r={r} cap={cap}: correction")
                SM.same(mp, want[1], f"T={T} r={r} cap={cap}: map")


def test_the_schedule_emits_frame_t_minus_r_and_flushes_the_rest():
    w = SM.weights(3)
    model, counts = spoiled(8, MM.SIMILARITY, 1)
    st = OM.Stream(w)
    out = [st.push(None if t == 0 else model[t - 1], None if t == 0 else counts[t - 1]) for t in range(8)]
    assert [None if e is None else e[0] for e in out] == [None, None, None, 0, 1, 2, 3, 4]
    assert [e[0] for e in st.flush()] == [5, 6, 7] and st.flush() == []
    assert OM.Stream(w).flush() == [], "nothing before any push"
    st = OM.Stream(w)
    st.push()
    st.push(model[0], counts[0])
    assert [e[0] for e in st.flush()] == [0, 1], "T <= r: everything at the flush"
    st = OM.Stream(SM.weights(0))
    assert [st.push(model[0], counts[0])[0] for _ in range(3)] == [0, 1, 2] and st.flush() == []


def test_the_ring_form_reads_only_its_window():
    """trajectory_ring on a ring filled up to the newest step of the window: slots outside it hold other steps or garbage"""
    r, T = 3, 40
    w = SM.weights(r)
    model, counts = spoiled(T, MM.AFFINE, 5)
    want = SM.trajectory(model, counts, T, w)
    for cap in (6, 7, 11):
        for f in (0, 2, 3, 17, 30):
            ring = OM.fill_ring(model, counts, cap, f + r)     # frame f + r has been pushed: steps 0 .. f + r - 1
            c, m = OM.trajectory_ring(*ring, cap, f, 1, -1, w)
            SM.same(c[0], want[0][f], f"cap {cap} frame {f}")
            SM.same(m[0], want[1][f], f"cap {cap} frame {f}: map")
        ring = OM.fill_ring(model, counts, cap, T - 1)
        c, m = OM.trajectory_ring(*ring, cap, T - r, r, T, w)
        SM.same(c, want[0][T - r:], f"cap {cap}: the flush")
        SM.same(m, want[1][T - r:], f"cap {cap}: the flush, map")
    # a NULL counts ring: the status decides nothing
    ring = OM.fill_ring(model, counts, 6, 20)
    SM.same(OM.trajectory_ring(ring[0], None, 6, 17, 1, -1, w)[0][0], SM.trajectory(model, None, T, w)[0][17], "no counts")


# ---------------------------------------------------------------------------------------------------------------------
# the product's interface, without a device
# ---------------------------------------------------------------------------------------------------------------------
ONLINE_SYMBOLS = ["oflk_stabilize_trajectory_ring", "oflk_stabilizer_create", "oflk_stabilizer_destroy", "oflk_stabilizer_reset",
                  "oflk_stabilizer_workspace_bytes", "oflk_stabilizer_lag", "oflk_stabilizer_frame_index", "oflk_stabilizer_push_device",
                  "oflk_stabilizer_push", "oflk_stabilizer_flush_device", "oflk_stabilizer_flush", "oflk_stabilizer_correction_device",
                  "oflk_stabilizer_tracker"]


def test_header_exports_and_signatures_carry_the_new_names():
    import _oflk
    from test_abi import ROOT, declared_functions

    L = _oflk.lib()
    declared = declared_functions()
    for name in ONLINE_SYMBOLS:
        assert name in declared and name in _oflk.SIGNATURES and hasattr(L, name), name
    header = (ROOT / "include" / "oflk.h").read_text()
    assert "typedef struct oflk_stabilizer oflk_stabilizer;" in header
    import lucas_kanade_pyramidal as P

    assert hasattr(P, "OnlineStabilizer") and P.StabilizedFrame._fields == ("index", "frame", "correction", "inside")


def _create(L, _oflk, w, device=0, H=64, W=80, u8=1, levels=3, win=5, iters=3, alpha=0.01, beta=0.5, mr=4.0, q=0.05, md=5.0, K=20, D=4,
            model=1, hyps=64, thr=1.0, seed=0, radius=3, wt=None, bad=None):
    v = w.copy()
    if bad is not None:
        v[2] = bad
    h = ctypes.c_void_p()
    rc = L.oflk_stabilizer_create(ctypes.byref(h), device, H, W, u8, levels, win, iters, alpha, beta, mr, q, md, K, D, model, hyps, thr,
                                  seed, v.ctypes.data_as(_oflk._f64p) if wt is None else wt, radius)
    return rc, h


def test_creation_refusals_come_before_any_device_call():
    """every refusal is decided on the host: this runs without a GPU"""
    import _oflk

    L = _oflk.lib()
    INV, UNS = _oflk.OFLK_ERR_INVALID, _oflk.OFLK_ERR_UNSUPPORTED
    w = np.ones(65, np.float64)
    nan = float("nan")
    null_w = ctypes.cast(None, _oflk._f64p)
    own = [dict(H=1), dict(W=1), dict(H=0), dict(radius=-1), dict(radius=65), dict(bad=0.0), dict(bad=nan), dict(bad=float("inf")),
           dict(bad=-2.0), dict(wt=null_w)]
    motion = [dict(model=3), dict(model=-1), dict(model=-2), dict(hyps=0), dict(hyps=MM.MAX_HYPOTHESES + 1), dict(thr=0.0), dict(thr=nan),
              dict(thr=float("inf"))]
    tracker = [dict(K=0), dict(D=-1), dict(q=-0.1), dict(q=1.5), dict(q=nan), dict(md=-1.0), dict(md=nan), dict(alpha=-1.0),
               dict(beta=nan), dict(mr=-1.0), dict(mr=nan), dict(levels=0), dict(iters=0), dict(device=-1)]
    for u8 in (0, 1):
        for kw in own + motion + tracker:
            rc, h = _create(L, _oflk, w, u8=u8, **kw)
            assert rc == INV and not h.value, (u8, kw)
            assert L.oflk_last_error()
        for kw in [dict(win=4), dict(win=13), dict(H=6, W=6), dict(H=1 << 15, W=1 << 15)]:
            rc, h = _create(L, _oflk, w, u8=u8, **kw)
            assert rc == UNS and not h.value, (u8, kw)
    assert L.oflk_stabilizer_create(None, 0, 64, 80, 1, 3, 5, 3, 0.01, 0.5, 4.0, 0.05, 5.0, 20, 4, 1, 64, 1.0, 0,
                                    w.ctypes.data_as(_oflk._f64p), 3) == INV


def test_a_stabiliser_answers_without_a_device_until_a_frame_is_pushed():
    """creation, the getters, a flush with nothing to emit, reset and destruction make no device call"""
    import _oflk

    L = _oflk.lib()
    INV = _oflk.OFLK_ERR_INVALID
    P = 0x10000   # an aligned address, never read
    for radius, D in [(3, 4), (0, 0), (64, 1)]:
        rc, h = _create(L, _oflk, np.ones(65, np.float64), radius=radius, D=D)
        assert rc == 0 and h.value
        assert L.oflk_stabilizer_lag(h) == radius and L.oflk_stabilizer_frame_index(h) == -1
        assert L.oflk_stabilizer_workspace_bytes(h) == 0
        tr = L.oflk_stabilizer_tracker(h)
        assert tr and L.oflk_tracker_frame_index(tr) == -1
        c, m = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.oflk_stabilizer_correction_device(h, ctypes.byref(c), ctypes.byref(m)) == INV, "nothing has been emitted"
        e, first, count = ctypes.c_int(5), ctypes.c_int(5), ctypes.c_int(5)
        for args in [(None, P, P, None, ctypes.byref(e), None), (h, None, P, None, ctypes.byref(e), None),
                     (h, P, None, None, ctypes.byref(e), None), (h, P, P, None, None, None)]:
            assert L.oflk_stabilizer_push_device(*args) == INV
        assert e.value == -1
        assert L.oflk_stabilizer_flush_device(h, P, None, None, ctypes.byref(count), None) == INV
        assert L.oflk_stabilizer_flush_device(h, None, None, ctypes.byref(first), ctypes.byref(count), None) == 0
        assert (first.value, count.value) == (0, 0), "nothing before any push"
        assert L.oflk_stabilizer_push_device(h, P, P, None, ctypes.byref(e), None) == INV and b"flushed" in L.oflk_last_error()
        assert L.oflk_stabilizer_push(h, P, P, None, None, ctypes.byref(e)) == INV and e.value == -1
        assert L.oflk_stabilizer_flush(h, None, None, None, ctypes.byref(first), ctypes.byref(count)) == 0 and count.value == 0
        assert L.oflk_stabilizer_reset(h, None) == 0 and L.oflk_stabilizer_frame_index(h) == -1
        assert L.oflk_stabilizer_workspace_bytes(h) == 0
        assert L.oflk_stabilizer_destroy(h) == 0
    assert L.oflk_stabilizer_destroy(None) == 0 and L.oflk_stabilizer_reset(None, None) == INV
    assert L.oflk_stabilizer_lag(None) == -1 and L.oflk_stabilizer_frame_index(None) == -1 and L.oflk_stabilizer_workspace_bytes(None) == 0
    assert not L.oflk_stabilizer_tracker(None)
    if _oflk.device_count() == 0:   # the first push is the first device call
        rc, h = _create(L, _oflk, np.ones(65, np.float64))
        e = ctypes.c_int(5)
        assert L.oflk_stabilizer_push_device(h, P, P, None, ctypes.byref(e), None) == _oflk.OFLK_ERR_NO_DEVICE and e.value == -1
        assert L.oflk_stabilizer_frame_index(h) == -1
        L.oflk_stabilizer_destroy(h)


def test_ring_trajectory_refusals_come_before_any_device_call():
    import _oflk

    L = _oflk.lib()
    INV = _oflk.OFLK_ERR_INVALID
    P = 0x10000
    w = np.ones(65, np.float64)

    def ring(model=P, counts=None, cap=6, f0=10, n=1, T=-1, radius=3, corr=P, mp=P, bad=None, wt=None):
        v = w.copy()
        if bad is not None:
            v[2] = bad
        return L.oflk_stabilize_trajectory_ring(model, counts, cap, f0, n, T, v.ctypes.data_as(_oflk._f64p) if wt is None else wt, radius,
                                                corr, mp, None)

    bad = [dict(radius=-1), dict(radius=65), dict(bad=0.0), dict(bad=-1.0), dict(bad=float("nan")), dict(bad=float("inf")),
           dict(wt=ctypes.cast(None, _oflk._f64p)), dict(model=None), dict(corr=None), dict(mp=None), dict(mp=P + 4),
           dict(cap=5), dict(cap=0), dict(cap=-6), dict(radius=0, cap=0), dict(radius=64, cap=127),
           dict(n=0), dict(n=-1), dict(n=2), dict(n=129, T=1000), dict(f0=-1), dict(T=-2),
           dict(T=10), dict(f0=8, n=3, T=10), dict(T=0), dict(f0=0, n=1, T=0)]
    for kw in bad:
        assert ring(**kw) == INV, kw
        assert L.oflk_last_error()


def test_python_arguments_are_checked_before_the_library_is_asked():
    import lucas_kanade_pyramidal as P

    good = dict(shape=(64, 80), max_corners=20)
    for kw in [dict(shape=(64,)), dict(shape=(1, 80)), dict(shape=(64, 1)), dict(shape=(64, 80, 3)), dict(dtype=np.float64),
               dict(model="homography"), dict(model=None), dict(radius=65), dict(radius=-1), dict(radius=2.5), dict(radius=True),
               dict(sigma=0.0), dict(sigma=float("nan")), dict(radius=64, sigma=0.5), dict(hypotheses=0), dict(threshold=0), dict(seed=-1),
               dict(detect_every=-1), dict(detect_every=1.5), dict(detect_every=True), dict(max_corners=0), dict(quality_level=2.0),
               dict(min_distance=-1), dict(num_levels=0), dict(window_size=4), dict(num_iterations=0), dict(alpha=-1),
               dict(max_residual=-1)]:
        args = dict(good, **kw)
        with pytest.raises(ValueError):
            P.OnlineStabilizer(**args)
    with P.OnlineStabilizer((64, 80), 20, radius=3, model="translation", dtype=np.float32) as s:   # no device call yet
        assert s.lag == 3 and s.radius == 3 and s.frame_index == -1 and s.shape == (64, 80) and s.flush() == []
        with pytest.raises(ValueError):
            s.push(np.zeros((64, 81), np.float32))
        with pytest.raises(ValueError):
            s.push(np.zeros((64, 80), np.float32))   # flushed: refused by the library before any device call
        s.reset()
        assert s.frame_index == -1
