"""CPU tests of the global motion fit: the statement (tests/motion_model.py) against planted scenes, np.linalg.lstsq and its
edge cases, and what the product refuses before any device call.  No GPU."""
import ctypes

import numpy as np
import pytest

import motion_model as MM

FAMILY = {MM.TRANSLATION: "translation", MM.SIMILARITY: "similarity", MM.AFFINE: "affine"}

# The returned coefficients against float64 np.linalg.lstsq on the returned inlier set, worst absolute difference over the
# planted scenes (PLANTED x {similarity, affine} x seeds 0, 1, 2): 1.183e-07, which is the float32 rounding of the result
# (half an ulp of the translation 3.5 is 1.19e-07).  The gate is four times that; the margin covers other seeds.
LSTSQ_WORST = 1.183e-07
LSTSQ_GATE = 4 * LSTSQ_WORST


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3])
def test_samples_are_distinct_and_in_range(m):
    for M in range(m, 71):
        pos = MM.sample(seed=7, index=3, hyps=200, m=m, M=M)
        assert pos.min() >= 0 and pos.max() < M
        s = np.sort(pos, 1)
        assert (s[:, 1:] != s[:, :-1]).all(), f"m={m} M={M}: a position was drawn twice"
    if m > 1:   # every position is reachable as a later pick
        assert set(MM.sample(1, 0, 400, m, m)[:, -1].tolist()) == set(range(m))


def test_the_draws_of_a_step_depend_on_seed_index_and_hypothesis_only():
    a = MM.sample(11, 5, 64, 3, 50)
    assert np.array_equal(MM.sample(11, 5, 128, 3, 50)[:64], a), "the number of hypotheses is not an input"
    assert not np.array_equal(MM.sample(11, 6, 64, 3, 50), a) and not np.array_equal(MM.sample(12, 5, 64, 3, 50), a)
    assert len({tuple(r) for r in a.tolist()}) > 50, "hypotheses draw different samples"
    # a step of a batch is the step alone with its index: no state is carried
    scenes = [MM.planted_scene(65, 0.4, s) for s in (1, 2, 3)]
    src, dst = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    batch = MM.estimate_batch(src, dst, None, MM.AFFINE, 64, 1.0, seed=9, step0=40)
    for s in range(3):
        MM.same(tuple(x[s] for x in batch), MM.estimate(src[s], dst[s], None, MM.AFFINE, 64, 1.0, 9, 40 + s), f"step {s}")


def test_the_hash_is_the_stated_one():
    """four rounds of murmur3's finaliser, written out on Python integers"""
    def fmix(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    for seed, index, h, j in [(0, 0, 0, 0), (1, 2, 3, 1), (0xFFFFFFFF, 0xFFFFFFFE, 65535, 2), (123456789, 2 ** 31 + 5, 256, 0)]:
        x = fmix(seed ^ 0x9E3779B9)
        for v in (index, h, j):
            x = fmix((x + v) & 0xFFFFFFFF)
        assert int(MM.draw(seed, index, np.uint64(h), j)) == x


# ---------------------------------------------------------------------------------------------------------------------
# planted scenes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("model", [MM.SIMILARITY, MM.AFFINE], ids=["similarity", "affine"])
@pytest.mark.parametrize("N,share,hyps", MM.PLANTED)
def test_planted_scenes_recover_the_planted_set_and_the_lstsq_coefficients(N, share, hyps, model, seed):
    src, dst, planted = MM.planted_scene(N, share, 100 + seed)
    c, mask, counts = MM.estimate(src, dst, None, model, hyps, 1.0, seed)
    assert np.array_equal(mask.astype(bool), planted), "the returned mask is the planted inlier set"
    assert counts.tolist() == [int(planted.sum()), N, 1]
    diff = float(np.abs(c.astype(np.float64) - MM.lstsq_fit(model, src, dst, planted)).max())
    print(f"N={N} {FAMILY[model]} seed {seed}: max |c - lstsq| = {diff:.3e}; against the planted coefficients "
          f"{np.abs(c - MM.planted_coefficients()).max():.3e}")
    assert diff <= LSTSQ_GATE
    assert np.abs(c - MM.planted_coefficients()).max() < 1e-4, "float32 input rounding only"


def test_translation_recovers_a_planted_shift():
    rng = np.random.default_rng(3)
    src = (rng.random((120, 2)) * [1919, 1079]).astype(np.float32)
    dst = src + np.float32([3.5, -2.25])
    out = rng.permutation(120)[:50]
    dst[out] += rng.uniform(5, 65, (50, 2)).astype(np.float32)
    planted = np.ones(120, bool)
    planted[out] = False
    c, mask, counts = MM.estimate(src, dst, None, MM.TRANSLATION, 32, 1.0, 4)
    assert np.array_equal(mask.astype(bool), planted) and counts.tolist() == [70, 120, 1]
    assert np.abs(c.astype(np.float64) - MM.lstsq_fit(MM.TRANSLATION, src, dst, planted)).max() <= LSTSQ_GATE


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def _edge(name):
    hit = [e for e in MM.edge_cases() if e[0].startswith(name)]
    assert hit, name
    return hit


def _run(e, seed=0, index=0, detail=None):
    _, src, dst, valid, model, hyps, thr = e
    return MM.estimate(src, dst, valid, model, hyps, thr, seed, index, detail)


def test_fewer_valid_correspondences_than_the_sample():
    for e in _edge("M="):
        c, mask, counts = _run(e)
        M = int(e[3].sum())
        assert np.isnan(c).all() and not mask.any() and counts.tolist() == [0, M, 0], e[0]


def test_every_hypothesis_degenerate():
    for name in ("identical points, similarity", "identical points, affine", "collinear points, affine"):
        (e,) = _edge(name)
        d = {}
        c, mask, counts = _run(e, detail=d)
        assert (d["score"] == -1).all(), name
        assert np.isnan(c).all() and not mask.any() and counts.tolist() == [0, len(e[1]), 0], name
    (e,) = _edge("collinear points, similarity")   # a line is enough for a similarity
    c, mask, counts = _run(e)
    assert counts.tolist() == [10, 10, 1] and np.array_equal(c, np.float32([1, 0, 3, 0, 1, 4]))


def test_an_exact_model_ties_every_score_and_hypothesis_zero_wins():
    for e in _edge("exact model"):
        d = {}
        c, mask, counts = _run(e, detail=d)
        N = len(e[1])
        assert (d["score"] == N).all() and d["best"] == 0, e[0]
        assert mask.all() and counts.tolist() == [N, N, 1]
        ref = MM.lstsq_fit(e[4], e[1], e[2], np.ones(N, bool))
        assert np.abs(c.astype(np.float64) - ref).max() <= LSTSQ_GATE, e[0]


def test_a_residual_exactly_on_the_threshold_is_an_inlier():
    for e in _edge("residual on the threshold"):
        d = {}
        c, mask, counts = _run(e, detail=d)
        N = len(e[1])
        best = d["best_model"]
        assert np.array_equal(best, np.float32([1, 0, 2, 0, 1, 1])), "the best hypothesis is the planted translation"
        r2 = MM.residual2(best, e[1][:, 0], e[1][:, 1], e[2][:, 0], e[2][:, 1])
        assert r2[7] == np.float32(25) and d["score"][d["best"]] == N, "(3, 4) is at distance 5 exactly: an inlier"
        assert counts[1] == N and counts[2] == 1


def test_nan_and_inf_coordinates_are_invalid_without_a_mask():
    for e in _edge("NaN and inf"):
        c, mask, counts = _run(e)
        bad = [3, 11, 4, 20, 21]
        N = len(e[1])
        assert counts.tolist() == [N - 5, N - 5, 1] and not mask[bad].any() and mask.sum() == N - 5, e[0]
        assert np.isfinite(c).all()
        keep = np.ones(N, bool)
        keep[bad] = False
        MM.same(_run(e), MM.estimate(e[1], e[2], keep, e[4], e[5], e[6]), "finiteness decides exactly as a mask would")


def test_a_refilled_slot_is_two_tracks():
    """slot 1 dies on the step into row 2 and is refilled there: excluded on step 1, included on step 2"""
    vis = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 1, 0]], bool)
    born = np.zeros_like(vis)
    born[0] = True
    born[2, 1] = True
    v = MM.tracks_valid(vis, born)
    assert v.tolist() == [[True, True, True], [True, False, False], [True, True, False]]
    assert MM.tracks_valid(vis).tolist() == [[True, True, True], [True, True, False], [True, True, False]]
    # ... and the fit sees it: the refilled slot jumps, which would be an outlier of step 1 if it were taken
    rng = np.random.default_rng(1)
    K, T = 30, 4
    p0 = (rng.random((K, 2)) * 100).astype(np.float32)
    rows = np.stack([p0 + np.float32(2 * t) for t in range(T)])
    vis, born = np.ones((T, K), bool), np.zeros((T, K), bool)
    born[0] = True
    born[2, 5] = True
    rows[2:, 5] += np.float32(40)
    c, mask, counts = MM.tracks(rows, vis, born, MM.TRANSLATION, 16, 0.5, 3)
    assert counts.tolist() == [[K, K, 1], [K - 1, K - 1, 1], [K, K, 1]]
    assert not mask[1, 5] and mask[2, 5]
    c2, mask2, counts2 = MM.tracks(rows, vis, None, MM.TRANSLATION, 16, 0.5, 3)
    assert counts2[1].tolist() == [K - 1, K, 1] and not mask2[1, 5], "without born the jump is an outlier of step 1"


# ---------------------------------------------------------------------------------------------------------------------
# the product's interface, without a device
# ---------------------------------------------------------------------------------------------------------------------
MOTION_SYMBOLS = ["oflk_motion_workspace", "oflk_estimate_motion", "oflk_tracks_motion", "oflk_estimate_motion_host",
                  "oflk_tracker_set_motion", "oflk_tracker_motion_device", "oflk_tracker_read_motion"]


def test_the_library_exports_the_motion_entry_points():
    import _oflk

    L = _oflk.lib()
    for name in MOTION_SYMBOLS:
        assert name in _oflk.SIGNATURES and hasattr(L, name), name
    assert _oflk.MOTION_MODELS == MM.FAMILIES and _oflk.MOTION_MAX_HYPOTHESES == MM.MAX_HYPOTHESES


def test_the_workspace_size_covers_its_pieces():
    import _oflk

    for S, N, Hn in [(1, 1, 1), (3, 65, 257), (1, 10000, 1024), (7, 1000, 64)]:
        need = S * 4 + S * N * 16 + S * Hn * 4 + S * Hn * 24
        got = _oflk.motion_workspace(S, N, Hn)
        assert need <= got <= need + 4 * 256 and got % 256 == 0


def test_refusals_come_before_any_device_call():
    """every refusal is OFLK_ERR_INVALID and is decided on the host: this runs without a GPU, with pointers that are never
    dereferenced"""
    import _oflk

    L = _oflk.lib()
    P, WS = 0x10000, 0x20000   # 8-byte and 256-byte aligned addresses, never read
    n = ctypes.c_size_t(0)
    big = 1 << 40

    def est(src=P, dst=P, valid=None, S=2, N=10, step0=0, model=1, hyps=16, thr=1.0, seed=0, ws=WS, ws_bytes=big, out=P, inl=P, cnt=P):
        return L.oflk_estimate_motion(src, dst, valid, S, N, step0, model, hyps, thr, seed, ws, ws_bytes, out, inl, cnt, None)

    def trk(tracks=P, vis=P, born=None, T=3, K=10, t0=0, model=1, hyps=16, thr=1.0, seed=0, ws=WS, ws_bytes=big, out=P, inl=P, cnt=P):
        return L.oflk_tracks_motion(tracks, vis, born, T, K, t0, model, hyps, thr, seed, ws, ws_bytes, out, inl, cnt, None)

    need = _oflk.motion_workspace(2, 10, 16)
    bad = [dict(model=3), dict(model=-1), dict(hyps=0), dict(hyps=MM.MAX_HYPOTHESES + 1), dict(thr=0.0), dict(thr=-1.0),
           dict(thr=float("nan")), dict(thr=float("inf")), dict(ws=None), dict(ws=WS + 8), dict(ws_bytes=need - 1),
           dict(out=None), dict(inl=None), dict(cnt=None)]
    for kw in bad + [dict(S=0), dict(N=0), dict(src=None), dict(dst=None), dict(src=P + 4), dict(dst=P + 4)]:
        assert est(**kw) == _oflk.OFLK_ERR_INVALID, kw
        assert L.oflk_last_error()
    for kw in bad + [dict(T=1), dict(K=0), dict(tracks=None), dict(vis=None), dict(tracks=P + 4)]:
        assert trk(**kw) == _oflk.OFLK_ERR_INVALID, kw
    f = np.zeros((2, 10, 2), np.float32)
    out, inl, cnt = np.zeros((2, 6), np.float32), np.zeros((2, 10), np.uint8), np.zeros((2, 3), np.int32)

    def host(src=f, S=2, N=10, model=1, hyps=16, thr=1.0, out=out):
        return L.oflk_estimate_motion_host(None if src is None else _oflk.ptr(src), _oflk.ptr(f), None, S, N, 0, model, hyps, thr, 0,
                                           None if out is None else _oflk.ptr(out), inl.ctypes.data, cnt.ctypes.data_as(_oflk._i32p))

    for kw in [dict(src=None), dict(S=0), dict(N=-1), dict(model=7), dict(hyps=0), dict(thr=0.0), dict(out=None)]:
        assert host(**kw) == _oflk.OFLK_ERR_INVALID, kw
    for args in [(0, 10, 16), (2, 0, 16), (2, 10, 0), (2, 10, MM.MAX_HYPOTHESES + 1)]:
        assert L.oflk_motion_workspace(*args, ctypes.byref(n)) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_motion_workspace(2, 10, 16, None) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_tracker_set_motion(None, 1, 16, 1.0, 0) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_tracker_read_motion(None, None, None, None, None) == _oflk.OFLK_ERR_INVALID
    assert L.oflk_tracker_motion_device(None, None, None, None) == _oflk.OFLK_ERR_INVALID


def test_a_tracker_takes_and_refuses_motion_settings_without_a_device():
    import _oflk

    tr = _oflk.Tracker(0, 48, 64, True, 50, 2)   # creation makes no device call
    try:
        tr.set_motion(1, 64, 1.0, 5)
        tr.set_motion(-1)
        for args in [(3, 64, 1.0, 0), (-2, 64, 1.0, 0), (1, 0, 1.0, 0), (1, MM.MAX_HYPOTHESES + 1, 1.0, 0), (1, 64, 0.0, 0),
                     (1, 64, float("nan"), 0)]:
            with pytest.raises(ValueError):
                tr.set_motion(*args)
        with pytest.raises(ValueError, match="pushed"):
            tr.read_motion()
        assert tr.workspace_bytes == 0
    finally:
        tr.close()


def test_python_arguments_are_checked_before_the_library_is_asked():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    p = np.zeros((5, 2), np.float32)
    for kw in [dict(model="homography"), dict(model=None), dict(hypotheses=0), dict(hypotheses=2.5), dict(hypotheses=True),
               dict(threshold=0), dict(threshold=float("nan")), dict(seed=-1), dict(seed=2 ** 32), dict(step0=-1)]:
        with pytest.raises(ValueError):
            K.estimate_motion(p, p, **kw)
    for a, b, v in [(p, p[:4], None), (p[:, :1], p[:, :1], None), (p, p, np.ones(4)), (p[:0], p[:0], None), (p[None, None], p[None, None], None)]:
        with pytest.raises(ValueError):
            K.estimate_motion(a, b, v)
    with pytest.raises(ValueError):
        K.tracks_motion(p[None], np.ones((1, 5)))   # T < 2
    with pytest.raises(ValueError):
        K.tracks_motion(np.zeros((3, 5, 2)), np.ones((3, 4)))
    with pytest.raises(ValueError):
        K.tracks_motion(np.zeros((3, 5, 2)), np.ones((3, 5)), np.ones((2, 5)))
    assert P.estimate_motion is K.estimate_motion and P.tracks_motion is K.tracks_motion and P.Motion is K.Motion
    with pytest.raises(ValueError):
        P.SparseKltTracker((48, 64), 20, motion="projective")
    with P.SparseKltTracker((48, 64), 20, motion=dict(model="affine", hypotheses=32)) as tr:
        tr.set_motion(None)
        with pytest.raises(ValueError):
            tr.set_motion("affine", threshold=-1)
