"""GPU tests of online video stabilisation (run on an MI355X: python -m pytest tests/test_gpu_stabilize_online.py -m gpu -q).

oflk_stabilize_trajectory_ring must equal its statement (tests/stabilize_online_model.py), and the frames and corrections of
T pushes and a flush of an oflk_stabilizer must equal `out` and `correction` of oflk_stabilize_sequence on the same frames,
run on the GPU in the same test, byte for byte; a NaN equals a NaN.  No tolerance anywhere.
"""
import numpy as np
import pytest

import motion_model as MM
import stabilize_model as SM
import stabilize_online_model as OM
from test_gpu_stabilize import _sequence, _spoil, _warp_device
from test_gpu_tracker import _from_device
from test_stabilize_cpu import SCENE, scene

pytestmark = pytest.mark.gpu

FAMILIES = [MM.TRANSLATION, MM.SIMILARITY, MM.AFFINE]


# ---------------------------------------------------------------------------------------------------------------------
# the ring kernel
# ---------------------------------------------------------------------------------------------------------------------
def _ring_device(ring_model, ring_counts, cap, f0, n, T, w, stream=0):
    """oflk_stabilize_trajectory_ring, the outputs preset with bytes that it must overwrite and a guard row behind them"""
    import torch

    import _oflk

    d = "cuda:0"
    t_model = torch.from_numpy(np.ascontiguousarray(ring_model, np.float32)).to(d)
    t_counts = None if ring_counts is None else torch.from_numpy(np.ascontiguousarray(ring_counts, np.int32)).to(d)
    corr = torch.full((n + 1, 6), -7.0, device=d)
    mp = torch.full((n + 1, 6), -7.0, dtype=torch.float64, device=d)
    _oflk.stabilize_trajectory_ring(t_model.data_ptr(), 0 if t_counts is None else t_counts.data_ptr(), cap, f0, n, T, w,
                                    corr.data_ptr(), mp.data_ptr(), stream)
    torch.cuda.synchronize()
    corr, mp = corr.cpu().numpy(), mp.cpu().numpy()
    assert (corr[n] == -7.0).all() and (mp[n] == -7.0).all(), "nothing is written behind the n rows"
    return corr[:n], mp[:n]


def _check_ring(ring, cap, f0, n, T, w, what):
    want = OM.trajectory_ring(*ring, cap, f0, n, T, w)
    got = _ring_device(*ring, cap, f0, n, T, w)
    SM.same(got[0], want[0], f"{what}: correction")
    SM.same(got[1], want[1], f"{what}: map")
    return want


@pytest.mark.parametrize("r", [0, 1, 3, 64])
def test_the_ring_kernel_equals_the_model(r):
    """spoiled step models (status 0, NaN, a zero determinant) in a ring of the least and of a larger capacity; frames whose
    window is clipped at the stream's start, whose window wraps the ring, and the frames of a flush for several T"""
    w = SM.weights(r)
    S = 4 * r + 11
    moved = wrapped = False
    for fam in FAMILIES:
        model = SM.noisy_models(S, fam, 10 * r + fam)
        counts = np.tile(np.int32([30, 40, 1]), (S, 1))
        model, counts = _spoil(model, counts, r + fam)
        for cap in (max(2 * r, 1), 2 * r + 5):
            # the open stream: frame f once frame f + r has been pushed (steps 0 .. f + r - 1 written, the rest garbage)
            for f in sorted({0, 1, r // 2, r, r + 1, 2 * r + 1, 3 * r + 2, S - r}):
                ring = OM.fill_ring(model, counts, cap, f + r)
                rf = min(r, f)
                want = _check_ring(ring, cap, f, 1, -1, w, f"r={r} family {fam} cap {cap} open frame {f}")
                wrapped = wrapped or (f - rf) % cap + 2 * rf > cap
                moved = moved or bool((want[0] != SM.IDENTITY.astype(np.float32)).any())
            # the flush: the last min(r, T) frames of a stream of T
            for T in sorted({1, 2, r, r + 1, 2 * r + 3} - {0}):
                n = min(r, T)
                if n:
                    ring = OM.fill_ring(model, counts, cap, T - 1)
                    _check_ring(ring, cap, T - n, n, T, w, f"r={r} family {fam} cap {cap} flush of T={T}")
        ring = OM.fill_ring(model, None, max(2 * r, 1), r + 4)
        _check_ring((ring[0], None), max(2 * r, 1), 4, 1, -1, w, f"r={r} family {fam}, NULL counts")
    assert moved == (r > 0) and wrapped == (r > 0), "frames are moved, and some windows wrap the ring"
    # the whole schedule against the offline trajectory, through the device
    T = 2 * r + 6
    model, counts = model[:T - 1], counts[:T - 1]
    offline = SM.trajectory(model, counts, T, w)
    cap = max(2 * r, 1)
    for t in range(r, T):
        got = _ring_device(*OM.fill_ring(model, counts, cap, t), cap, t - r, 1, -1, w)
        SM.same(got[0][0], offline[0][t - r], f"r={r}: frame {t - r} at the push of {t}")
        SM.same(got[1][0], offline[1][t - r], f"r={r}: frame {t - r} at the push of {t}, map")
    if r:
        got = _ring_device(*OM.fill_ring(model, counts, cap, T - 1), cap, T - r, r, T, w)
        SM.same(got[0], offline[0][T - r:], f"r={r}: the flush")
        SM.same(got[1], offline[1][T - r:], f"r={r}: the flush, map")


def test_a_constant_pan_is_the_identity_from_the_ring_too():
    r, cap = 3, 6
    model = np.tile(np.float32([1, 0, 3, 0, 1, -2]), (20, 1))
    ident = np.tile(SM.IDENTITY, (1, 1))
    for f in (0, 2, 9, 14):
        corr, mp = _ring_device(*OM.fill_ring(model, None, cap, f + r), cap, f, 1, -1, SM.weights(r))
        SM.same(corr, ident.astype(np.float32), f"frame {f}: correction, bit for bit")
        assert np.array_equal(mp, ident)
    corr, mp = _ring_device(*OM.fill_ring(model, None, cap, 20), cap, 18, 3, 21, SM.weights(r))
    SM.same(corr, np.tile(SM.IDENTITY, (3, 1)).astype(np.float32), "the flush")


# ---------------------------------------------------------------------------------------------------------------------
# the stabiliser
# ---------------------------------------------------------------------------------------------------------------------
def _stabilizer(frames, K, D, q, md, family, hyps, thr, seed, w, levels=3, win=5, iters=3):
    import _oflk

    return _oflk.Stabilizer(0, frames.shape[1], frames.shape[2], frames.dtype == np.uint8, K, D, family, w, hyps, thr, seed, levels, win,
                            iters, quality_level=q, min_distance=md)


def _stream_host(st, frames, inside=False):
    """push every frame and flush: (indices in emission order, out, correction (n, 6), inside or None)"""
    idx, out, corr, ins = [], [], [], []
    for t, f in enumerate(frames):
        e, o, c, i = st.push(np.ascontiguousarray(f), inside)
        assert e == (t - st.radius if t >= st.radius else -1) and st.frame_index == t
        if e >= 0:
            idx.append(e), out.append(o), corr.append(c), ins.append(i)
    first, o, c, i = st.flush(inside)
    assert len(o) == min(st.radius, len(frames)) and first == len(frames) - len(o)
    idx += list(range(first, first + len(o)))
    out += list(o)
    corr += list(c)
    ins += [None] * len(o) if i is None else list(i)
    return idx, np.stack(out), np.stack(corr), np.stack(ins) if inside else None


def _scene_args(r=None):
    s = SCENE
    w = SM.weights(s["r"], s["sigma"]) if r is None else SM.weights(r)
    return (s["K"], s["D"], s["q"], s["md"], s["family"], s["hyps"], s["thr"], s["seed"], w)


def _against_the_sequence_call(frames, args, what, **kw):
    """the stabiliser's frames and corrections against the parent's call on the GPU; returns the sequence call's outputs"""
    want = _sequence(frames, *args, **kw)
    st = _stabilizer(frames, *args, **kw)
    try:
        idx, out, corr, _ = _stream_host(st, frames)
    finally:
        st.close()
    assert idx == list(range(len(frames))), f"{what}: emission order {idx}"
    SM.same(out, want[0], f"{what}: out")
    SM.same(corr, want[1], f"{what}: correction")
    return want


def test_pushes_and_a_flush_equal_the_sequence_call_and_the_cpu_chain():
    frames, path, cpu = scene(0)
    want = _against_the_sequence_call(frames, _scene_args(), "uint8")
    SM.same(want[0], cpu[0], "the sequence call against the CPU chain: out")
    SM.same(want[1], cpu[1], "the sequence call against the CPU chain: correction")
    assert (want[0] != frames).any(), "the frames are moved"
    # the first 13 frames: the last pushed frame, 12, is a detection frame, and its newborn must not count
    assert 12 % SCENE["D"] == 0
    _against_the_sequence_call(frames[:13], _scene_args(), "13 frames")
    _against_the_sequence_call(frames.astype(np.float32), _scene_args(), "float32")


@pytest.mark.parametrize("r", [0, 1, 20])
def test_other_radii_equal_the_sequence_call(r):
    """r = 0: every push emits its own frame under the identity; r = 20 > T: everything comes at the flush"""
    frames, _, _ = scene(0)
    want = _against_the_sequence_call(frames, _scene_args(r), f"r={r}")
    if r == 0:
        SM.same(want[0], frames, "r = 0 moves nothing")


def test_a_long_stream_wraps_both_rings_many_times():
    """70 frames of 24 x 32 at two levels, r = 5, D = 8: the delay line of 6 frames and the ring of 10 steps wrap many times"""
    frames, _ = SM.jitter_scene(9, T=70, H=24, W=32)
    want = _against_the_sequence_call(frames, (16, 8, 0.05, 3.0, MM.SIMILARITY, 32, 1.0, 2, SM.weights(5)), "70 frames", levels=2)
    assert want[3][:, 2].sum() > 35, "most steps are fitted"


def test_an_odd_width_takes_the_element_wise_warp():
    frames, _ = SM.jitter_scene(4, T=10, H=24, W=33)
    want = _against_the_sequence_call(frames, (16, 4, 0.05, 3.0, MM.TRANSLATION, 32, 1.0, 1, SM.weights(2)), "24 x 33", levels=2)
    assert want[3][:, 2].sum() >= 5 and (want[0] != frames).any()
    _against_the_sequence_call(frames.astype(np.float32), (16, 4, 0.05, 3.0, MM.TRANSLATION, 32, 1.0, 1, SM.weights(2)),
                               "24 x 33 float32", levels=2)


def test_a_frame_without_texture_holds_its_steps():
    frames = scene(0)[0].copy()
    frames[6] = 128
    want = _against_the_sequence_call(frames, _scene_args(), "a constant frame")
    assert want[4][5] == 1 and want[4][6] == 1 and want[4].sum() < 13, "the steps into and out of frame 6 are held"


def test_emission_on_the_device_writes_only_what_it_emits():
    """push_device on a side stream: d_out and d_inside keep their preset bytes while nothing is emitted; every emitted frame
    equals push's, its inside mask warp_affine's under the map of correction_device, whose rows equal the returned ones;
    the workspace does not grow after the first push"""
    import torch

    frames, _, _ = scene(0)
    T, H, W = frames.shape
    args = _scene_args()
    r = SCENE["r"]
    host = _stabilizer(frames, *args)
    dev = _stabilizer(frames, *args)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    try:
        idx, out, corr, ins = _stream_host(host, frames, inside=True)
        host_bytes = host.workspace_bytes
        d_frames = torch.from_numpy(frames).to("cuda:0")
        d_out = torch.full((r, H, W), 77, dtype=torch.uint8, device="cuda:0")
        d_ins = torch.full((r, H, W), 9, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert dev.workspace_bytes == 0
        grown = None
        for t in range(T):
            e = dev.push_device(d_frames[t].data_ptr(), d_out.data_ptr(), d_ins.data_ptr(), s)
            assert e == (t - r if t >= r else -1) and dev.frame_index == t and dev.tracker.frame_index == t
            grown = dev.workspace_bytes if grown is None else grown
            assert dev.workspace_bytes == grown > 0, "no later push allocates"
            side.synchronize()
            if e < 0:
                assert (d_out == 77).all() and (d_ins == 9).all(), f"frame {t}: nothing is emitted, nothing is written"
                with pytest.raises(ValueError):
                    dev.correction_device()
                continue
            SM.same(d_out[0].cpu().numpy(), out[e], f"frame {e}: out")
            SM.same(d_ins[0].cpu().numpy(), ins[e], f"frame {e}: inside")
            assert (d_out[1:] == 77).all() and (d_ins[1:] == 9).all()
            pc, pm = dev.correction_device()
            SM.same(_from_device(pc, (6,), "<f4"), corr[e], f"frame {e}: correction_device")
            mp = _from_device(pm, (1, 6), "<f8")
            w_out, w_ins = _warp_device(frames[e:e + 1], mp)
            SM.same(w_out[0], out[e], f"frame {e}: warp_affine under the device map")
            SM.same(w_ins[0], ins[e], f"frame {e}: warp_affine's inside")
        first, count = dev.flush_device(d_out.data_ptr(), d_ins.data_ptr(), s)
        side.synchronize()
        assert (first, count) == (T - r, r) and dev.workspace_bytes == grown
        SM.same(d_out.cpu().numpy(), out[T - r:], "the flush: out")
        SM.same(d_ins.cpu().numpy(), ins[T - r:], "the flush: inside")
        pc, pm = dev.correction_device()
        SM.same(_from_device(pc, (r, 6), "<f4"), corr[T - r:], "the flush: correction_device")
        assert dev.flush_device(d_out.data_ptr(), 0, s) == (T, 0), "a second flush emits nothing"
        assert host_bytes == grown + (1 + frames.itemsize) * H * W, "the host forms add one staged frame and one mask"
        assert ins.any() and not ins.all(), "the border is marked"
    finally:
        host.close()
        dev.close()


def test_two_stabilisers_reset_and_the_refused_push():
    """two stabilisers fed in turn do not disturb each other; a push after a flush is refused and writes nothing; after a
    reset the same frames give the same bytes; the inner tracker's rows and motion are a plain tracker's"""
    import torch

    import _oflk
    import sparse_replenish_model as RM

    frames, _, _ = scene(0)
    other, _ = SM.jitter_scene(1)
    args = _scene_args()
    K, D, q, md, fam, hyps, thr, seed, _ = args
    a, b = _stabilizer(frames, *args), _stabilizer(other, *args)
    solo = _stabilizer(other, *args)
    plain = _oflk.Tracker(0, frames.shape[1], frames.shape[2], True, K, D, 3, 5, 3, quality_level=q, min_distance=md)
    try:
        plain.set_motion(fam, hyps, thr, seed)
        want_b = _stream_host(solo, other)
        got_a, got_b = [], []
        for t in range(len(frames)):
            got_a.append(a.push(np.ascontiguousarray(frames[t])))
            got_b.append(b.push(np.ascontiguousarray(other[t])))
            row, motion = plain.push(np.ascontiguousarray(frames[t])), plain.read_motion()
            inner = a.tracker.read_row()
            RM.same((inner[0], inner[1], inner[2], np.int32([inner[5]]), inner[4]), (row[0], row[1], row[2], np.int32([row[5]]), row[4]),
                    f"the inner tracker's row {t}")
            assert np.array_equal(inner[3][inner[1] != 0], row[3][row[1] != 0])
            for g, x, name in zip(a.tracker.read_motion(), motion, ("model", "inlier", "counts")):
                SM.same(g, x, f"the inner tracker's motion of step {t - 1}: {name}")
            pm = a.tracker.motion_device()
            SM.same(_from_device(pm[0], (6,), "<f4"), motion[0], f"motion_device of step {t - 1}")
            SM.same(_from_device(pm[2], (3,), "<i4"), motion[2], f"motion_device of step {t - 1}: counts")
        fa, fb = a.flush(), b.flush()
        r = SCENE["r"]
        out_b = np.stack([g[1] for g in got_b if g[0] >= 0] + list(fb[1]))
        corr_b = np.stack([g[2] for g in got_b if g[0] >= 0] + list(fb[2]))
        SM.same(out_b, want_b[1], "two at once: out")
        SM.same(corr_b, want_b[2], "two at once: correction")
        out_a = np.stack([g[1] for g in got_a if g[0] >= 0] + list(fa[1]))
        # a push after the flush: refused, the frame index stays, nothing is written
        d_frame = torch.from_numpy(frames[0]).to("cuda:0")
        d_out = torch.full(frames[0].shape, 77, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(ValueError):
            a.push_device(d_frame.data_ptr(), d_out.data_ptr())
        with pytest.raises(ValueError):
            a.push(np.ascontiguousarray(frames[0]))
        torch.cuda.synchronize()
        assert (d_out == 77).all() and a.frame_index == len(frames) - 1
        nbytes = a.workspace_bytes
        a.reset()
        assert a.frame_index == -1 and a.tracker.frame_index == -1
        again = _stream_host(a, frames)
        SM.same(again[1], out_a, "after a reset: out")
        assert a.workspace_bytes == nbytes, "a reset keeps the state"
    finally:
        for x in (a, b, solo, plain):
            x.close()


def test_the_python_class_returns_the_same_arrays():
    import lucas_kanade_pyramidal as P

    frames, _, _ = scene(0)
    s = SCENE
    T = len(frames)
    want = P.lucas_kanade_pyramidal_sequence_stabilize(frames, s["K"], s["D"], model="translation", radius=s["r"], sigma=s["sigma"],
                                                       hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"], quality_level=s["q"],
                                                       min_distance=s["md"])
    plain = P.SparseKltTracker(frames.shape[1:], s["K"], s["D"], quality_level=s["q"], min_distance=s["md"],
                               motion=dict(model="translation", hypotheses=s["hyps"], threshold=s["thr"], seed=s["seed"]))
    with P.OnlineStabilizer(frames.shape[1:], s["K"], s["D"], model="translation", radius=s["r"], sigma=s["sigma"], hypotheses=s["hyps"],
                            threshold=s["thr"], seed=s["seed"], quality_level=s["q"], min_distance=s["md"], inside=True) as st, plain:
        assert st.lag == s["r"] and st.frame_index == -1
        got = []
        for t, f in enumerate(frames):
            e = st.push(f)
            assert (e is None) == (t < s["r"]) and st.frame_index == t
            got += [] if e is None else [e]
            row, motion = plain.push(f), plain.motion()
            mine, mm = st.row(), st.motion()
            assert np.array_equal(mine.visible, row.visible) and np.array_equal(mine.born, row.born) and mine.detected == row.detected
            SM.same(mine.xy, row.xy, f"row {t}")
            SM.same(mm.model, motion.model, f"motion of step {t - 1}")
            assert (mm.status, mm.n_inliers, mm.n_valid) == (motion.status, motion.n_inliers, motion.n_valid)
        rest = st.flush()
        assert len(rest) == s["r"] and st.flush() == []
        got += rest
        with pytest.raises(ValueError):
            st.push(frames[0])
        assert [g.index for g in got] == list(range(T))
        SM.same(np.stack([g.frame for g in got]), want.frames, "frames")
        SM.same(np.stack([g.correction for g in got]), want.correction, "correction")
        assert got[3].correction.shape == (2, 3) and got[3].inside.dtype == bool and got[3].inside.shape == frames.shape[1:]
        _, mp, _ = SM.trajectory(want.model.reshape(T - 1, 6), np.stack([want.status] * 3, -1), T, SM.weights(s["r"], s["sigma"]))
        SM.same(np.stack([g.inside for g in got]), SM.warp(frames, mp)[1].astype(bool), "inside")
