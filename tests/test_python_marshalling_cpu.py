"""What the Python tier hands to the C ABI, call by call: every public entry point that takes tracking, fit, trajectory-window,
refine or alignment settings, the _oflk bindings that tests and tools use directly, and the other calls that share their
pixel-type dispatch, map parsing or integer checks (flows of a pair, features, warps, mosaic composites and chains), run once
per pixel type and layout against a stub in place of liboflk.so.  The stub records (name, args) of every call and returns 0; nothing here needs the
library or a device.

Pinned per recorded C call, in tests/golden/python_marshalling.json: the function's name, every scalar argument's Python
type and exact value (its repr) position by position, and for every pointer argument whether it is NULL.  Which positions
are pointers is read from _oflk.SIGNATURES, which tests/test_abi.py holds to the header.  The file was recorded from the
modules before their settings became records (`python tests/test_python_marshalling_cpu.py --write` records the modules it
imports); the outputs of the stubbed calls are whatever np.empty left, so only what goes in is compared.

The stub fills two outputs, without which a later call of the same entry point would be refused on the host: the canvas
box of oflk_mosaic_canvas and of oflk_mosaic_sequence[_u8] (8 x 8 at the origin)."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "python_marshalling.json"
T, H, W, K = 3, 24, 32, 4


class StubLib:
    """stands in for the loaded library: any attribute is a callable that records (name, args) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            if name == "oflk_last_error":
                return b""
            self.calls.append((name, args))
            if name == "oflk_mosaic_canvas":                        # (box, dropped, T, &x0, &y0, &Wc, &Hc)
                args[5]._obj.value = args[6]._obj.value = 8
            if name in ("oflk_mosaic_sequence", "oflk_mosaic_sequence_u8"):
                args[22][2] = args[22][3] = 8                       # canvas (x0, y0, Wc, Hc)
            return 0
        return fn


def encode(name, args):
    """one recorded call as text: pointers as ptr / NULL, scalars as their repr (which tells 2 from 2.0 from True)"""
    import _oflk

    types = _oflk.SIGNATURES[name][1]
    assert len(args) == len(types), (name, len(args), len(types))
    words = []
    for a, t in zip(args, types):
        if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
            words.append("NULL" if a is None or not a else "ptr")
        else:
            words.append(repr(a))
    return f"{name}({', '.join(words)})"


def recorded(monkeypatch, thunk):
    """the calls `thunk` makes, encoded, with the stub in the library's place"""
    import _oflk

    stub = StubLib()
    monkeypatch.setattr(_oflk, "_lib", stub)
    thunk()
    return [encode(name, args) for name, args in stub.calls]


def frames(kind):
    ramp = (np.arange(T * H * W, dtype=np.int64).reshape(T, H, W) * 7) % 251
    if kind == "u8":
        return ramp.astype(np.uint8)
    if kind == "f32":
        return ramp.astype(np.float32)
    if kind == "colour":
        return np.stack([ramp, ramp[::-1], ramp // 2], axis=-1).astype(np.uint8)
    assert kind == "nv12"
    return np.concatenate([ramp, ramp[:, :H // 2]], axis=1).astype(np.uint8)


KLT = dict(num_levels=2, window_size=7, num_iterations=4, alpha=0.03, beta=0.25)
SELECT = dict(max_corners=K, quality_level=0.02, min_distance=3.0)
FIT = dict(hypotheses=64, threshold=1.5, seed=7)
WINDOW = dict(radius=2, sigma=1.5)
REFINES = {"": {}, "refine": dict(refine_iterations=2, refine_levels=2),
           "refine_photo_robust": dict(refine_iterations=2, refine_levels=2, refine_photometric=True, refine_robust_delta=4.5)}
QUERIES3 = np.float32([[0, 5, 6], [1, 7.5, 8.25]])
QUERIES2 = np.float32([[5, 6], [7.5, 8.25]])
TRACKS = np.arange(T * K * 2, dtype=np.float32).reshape(T, K, 2)
VISIBLE = np.ones((T, K), bool)
BORN = np.zeros((T, K), bool)
PTR = 0x100000


def cases():
    """label -> thunk; the imports happen when a thunk runs"""
    import _oflk
    import lucas_kanade_core as C
    import lucas_kanade_pyramidal as P

    out = {}
    for px in ("f32", "u8"):
        f = frames(px)
        out[f"klt-{px}"] = lambda f=f: P.lucas_kanade_pyramidal_sequence_klt(f, **SELECT, **KLT)
        out[f"klt_replenish-{px}"] = lambda f=f: P.lucas_kanade_pyramidal_sequence_klt_replenish(f, detect_every=2, **SELECT, **KLT)
        out[f"sparse_tracks-{px}"] = lambda f=f: P.lucas_kanade_pyramidal_sequence_sparse_tracks(f, QUERIES3, max_residual=5.0, **KLT)
        out[f"sparse_tracks-frame0-{px}"] = lambda f=f: P.lucas_kanade_pyramidal_sequence_sparse_tracks(f, QUERIES2, max_residual=5.0, **KLT)
        out[f"klt_sparse-{px}"] = lambda f=f: P.lucas_kanade_pyramidal_sequence_klt_sparse(f, max_residual=5.0, **SELECT, **KLT)
        out[f"klt_sparse_replenish-{px}"] = lambda f=f: P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(
            f, detect_every=2, max_residual=5.0, **SELECT, **KLT)
        out[f"sparse-{px}"] = lambda f=f: P.lucas_kanade_sparse(f[0], f[1], QUERIES2, 2, 7, 4)
        out[f"tracker-{px}"] = lambda px=px: P.SparseKltTracker((H, W), detect_every=2, max_residual=5.0, **SELECT, **KLT,
                                                                 dtype=np.uint8 if px == "u8" else np.float32, device=1)
        out[f"online-{px}"] = lambda px=px: P.OnlineStabilizer((H, W), detect_every=2, model="affine", max_residual=5.0, **SELECT,
                                                                **KLT, **FIT, **WINDOW, dtype=np.uint8 if px == "u8" else np.float32,
                                                                device=1)
        for kind in ("homography", "affine"):
            nc = 9 if kind == "homography" else 6
            m1, m2 = np.ones((T, nc), np.float32), np.ones((T - 1, nc), np.float32)
            st1, st2 = np.ones(T, np.int32), np.ones(T - 1, np.int32)
            for form, kw in (("plain", {}), ("photo", dict(photometric=True)), ("robust", dict(robust_delta=4.5)),
                             ("robust_photo", dict(robust_delta=4.5, photometric=True))):
                out[f"refine_alignment-{kind}-{form}-{px}"] = lambda f=f, m=m1, st=st1, kind=kind, kw=kw: C.refine_alignment(
                    f, f[::-1].copy(), m, st, kind, 2, 4, 0.5, **kw)
                out[f"sequence_refine_alignment-{kind}-{form}-{px}"] = lambda f=f, m=m2, kind=kind, kw=kw: C.sequence_refine_alignment(
                    f, m, None, kind, 2, 4, 0.5, **kw)
                out[f"_oflk.align_host-{kind}-{form}-{px}"] = lambda f=f, m=m1, m2=m2, st=st1, kind=kind, kw=kw: (
                    (_oflk.align_robust_host(f, f, m, st, 2, 4, _oflk.ALIGN_KINDS[kind], 0.5, 4.5, "photometric" in kw),
                     _oflk.align_robust_host(f, None, m2, None, 2, 4, _oflk.ALIGN_KINDS[kind], 0.5, 4.5, "photometric" in kw))
                    if "robust_delta" in kw else
                    (_oflk.align_host(f, f, m, st, 2, 4, _oflk.ALIGN_KINDS[kind], 0.5, "photometric" in kw),
                     _oflk.align_host(f, None, m2, None, 2, 4, _oflk.ALIGN_KINDS[kind], 0.5, "photometric" in kw)))
        m1 = np.ones((T, 9), np.float32)
        out[f"alignment_weights-{px}"] = lambda f=f, m=m1: C.alignment_weights(f, f[::-1].copy(), m, "homography", 4.5)
        out[f"alignment_weights-photo-{px}"] = lambda f=f, m=m1: C.alignment_weights(f, f[::-1].copy(), m, "homography", 4.5, 1.25, [1.0, 2.0, 3.0])
        out[f"_oflk.align_weights_host-{px}"] = lambda f=f, m=m1: (
            _oflk.align_weights_host(f, f, m, 1, 4.5), _oflk.align_weights_host(f, f, m, 1, 4.5, np.ones((T, 2), np.float32)))
    for px in ("f32", "u8", "colour"):
        f = frames(px)
        for name, kw in REFINES.items():
            label = f"-{name}" if name else ""
            out[f"stabilize{label}-{px}"] = lambda f=f, kw=kw: P.lucas_kanade_pyramidal_sequence_stabilize(
                f, detect_every=2, model="affine", max_residual=5.0, **SELECT, **KLT, **FIT, **WINDOW,
                **(dict(order="bgr") if f.ndim == 4 else {}), **kw)
            out[f"mosaic{label}-{px}"] = lambda f=f, kw=kw: P.lucas_kanade_pyramidal_sequence_mosaic(
                f, detect_every=2, max_residual=5.0, anchor=1, extent=100.0, blend="mean", max_pixels=5000, **SELECT, **KLT, **FIT,
                **(dict(order="bgr") if f.ndim == 4 else {}), **kw)
    f = frames("nv12")
    for name, kw in (("", {}), ("-refine_robust", dict(refine_iterations=2, refine_levels=2, refine_robust_delta=4.5))):
        out[f"stabilize_nv12{name}"] = lambda f=f, kw=kw: P.lucas_kanade_pyramidal_sequence_stabilize_nv12(
            f, detect_every=2, model="affine", max_residual=5.0, siting="center", **SELECT, **KLT, **FIT, **WINDOW, **kw)
    out["mosaic-defaults-u8"] = lambda: P.lucas_kanade_pyramidal_sequence_mosaic(frames("u8"))
    out["detect_every-2^40"] = lambda: (
        P.lucas_kanade_pyramidal_sequence_klt_replenish(frames("u8"), K, 2 ** 40),
        P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames("u8"), K, 2 ** 40),
        P.lucas_kanade_pyramidal_sequence_stabilize(frames("u8"), K, 2 ** 40),
        P.lucas_kanade_pyramidal_sequence_stabilize(frames("colour"), K, 2 ** 40),
        P.lucas_kanade_pyramidal_sequence_stabilize_nv12(frames("nv12"), K, 2 ** 40),
        P.lucas_kanade_pyramidal_sequence_mosaic(frames("u8"), K, 2 ** 40),
        P.SparseKltTracker((H, W), K, 2 ** 40), P.OnlineStabilizer((H, W), K, 2 ** 40))
    out["integers-as-int64-and-float"] = lambda: (
        P.lucas_kanade_pyramidal_sequence_klt_sparse_replenish(frames("u8"), np.int64(K), 2.0, num_levels=np.int64(2), num_iterations=4.0),
        P.lucas_kanade_pyramidal_sequence_stabilize(frames("u8"), 4.0, np.int64(2), radius=2.0, hypotheses=np.int64(64), seed=7.0,
                                                    refine_iterations=0.0),
        P.lucas_kanade_pyramidal_sequence_mosaic(frames("u8"), K, 2, anchor=np.int64(1), max_pixels=5000.0),
        P.SparseKltTracker((H, W), K, 0.0), C.refine_alignment(frames("u8"), frames("u8"), np.ones((T, 9), np.float32), None,
                                                               "homography", np.int64(2), 4.0))

    def tracker_motion():
        t = P.SparseKltTracker((H, W), K, motion="translation")
        t.set_motion("affine", **FIT)
        t.set_motion(None)
        P.SparseKltTracker((H, W), K, motion=dict(model="similarity", hypotheses=8, threshold=2.5, seed=3))
    out["tracker-set_motion"] = tracker_motion
    out["online-colour"] = lambda: P.OnlineStabilizer((H, W, 4), detect_every=2, model="affine", max_residual=5.0, **SELECT, **KLT,
                                                      **FIT, **WINDOW, order="bgr", device=1)
    out["online-nv12"] = lambda: P.OnlineStabilizer((H, W), detect_every=2, model="affine", max_residual=5.0, **SELECT, **KLT, **FIT,
                                                    **WINDOW, layout="nv12", siting="center", device=1)
    src = TRACKS[:-1]
    out["tracks_motion"] = lambda: C.tracks_motion(TRACKS, VISIBLE, BORN, "affine", **FIT, t0=5)
    out["estimate_motion"] = lambda: (C.estimate_motion(src, src + 1, None, "translation", **FIT, step0=5),
                                      C.estimate_motion(src[0], src[0] + 1, VISIBLE[0], "similarity", **FIT))
    out["tracks_homography"] = lambda: C.tracks_homography(TRACKS, VISIBLE, None, **FIT, t0=5)
    out["estimate_homography"] = lambda: (C.estimate_homography(src, src + 1, None, **FIT, step0=5),
                                          C.estimate_homography(src[0], src[0] + 1, VISIBLE[0], **FIT))
    out["stabilize_trajectory"] = lambda: (C.stabilize_trajectory(np.ones((T - 1, 2, 3), np.float32), [1, 0], **WINDOW),
                                           C.stabilize_trajectory(np.ones((T - 1, 6), np.float32), None, 3),
                                           C.stabilize_trajectory(np.zeros((0, 6), np.float32), None, 0))
    out["_oflk.align_workspace"] = lambda: (_oflk.align_workspace(2, H, W, 3, 1), _oflk.align_workspace(2, H, W, 3, 1, True),
                                            _oflk.align_workspace(2, H, W, 3, 0, False, True), _oflk.align_workspace(2, H, W, 3, 0, True, True))
    d_io = (PTR + 0x1000, 0, PTR + 0x10000, 1 << 20, PTR + 0x3000, PTR + 0x4000, PTR + 0x5000)
    for u8 in (False, True):
        out[f"_oflk.align_refine-u8={u8}"] = lambda u8=u8: (
            _oflk.align_refine(PTR, PTR + 0x100, 2, H, W, 2, 4, 1, 0.5, *d_io, u8, 9),
            _oflk.align_refine(PTR, PTR + 0x100, 2, H, W, 2, 4, 1, 0.5, *d_io, u8, 9, PTR + 0x6000),
            _oflk.align_refine(PTR, PTR + 0x100, 2, H, W, 2, 4, 1, 0.5, *d_io, u8, 9, None, 4.5),
            _oflk.align_refine(PTR, PTR + 0x100, 2, H, W, 2, 4, 1, 0.5, *d_io, u8, 9, PTR + 0x6000, 4.5))
        out[f"_oflk.align_sequence-u8={u8}"] = lambda u8=u8: (
            _oflk.align_sequence(PTR, T, H, W, 2, 4, 0, 0.5, *d_io, u8, 9),
            _oflk.align_sequence(PTR, T, H, W, 2, 4, 0, 0.5, *d_io, u8, 9, PTR + 0x6000),
            _oflk.align_sequence(PTR, T, H, W, 2, 4, 0, 0.5, *d_io, u8, 9, None, 4.5),
            _oflk.align_sequence(PTR, T, H, W, 2, 4, 0, 0.5, *d_io, u8, 9, PTR + 0x6000, 4.5))
        out[f"_oflk.align_weights-u8={u8}"] = lambda u8=u8: (
            _oflk.align_weights(PTR, PTR + 0x100, 2, H, W, 1, 4.5, PTR + 0x1000, 0, PTR + 0x8000, u8, 9),
            _oflk.align_weights(PTR, PTR + 0x100, 2, H, W, 1, 4.5, PTR + 0x1000, PTR + 0x6000, PTR + 0x8000, u8))
    w = np.array([1.0, 0.5, 0.25])
    out["_oflk.Tracker"] = lambda: (_oflk.Tracker(1, H, W, True, K, 2, 2, 7, 4, 0.03, 0.25, 5.0, 0.02, 3.0), _oflk.Tracker(0, H, W, False, K, 0))
    out["_oflk.Stabilizer"] = lambda: (
        _oflk.Stabilizer(1, H, W, True, K, 2, 2, w, 64, 1.5, 7, 2, 7, 4, 0.03, 0.25, 5.0, 0.02, 3.0),
        _oflk.Stabilizer(0, H, W, False, K, 2, 1, w),
        _oflk.Stabilizer(1, H, W, True, K, 2, 2, w, 64, 1.5, 7, 2, 7, 4, 0.03, 0.25, 5.0, 0.02, 3.0, 4, 1),
        _oflk.Stabilizer(1, H, W, True, K, 2, 2, w, 64, 1.5, 7, 2, 7, 4, 0.03, 0.25, 5.0, 0.02, 3.0, nv12=True, siting=1))

    def plan_calls():
        plan = _oflk.Plan(0, T - 1, H, W, 2, 7, 4)
        _oflk.sparse_tracks(plan, PTR, PTR + 0x100, 2, PTR + 0x200, PTR + 0x300, 0.03, 0.25, 5.0, 1, PTR + 0x400, True, 9)
        _oflk.sparse_tracks(plan, PTR, PTR + 0x100, 2, PTR + 0x200, PTR + 0x300)
        _oflk.sparse_klt_replenish(plan, PTR, PTR + 0x1000, 4096, PTR + 0x100, PTR + 0x200, PTR + 0x300, PTR + 0x400, PTR + 0x500,
                                   PTR + 0x600, K, 2, 0.02, 3.0, 0.03, 0.25, 5.0, 1, PTR + 0x700, True, 9)
        _oflk.sparse_klt_replenish(plan, PTR, PTR + 0x1000, 4096, PTR + 0x100, PTR + 0x200, PTR + 0x300, PTR + 0x400, PTR + 0x500,
                                   PTR + 0x600, K, 2)
    out["_oflk.sparse_tracks-and-klt_replenish"] = plan_calls
    # the other calls whose pixel-type dispatch, map parsing or integer checks are shared
    aff, per = np.arange(T * 6, dtype=np.float64).reshape(T, 2, 3), np.arange(T * 9, dtype=np.float64).reshape(T, 3, 3)
    for px in ("f32", "u8", "colour"):
        f = frames(px)
        out[f"warp-{px}"] = lambda f=f: (C.warp_affine(f, aff), C.warp_affine(f, aff.reshape(T, 6), True), C.warp_perspective(f, per),
                                         C.warp_perspective(f, per.reshape(T, 9), True))
        out[f"mosaic_composite-{px}"] = lambda f=f: (
            C.mosaic_composite(f, per, (8, 9), (-2, 3), [0, 1, 0], "last", True),
            C.mosaic_composite(f, per.reshape(T, 9), (8, 9), exposure=np.ones((T, 2))))
    for px in ("f32", "u8"):
        f = frames(px)
        out[f"warp-one-frame-{px}"] = lambda f=f: (C.warp_affine(f[0], aff[0]), C.warp_perspective(f[0], per[0].reshape(9), True))
        out[f"single_scale-{px}"] = lambda f=f: C.lucas_kanade_single_scale(f[0], f[1], 7)
        out[f"pyramidal-{px}"] = lambda f=f: (P.lucas_kanade_pyramidal_with_log(f[0], f[1], 2, 7, 4),
                                              P.lucas_kanade_pyramidal_sequence_with_log(f, 2, 7, 4))
        out[f"features-{px}"] = lambda f=f: (
            C.corner_min_eigenvalue(f, 7), C.good_features_to_track_batch(f, **SELECT, window_size=7),
            C.replenish_features(f[0], np.zeros((K, 2), np.float32), np.zeros(K), None, 0.02, 3.0, 7, np.int64(2)),
            C.replenish_features(f[0], np.zeros((K, 2), np.float32), np.ones(K), K, t=3.0, qt=np.zeros(K), qxy=np.zeros((K, 2))))
    nv = frames("nv12")
    out["warp-nv12"] = lambda: (P.warp_affine_nv12(nv, aff, "center"), P.warp_affine_nv12(nv[0], aff[0].reshape(6), return_inside=True),
                                P.warp_perspective_nv12(nv, per.reshape(T, 9), "center", True), P.warp_perspective_nv12(nv[0], per[0]))
    hom = np.ones((T - 1, 3, 3), np.float32)
    out["mosaic_chain"] = lambda: (C.mosaic_chain(hom, [1, 0], (H, W), np.int64(1), 100), C.mosaic_chain(hom.reshape(T - 1, 9), None, (H, W)),
                                   C.mosaic_chain(np.zeros((0, 9), np.float32), None, (H, W), 0.0))
    out["exposure_chain"] = lambda: (C.exposure_chain([1.0, 1.5], [0.0, 2.0], [1, 0], np.int64(2)), C.exposure_chain([1.0, 1.5], [0.0, 2.0]),
                                     C.exposure_chain([], [], None, 0.0))
    out["_oflk.mosaic_accumulate"] = lambda: (
        _oflk.mosaic_accumulate(PTR, T, H, W, PTR + 0x100, 0, -2, 3, 8, 9, 1, PTR + 0x1000, 4096),
        _oflk.mosaic_accumulate(PTR, T, H, W, PTR + 0x100, PTR + 0x200, -2, 3, 8, 9, 3, PTR + 0x1000, 4096, True, 9, PTR + 0x300),
        _oflk.mosaic_accumulate(PTR, T, H, W, PTR + 0x100, 0, -2, 3, 8, 9, 1, PTR + 0x1000, 4096, d_exposure=0))
    return out


def labels():
    return sorted(json.loads(GOLDEN.read_text())) if GOLDEN.exists() else []


@pytest.mark.parametrize("label", labels())
def test_the_c_calls_of_an_entry_point_are_the_recorded_ones(label, monkeypatch):
    got = recorded(monkeypatch, cases()[label])
    assert got == json.loads(GOLDEN.read_text())[label]


def test_every_case_is_recorded_and_makes_a_call():
    golden = json.loads(GOLDEN.read_text())
    assert sorted(golden) == sorted(cases())
    assert all(golden.values())


def test_detect_every_is_clamped_and_integers_may_come_as_int64_or_float():
    """2^40 goes to the library as 2^31 - 1, on every path that takes it; np.int64(2) and 2.0 go as the int 2"""
    golden = json.loads(GOLDEN.read_text())
    clamped = [c for c in golden["detect_every-2^40"] if not c.startswith("oflk_stabilizer_tracker(")]
    assert len(clamped) == 8 and all(f", {2 ** 31 - 1}, " in c or c.endswith(f", {2 ** 31 - 1})") for c in clamped)
    assert not any(str(2 ** 40) in c for c in clamped)
    plain = golden["integers-as-int64-and-float"]
    assert len(plain) == 5 and not any("int64" in c for c in plain)
    assert plain[0].startswith("oflk_pyramidal_sequence_klt_sparse_replenish_u8(ptr, 3, 24, 32, 2, 5, 4, ") and ", 4, 2, ptr" in plain[0]
    assert ", 4, 2, 1, 64, 1.0, 7, ptr, 2, ptr" in plain[1] and ", 0, 1, 256.0, 1, ptr, 5000, ptr" in plain[2]
    assert plain[3].endswith(", 4, 0)") and plain[4].startswith("oflk_align_refine_host_u8(ptr, ptr, 3, 24, 32, 2, 4, 1, ")


if __name__ == "__main__":   # record the modules that are importable: --write stores, otherwise the table is printed
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "optical-flow-fpga_amd", "python"))
    os.environ.setdefault("OFLK_QUIET", "1")
    monkeypatch = pytest.MonkeyPatch()
    table = {label: recorded(monkeypatch, thunk) for label, thunk in cases().items()}
    monkeypatch.undo()
    text = json.dumps(table, indent=0, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        GOLDEN.write_text(text)
    else:
        print(text)
