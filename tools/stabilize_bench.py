#!/usr/bin/env python3
"""Device time of the stabiliser's warp and host-to-host time of the sequence call (development tool, not part of the bench
contract).

Leg 1, the warp: oflk_warp_affine on F = 32 device frames of 1080p, float32 and uint8, under the identity map and under a
2 degree rotation with a 3.5 px shift, against a device-to-device copy of the same [F][H][W] tensor in the same process: the
copy moves the same algorithmic bytes, read once and written once, and is the ceiling.  The two take turns; events around
`--reps` back-to-back calls give the time per frame; one JSON line per (type, map) with the median over `--steps` batches.

Leg 2 (--sequence): oflk_stabilize_sequence_u8 on `--frames` 1080p uint8 frames (tools/sparse_bench.py's scene), K = 1000,
D = 4, host arrays in and out, next to oflk_pyramidal_sequence_klt_sparse_replenish_u8 on the same frames: what
stabilisation adds is the second upload, the warp and the download.  Wall clock, the two taking turns; one JSON line.

    python tools/stabilize_bench.py [--steps 7] [--reps 10] [--sequence] [--frames 129]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))
sys.path.insert(0, str(ROOT / "tests"))


def scene(T, H, W):
    import numpy as np

    from oflk_synth import synth_pair

    base = synth_pair(H, W, pair_index=0)[0].astype(np.float32)
    rng = np.random.default_rng(0)
    frames = np.empty((T, H, W), np.uint8)
    for t in range(T):
        f = np.roll(base, (t, 2 * t), axis=(0, 1)) + rng.normal(0.0, 1.5, (H, W)).astype(np.float32)
        frames[t] = np.rint(np.clip(f, 0.0, 255.0)).astype(np.uint8)
    return frames


def warp_leg(args):
    import numpy as np
    import torch

    import _oflk

    F, H, W = 32, 1080, 1920
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    th = np.deg2rad(2.0)
    c, s = np.cos(th), np.sin(th)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    maps = {"identity": [1, 0, 0, 0, 1, 0],
            "rotation 2 deg, shift 3.5 px": [c, -s, cx - (c * cx - s * cy) + 3.5, s, c, cy - (s * cx + c * cy) + 3.5]}
    frames8 = torch.from_numpy(scene(F, H, W)).to(d)
    for u8 in (False, True):
        src = frames8 if u8 else frames8.to(torch.float32)
        out, cpy = torch.empty_like(src), torch.empty_like(src)
        for name, m in maps.items():
            t_map = torch.from_numpy(np.tile(np.float64(m), (F, 1))).to(d)

            def warp():
                _oflk.warp_affine(src.data_ptr(), F, H, W, t_map.data_ptr(), out.data_ptr(), 0, u8, st)

            def copy():
                cpy.copy_(src)

            us = {"warp": [], "copy": []}
            for fn in (warp, copy):
                fn()
            torch.cuda.synchronize()
            for step in range(args.steps):
                for k, fn in ((("warp", warp), ("copy", copy)) if step % 2 == 0 else (("copy", copy), ("warp", warp))):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        fn()
                    b.record()
                    b.synchronize()
                    us[k].append(a.elapsed_time(b) * 1e3 / args.reps / F)
            wm, cm = statistics.median(us["warp"]), statistics.median(us["copy"])
            nbytes = 2 * H * W * src.element_size()
            print(json.dumps({"tool": "stabilize_bench", "leg": "warp", "pixels": "uint8" if u8 else "float32", "map": name, "F": F,
                              "H": H, "W": W, "warp_us_per_frame": round(wm, 2), "copy_us_per_frame": round(cm, 2),
                              "warp_over_copy": round(wm / cm, 3), "warp_TBps": round(nbytes / wm * 1e-6, 3),
                              "copy_TBps": round(nbytes / cm * 1e-6, 3),
                              "warp_us_min_max": [round(min(us["warp"]), 2), round(max(us["warp"]), 2)],
                              "copy_us_min_max": [round(min(us["copy"]), 2), round(max(us["copy"]), 2)], "reps": args.reps,
                              "steps": args.steps}), flush=True)


def sequence_leg(args):
    import numpy as np

    import _oflk

    T, H, W, K, D = args.frames, 1080, 1920, 1000, 4
    frames = scene(T, H, W)
    L = _oflk.lib()
    w = _oflk.stabilize_weights(15)
    out = np.empty_like(frames)
    corr, model = np.empty((T, 6), np.float32), np.empty((T - 1, 6), np.float32)
    counts, held = np.empty((T - 1, 3), np.int32), np.empty(T - 1, np.uint8)
    tr, vis, born = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8), np.empty((T, K), np.uint8)
    det = np.empty(T, np.int32)

    def stabilize():
        _oflk.check(L.oflk_stabilize_sequence_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 4.0, 0.01, 10.0, K, D, 1, 256, 1.0, 0,
                                                 _oflk._f64(w), 15, out.ctypes.data, _oflk.ptr(corr), _oflk.ptr(model),
                                                 counts.ctypes.data_as(_oflk._i32p), held.ctypes.data))

    def track():
        _oflk.check(L.oflk_pyramidal_sequence_klt_sparse_replenish_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 4.0, 0.01, 10.0,
                                                                      K, D, _oflk.ptr(tr), vis.ctypes.data, born.ctypes.data,
                                                                      det.ctypes.data_as(_oflk._i32p), None))

    ms = {"stabilize": [], "track": []}
    stabilize()
    track()
    for step in range(args.steps):
        for k, fn in ((("stabilize", stabilize), ("track", track)) if step % 2 == 0 else (("track", track), ("stabilize", stabilize))):
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    sm, tm = statistics.median(ms["stabilize"]), statistics.median(ms["track"])
    print(json.dumps({"tool": "stabilize_bench", "leg": "sequence", "frames": T, "H": H, "W": W, "K": K, "detect_every": D,
                      "model": "similarity", "hypotheses": 256, "radius": 15, "stabilize_ms": round(sm, 1), "track_ms": round(tm, 1),
                      "added_ms": round(sm - tm, 1), "stabilize_ms_per_frame": round(sm / T, 3), "track_ms_per_frame": round(tm / T, 3),
                      "stabilize_ms_min_max": [round(min(ms["stabilize"]), 1), round(max(ms["stabilize"]), 1)],
                      "track_ms_min_max": [round(min(ms["track"]), 1), round(max(ms["track"]), 1)], "steps": args.steps,
                      "fitted_steps": int(counts[:, 2].sum()), "held_steps": int(held.sum()),
                      "moved_frames": int((corr != np.float32([1, 0, 0, 0, 1, 0])).any(1).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--sequence", action="store_true", help="time the sequence call host to host instead")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

    if args.sequence:
        sequence_leg(args)
    else:
        warp_leg(args)


if __name__ == "__main__":
    main()
