#!/usr/bin/env python3
"""Device time of the colour kernels and host-to-host time of the colour sequence call (development tool, not part of the
bench contract).  Every leg alternates its candidates in one process, device events (or a wall clock around a synchronous
call) around `--reps` back-to-back calls, and prints one JSON line with the median over `--steps` batches and the spread.

Leg "warp" (default): F = 64 uint8 RGB frames of 1080p under a 2 degree rotation (affine) and under a mild homography
(perspective).  Three candidates take turns:
    packed          one oflk_warp_*_packed call on the interleaved frames
    planar          three oflk_warp_affine / oflk_warp_perspective calls on planes split beforehand: what every caller has
                    without the packed kernels; the split and the re-join are not counted
    planar+torch    the same three calls with a torch split ahead of them and a torch re-interleave behind them, counted
The packed call is accepted when its median is no slower than `planar`.  The outputs of the first two are compared byte for
byte before anything is timed.

Leg "luma" (--luma): oflk_luma_u8 on 64 such frames (RGB and RGBA) against a device-to-device copy that moves the same
bytes.  The kernel reads C and writes 1 byte per pixel, so the reference is a copy of (C + 1) F H W / 2 bytes, which reads
and writes as many bytes in total.

Leg "sequence" (--sequence): oflk_stabilize_sequence_packed host to host on `--frames` RGB frames of 1080p against
oflk_stabilize_sequence_u8 on their luma: what colour adds (an upload and a download three times larger, and the luma pass).

    python tools/colour_bench.py [--steps 7] [--reps 5] [--luma | --sequence] [--frames 129]
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
sys.path.insert(0, str(ROOT / "tools"))

GAINS = ((0.9, 10), (0.6, 60), (0.75, 0), (0.5, 100))


def colour_scene(T, H, W, C):
    """stabilize_bench's grey scene, every plane under a gain and an offset of its own: (T, H, W, C) uint8"""
    import numpy as np

    from stabilize_bench import scene

    grey = scene(T, H, W).astype(np.float32)
    out = np.empty((T, H, W, C), np.uint8)
    for c in range(C):
        out[..., c] = np.rint(GAINS[c][0] * grey + GAINS[c][1]).astype(np.uint8)
    return out


def take_turns(cands, steps, reps, per):
    """cands: {name: fn}.  Returns {name: [us per `per` units, one per step]}, the order rotated from step to step"""
    import torch

    names = list(cands)
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in names}
    for step in range(steps):
        order = names[step % len(names):] + names[:step % len(names)]
        for k in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                cands[k]()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / reps / per)
    return us


def summary(us):
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in us.items()}


def warp_leg(args):
    import numpy as np
    import torch

    import _oflk

    F, H, W, C = 64, 1080, 1920, 3
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    th = np.deg2rad(2.0)
    c, s = np.cos(th), np.sin(th)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    rot = [c, -s, cx - (c * cx - s * cy) + 3.5, s, c, cy - (s * cx + c * cy) + 3.5]
    maps = {"affine": rot, "perspective": [1.01, 0.004, -6.0, -0.003, 0.995, 4.0, 4e-6, -3e-6, 1.0]}
    packed = torch.from_numpy(colour_scene(F, H, W, C)).to(d)
    planes = [packed[..., k].contiguous() for k in range(C)]
    out_packed = torch.empty_like(packed)
    out_planes = [torch.empty_like(p) for p in planes]
    for kind, m in maps.items():
        t_map = torch.from_numpy(np.tile(np.float64(m), (F, 1))).to(d)
        warp_packed = _oflk.warp_affine_packed if kind == "affine" else _oflk.warp_perspective_packed
        warp_plane = _oflk.warp_affine if kind == "affine" else _oflk.warp_perspective

        def run_packed():
            warp_packed(packed.data_ptr(), F, H, W, C, t_map.data_ptr(), out_packed.data_ptr(), 0, st)

        def run_planar(src=planes):
            for k in range(C):
                warp_plane(src[k].data_ptr(), F, H, W, t_map.data_ptr(), out_planes[k].data_ptr(), 0, True, st)

        def run_planar_torch():
            run_planar([packed[..., k].contiguous() for k in range(C)])
            return torch.stack(out_planes, dim=-1)

        run_packed()
        joined = run_planar_torch()
        torch.cuda.synchronize()
        same = bool(torch.equal(joined, out_packed))
        us = take_turns({"packed": run_packed, "planar": run_planar, "planar+torch": run_planar_torch}, args.steps, args.reps, F)
        r = summary(us)
        print(json.dumps({"tool": "colour_bench", "leg": "warp", "kind": kind, "F": F, "H": H, "W": W, "C": C, "unit": "us per frame",
                          **r, "packed_over_planar": round(r["packed"]["median_us"] / r["planar"]["median_us"], 3),
                          "packed_over_planar_torch": round(r["packed"]["median_us"] / r["planar+torch"]["median_us"], 3),
                          "accepted": r["packed"]["median_us"] <= r["planar"]["median_us"], "bytes_equal": same,
                          "reps": args.reps, "steps": args.steps}), flush=True)


def luma_leg(args):
    import torch

    import _oflk

    F, H, W = 64, 1080, 1920
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    for C in (3, 4):
        packed = torch.from_numpy(colour_scene(F, H, W, C)).to(d)
        n = F * H * W
        luma = torch.empty((F, H, W), dtype=torch.uint8, device=d)
        moved = n * (C + 1)                      # bytes the kernel reads and writes
        src = torch.empty(moved // 2, dtype=torch.uint8, device=d)
        dst = torch.empty_like(src)              # the copy reads moved / 2 and writes moved / 2

        def run_luma():
            _oflk.luma(packed.data_ptr(), F, H, W, C, luma.data_ptr(), 0, st)

        def run_copy():
            dst.copy_(src)

        r = summary(take_turns({"luma": run_luma, "copy": run_copy}, args.steps, args.reps, F))
        print(json.dumps({"tool": "colour_bench", "leg": "luma", "F": F, "H": H, "W": W, "C": C, "unit": "us per frame", **r,
                          "luma_over_copy": round(r["luma"]["median_us"] / r["copy"]["median_us"], 3),
                          "luma_TBps": round(moved / F / r["luma"]["median_us"] * 1e-6, 3),
                          "copy_TBps": round(moved / F / r["copy"]["median_us"] * 1e-6, 3), "reps": args.reps, "steps": args.steps}),
              flush=True)


def sequence_leg(args):
    import numpy as np

    import _oflk

    T, H, W, C, K, D = args.frames, 1080, 1920, 3, 1000, 4
    frames = colour_scene(T, H, W, C)
    grey = _oflk.luma_host(frames, 0)
    L = _oflk.lib()
    w = _oflk.stabilize_weights(15)
    out, out_grey = np.empty_like(frames), np.empty_like(grey)
    res = {k: (np.empty((T, 6), np.float32), np.empty((T - 1, 6), np.float32), np.empty((T - 1, 3), np.int32), np.empty(T - 1, np.uint8))
           for k in ("colour", "grey")}
    tail = (3, 5, 3, 0.01, 0.5, 4.0, 0.01, 10.0, K, D, 1, 256, 1.0, 0, _oflk._f64(w), 15)

    def outs(k):
        corr, model, counts, held = res[k]
        return (_oflk.ptr(corr), _oflk.ptr(model), counts.ctypes.data_as(_oflk._i32p), held.ctypes.data)

    def colour():
        _oflk.check(L.oflk_stabilize_sequence_packed(frames.ctypes.data, T, H, W, C, 0, *tail, out.ctypes.data, *outs("colour")))

    def plain():
        _oflk.check(L.oflk_stabilize_sequence_u8(grey.ctypes.data, T, H, W, *tail, out_grey.ctypes.data, *outs("grey")))

    ms = {"colour": [], "grey": []}
    colour()
    plain()
    same = all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(res["colour"], res["grey"]))
    for step in range(args.steps):
        for k, fn in ((("colour", colour), ("grey", plain)) if step % 2 == 0 else (("grey", plain), ("colour", colour))):
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    cm, gm = statistics.median(ms["colour"]), statistics.median(ms["grey"])
    print(json.dumps({"tool": "colour_bench", "leg": "sequence", "frames": T, "H": H, "W": W, "C": C, "K": K, "detect_every": D,
                      "radius": 15, "colour_ms": round(cm, 1), "grey_ms": round(gm, 1), "added_ms": round(cm - gm, 1),
                      "colour_ms_per_frame": round(cm / T, 3), "grey_ms_per_frame": round(gm / T, 3),
                      "colour_ms_min_max": [round(min(ms["colour"]), 1), round(max(ms["colour"]), 1)],
                      "grey_ms_min_max": [round(min(ms["grey"]), 1), round(max(ms["grey"]), 1)], "steps": args.steps,
                      "trajectory_equal": bool(same), "fitted_steps": int(res["colour"][2][:, 2].sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--luma", action="store_true", help="time k_luma against a copy of the same bytes instead")
    ap.add_argument("--sequence", action="store_true", help="time the sequence call host to host instead")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

    if args.sequence:
        sequence_leg(args)
    elif args.luma:
        luma_leg(args)
    else:
        warp_leg(args)


if __name__ == "__main__":
    main()
