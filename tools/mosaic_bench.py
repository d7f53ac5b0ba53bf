#!/usr/bin/env python3
"""Device time of the mosaic's accumulate + resolve against the same picture assembled from the perspective warp (development
tool, not part of the bench contract).

Scene "pan": F = 129 uint8 frames of 1080p, all resident on the device, frame f under the planted projective row
(2e-5, -1e-5, 1) after a shift of 24 f px: the canvas is about 2.6 frames wide and a canvas pixel is covered by at most 84 of
the 129 frames.  Scene "still": the same frames all under the one map of frame 0, the canvas that frame's box: every frame
covers every pixel and the cull can save nothing, which prices it.

Legs, each in a process of its own under its own time limit (a leg that fails or runs out of time ends the run):
  mean, feather   oflk_mosaic_accumulate (one launch for the F frames, on a state cleared in the same window) and
                  oflk_mosaic_resolve with the count
  median          oflk_mosaic_median with the count: one launch, no state.  A pixel of the pan is covered by up to 84 frames,
                  one of the still scene by all 129: both are beyond twice oflk_mosaic_median_capacity(), the still scene
                  everywhere, so the frames are walked two and three times there
  baseline        what the library offered before: the frames padded to the canvas size (prepared outside the timed window),
                  oflk_warp_perspective with inside over them, the sum and the count over the frames taken with torch
Events around `--reps` back-to-back repetitions give one window; one JSON line per leg with the median and min - max over
`--steps` windows, the number of covered (pixel, frame) pairs and the time per covered pair.

  resolve         (only with --leg resolve) oflk_mosaic_resolve alone, uint8 output with the count, on the pan's canvas made
                  `--extra-columns` wider (a width that is a multiple of 4 takes the dword store, any other the byte store);
                  the state holds the first 4 frames under exposures that put a third of the pixels beyond either end of the
                  byte range.  Compare two libraries with OFLK_LIB, their runs alternating

    python tools/mosaic_bench.py [--steps 7] [--reps 3] [--frames 129] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))

H, W, PAN = 1080, 1920, 24
ROW = (2e-5, -1e-5, 1.0)


def scene(name, F):
    """(maps (F, 9) from canvas coordinates to frame f's, (x0, y0, Wc, Hc))"""
    import numpy as np

    proj = np.array([[1, 0, 0], [0, 1, 0], ROW])
    maps, lo, hi = [], [], []
    for f in range(F):
        shift = PAN * f if name == "pan" else 0
        m = proj @ np.array([[1, 0, -shift], [0, 1, 0], [0, 0, 1.0]])
        maps.append((m / m[2, 2]).reshape(9))
        c = np.linalg.inv(m) @ np.array([[0, W - 1, W - 1, 0], [0, 0, H - 1, H - 1], [1, 1, 1, 1.0]])
        c = c[:2] / c[2]
        lo.append(c.min(1))
        hi.append(c.max(1))
    x0, y0 = (int(v) for v in np.floor(np.min(lo, 0)))
    x1, y1 = (int(v) for v in np.ceil(np.max(hi, 0)))
    return np.array(maps), (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def leg(args):
    import numpy as np
    import torch

    import _oflk

    F = args.frames
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    maps, (x0, y0, Wc, Hc) = scene(args.scene, F)
    rng = np.random.default_rng(0)
    if args.leg == "resolve":
        Wc += args.extra_columns
    frames = torch.from_numpy(rng.integers(0, 256, (4 if args.leg == "resolve" else F, H, W), dtype=np.uint8)).to(d)
    out = torch.empty((Hc, Wc), dtype=torch.uint8, device=d)
    count = torch.empty((Hc, Wc), dtype=torch.int32, device=d)
    if args.leg == "baseline":
        padded = torch.zeros((F, Hc, Wc), dtype=torch.uint8, device=d)
        padded[:, :H, :W] = frames
        shifted = np.stack([(m.reshape(3, 3) @ np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1.0]])).reshape(9) for m in maps])
        t_map = torch.from_numpy(shifted).to(d)
        warped, inside = torch.empty_like(padded), torch.empty_like(padded)

        # A padded frame is the frame with zeros to its right and below, and the warp's `inside` is that of the padded size:
        # it also counts samples of the pad.  A faithful assembly needs one more masking pass per frame; this stand-in leaves
        # it out, which flatters the baseline's time and makes its covered_pairs an overcount.
        def run():
            _oflk.warp_perspective(padded.data_ptr(), F, Hc, Wc, t_map.data_ptr(), warped.data_ptr(), inside.data_ptr(), True, st)
            s = torch.sum(warped, 0, dtype=torch.float32)
            count.copy_(torch.sum(inside, 0, dtype=torch.int32))
            out.copy_(torch.where(count > 0, s / count.clamp(min=1), torch.zeros_like(s)).round().to(torch.uint8))
    elif args.leg == "resolve":
        nbytes = _oflk.mosaic_state_bytes(Hc, Wc)
        state = torch.zeros(nbytes, dtype=torch.uint8, device=d)
        t_map = torch.from_numpy(maps[:4].copy()).to(d)
        t_exp = torch.from_numpy(np.array([[3.0, -255.0]] * 4)).to(d)
        _oflk.mosaic_accumulate(frames.data_ptr(), 4, H, W, t_map.data_ptr(), 0, x0, y0, Hc, Wc, _oflk.MOSAIC_BLENDS["mean"], state.data_ptr(),
                                nbytes, True, st, t_exp.data_ptr())

        def run():
            _oflk.mosaic_resolve(state.data_ptr(), Hc, Wc, out.data_ptr(), count.data_ptr(), True, st)
    elif args.leg == "median":
        t_map = torch.from_numpy(maps).to(d)

        def run():
            _oflk.mosaic_median(frames.data_ptr(), F, H, W, t_map.data_ptr(), 0, 0, x0, y0, Hc, Wc, out.data_ptr(), count.data_ptr(), True, st)
    else:
        blend = _oflk.MOSAIC_BLENDS[args.leg]
        nbytes = _oflk.mosaic_state_bytes(Hc, Wc)
        state = torch.empty(nbytes, dtype=torch.uint8, device=d)
        t_map = torch.from_numpy(maps).to(d)

        def run():
            state.zero_()
            _oflk.mosaic_accumulate(frames.data_ptr(), F, H, W, t_map.data_ptr(), 0, x0, y0, Hc, Wc, blend, state.data_ptr(), nbytes,
                                    True, st)
            _oflk.mosaic_resolve(state.data_ptr(), Hc, Wc, out.data_ptr(), count.data_ptr(), True, st)

    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / args.reps)
    pairs = int(count.sum(dtype=torch.int64).item())
    med = statistics.median(ms)
    print(json.dumps({"tool": "mosaic_bench", "scene": args.scene, "leg": args.leg, "F": F, "H": H, "W": W, "canvas": [Wc, Hc],
                      "origin": [x0, y0], "ms": round(med, 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                      "covered_pairs": pairs, "pairs_over_canvas_times_F": round(pairs / (Wc * Hc * F), 4),
                      "ns_per_covered_pair": round(med * 1e6 / max(pairs, 1), 4),
                      "us_per_frame_area_covered": round(med * 1e3 / max(pairs / (H * W), 1e-9), 2),
                      "max_count": int(count.max().item()), "reps": args.reps, "steps": args.steps,
                      **({"us_per_resolve": round(med * 1e3, 2), "us_min_max": [round(min(ms) * 1e3, 2), round(max(ms) * 1e3, 2)],
                          "bytes_at_0_and_255": [int((out == 0).sum().item()), int((out == 255).sum().item())],
                          "library": os.environ.get("OFLK_LIB", "")} if args.leg == "resolve" else {})}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--scene", choices=["pan", "still"])
    ap.add_argument("--leg", choices=["mean", "feather", "median", "baseline", "resolve"], help="run this one leg in this process")
    ap.add_argument("--extra-columns", type=int, default=0, help="the resolve leg: columns added to the canvas")
    args = ap.parse_args()
    if args.leg:
        import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

        leg(args)
        return 0
    for sc in ("pan", "still"):
        for lg in ("mean", "feather", "median", "baseline"):
            cmd = [sys.executable, __file__, "--scene", sc, "--leg", lg, "--steps", str(args.steps), "--reps", str(args.reps),
                   "--frames", str(args.frames)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps({"tool": "mosaic_bench", "scene": sc, "leg": lg, "error": f"no result within {args.limit} s"}), flush=True)
                return 1
            if rc != 0:   # nothing more is started on the device after a leg that failed
                print(json.dumps({"tool": "mosaic_bench", "scene": sc, "leg": lg, "error": f"exit status {rc}"}), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
