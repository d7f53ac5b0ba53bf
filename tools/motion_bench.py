#!/usr/bin/env python3
"""Device time of the global motion fit (development tool, not part of the bench contract).

Leg 1, the fit alone: one step of K correspondences on the device (a planted similarity, 30 % outliers, every slot valid),
K in (1 000, 10 000), Hn in (64, 256, 1 024), each of the kernel family's four models (the homography through
oflk_homography_workspace and oflk_estimate_homography, nine floats per model).  Events around `--reps` back-to-back calls of
oflk_estimate_motion give the time per step; one JSON line per (K, Hn, family) with the median over `--steps` such batches.
The split into the three launches comes from a separate run under `rocprofv3 --kernel-trace --stats`.

Leg 2 (--push), the online tracker: on 1080p uint8 frames (tools/sparse_bench.py's scene), K in (1 000, 10 000) and
detect_every 4, the device time of a non-detecting oflk_tracker_push_device in the steady state with the motion row on
(similarity, Hn 256) against the same push with it off, two trackers taking turns on every frame.  One JSON line per K.

    python tools/motion_bench.py [--steps 5] [--reps 20] [--budgets 1000,10000] [--hypotheses 64,256,1024] [--push] [--frames 41]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))
sys.path.insert(0, str(ROOT / "tests"))

FAMILIES = ["translation", "similarity", "affine", "homography"]   # index = the kernels' model code


def fit_leg(args):
    import numpy as np
    import torch

    import _oflk
    import motion_model as MM

    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    for K in args.budgets:
        src, dst, planted = MM.planted_scene(K, 0.3, 1)
        t_src, t_dst = torch.from_numpy(src).to(d), torch.from_numpy(dst).to(d)
        out = torch.empty(9, device=d)
        inl = torch.empty(K, dtype=torch.uint8, device=d)
        cnt = torch.empty(3, dtype=torch.int32, device=d)
        for hyps in args.hypotheses:
            for code, family in enumerate(FAMILIES):
                nb = (_oflk.homography_workspace if family == "homography" else _oflk.motion_workspace)(1, K, hyps)
                ws = torch.empty(nb, dtype=torch.uint8, device=d)

                def call():
                    if family == "homography":
                        _oflk.estimate_homography(t_src.data_ptr(), t_dst.data_ptr(), 0, 1, K, ws.data_ptr(), nb, out.data_ptr(),
                                                  inl.data_ptr(), cnt.data_ptr(), hyps, 1.0, 0, 0, st)
                    else:
                        _oflk.estimate_motion(t_src.data_ptr(), t_dst.data_ptr(), 0, 1, K, ws.data_ptr(), nb, out.data_ptr(),
                                              inl.data_ptr(), cnt.data_ptr(), code, hyps, 1.0, 0, 0, st)

                call()
                torch.cuda.synchronize()
                us = []
                for _ in range(args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        call()
                    b.record()
                    b.synchronize()
                    us.append(a.elapsed_time(b) * 1e3 / args.reps)
                c = cnt.cpu().numpy()
                print(json.dumps({"tool": "motion_bench", "leg": "fit", "K": K, "hypotheses": hyps, "model": family,
                                  "us_per_step": round(statistics.median(us), 2),
                                  "us_min_max": [round(min(us), 2), round(max(us), 2)], "reps": args.reps, "steps": args.steps,
                                  "n_inliers": int(c[0]), "planted": int(planted.sum()), "workspace_bytes": nb}), flush=True)


def push_leg(args):
    import numpy as np
    import torch

    import _oflk
    from oflk_synth import synth_pair

    T, H, W = args.frames, 1080, 1920
    base = synth_pair(H, W, pair_index=0)[0].astype(np.float32)
    rng = np.random.default_rng(0)
    frames = np.empty((T, H, W), np.uint8)
    for t in range(T):
        f = np.roll(base, (t, 2 * t), axis=(0, 1)) + rng.normal(0.0, 1.5, (H, W)).astype(np.float32)
        frames[t] = np.rint(np.clip(f, 0.0, 255.0)).astype(np.uint8)
    d_frames = torch.from_numpy(frames).to("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for K, md in zip(args.budgets, (10.0, 4.0) if len(args.budgets) == 2 else [4.0] * len(args.budgets)):
        tk = {"off": _oflk.Tracker(0, H, W, True, K, 4, 3, 5, 3, 0.01, 0.5, 4.0, 0.01, md),
              "on": _oflk.Tracker(0, H, W, True, K, 4, 3, 5, 3, 0.01, 0.5, 4.0, 0.01, md)}
        tk["on"].set_motion(1, 256, 1.0, 0)
        ms = {"off": [], "on": []}
        try:
            for t in range(T):
                for k in (("off", "on") if t % 2 == 0 else ("on", "off")):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    tk[k].push_device(d_frames[t].data_ptr(), st)
                    b.record()
                    b.synchronize()
                    if t >= 8 and t % 4 != 0:
                        ms[k].append(a.elapsed_time(b) * 1e3)
            cnt = tk["on"].read_motion()[2]
        finally:
            for x in tk.values():
                x.close()
        print(json.dumps({"tool": "motion_bench", "leg": "push", "K": K, "min_distance": md, "frames": T, "detect_every": 4,
                          "model": "similarity", "hypotheses": 256, "samples": len(ms["on"]),
                          "push_off_us": round(statistics.median(ms["off"]), 2), "push_on_us": round(statistics.median(ms["on"]), 2),
                          "push_off_us_min_max": [round(min(ms["off"]), 2), round(max(ms["off"]), 2)],
                          "push_on_us_min_max": [round(min(ms["on"]), 2), round(max(ms["on"]), 2)],
                          "last_counts": cnt.tolist()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--budgets", type=lambda v: [int(x) for x in v.split(",")], default=[1000, 10000])
    ap.add_argument("--hypotheses", type=lambda v: [int(x) for x in v.split(",")], default=[64, 256, 1024])
    ap.add_argument("--push", action="store_true", help="time the tracker's push with the motion row on and off instead")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

    if args.push:
        push_leg(args)
    else:
        fit_leg(args)


if __name__ == "__main__":
    main()
