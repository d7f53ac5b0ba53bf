#!/usr/bin/env python3
"""k_pyr_down on one kind of 1080p frames: time per launch.

    python3 tools/pyr_redo.py --frames bench|dots [--pairs 8]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="bench", choices=["bench", "dots"])
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch

    import _oflk
    from oflk_synth import synth_pair

    B, H, W = args.pairs, 1080, 1920
    if args.frames == "bench":
        host = [synth_pair(H, W, i) for i in range(min(B, 4))]
    else:   # single 255 dots on black, one every 23 rows and 29 columns
        f = np.zeros((H, W), np.float32)
        f[5::23, 7::29] = 255.0
        host = [(f, np.roll(f, (1, 2), axis=(0, 1)))]
    dev = torch.device("cuda", 0)
    prev = torch.stack([torch.from_numpy(host[b % len(host)][0]) for b in range(B)]).to(dev)
    curr = torch.stack([torch.from_numpy(host[b % len(host)][1]) for b in range(B)]).to(dev)
    u, v = torch.empty_like(prev), torch.empty_like(prev)
    st = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    for _ in range(2):
        plan.pyramidal(prev.data_ptr(), curr.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    torch.cuda.synchronize()
    plan.set_profiling(True)
    for _ in range(args.reps):
        plan.pyramidal(prev.data_ptr(), curr.data_ptr(), u.data_ptr(), v.data_ptr(), st)
    torch.cuda.synchronize()
    t = plan.kernel_times()["pyr_down_fused"]
    out = {"frames": args.frames, "pairs": B, "lib": str(_oflk.LIB_PATH.name),
           "pyr_down_us_per_launch": round(1e3 * t["total_ms"] / t["launches"], 1), "launches": t["launches"]}
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
