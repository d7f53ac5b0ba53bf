#!/usr/bin/env python3
"""Frame sequence against the equivalent pair batch (development tool, not part of the bench contract).

Both inputs are device-resident and hold the same seeded content: T frames of 1080p (a synthetic scene drifting by one
row and two columns per frame, with seeded noise), and the T-1 pairs (f[b], f[b+1]) as two separate arrays.  For each
arithmetic mode one plan of T-1 pairs runs both forms, alternating which goes first, for a bounded number of steps; the
tool prints one JSON line per mode with ms per call (median over the steps), Gpix/s of flow, the pyr_down time per call
from the plan's kernel profiling, and whether the two forms' outputs are byte-equal.

    python tools/seq_bench.py [--frames 129] [--steps 10] [--warmup 2]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))

MODES = {"exact": 0, "tolerant": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=10, help="timed calls of each form per mode (at most 100)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.frames < 2:
        ap.error("--frames must be >= 2")
    steps = max(1, min(args.steps, 100))
    import numpy as np
    import torch

    import _oflk
    from oflk_synth import synth_pair

    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    B = T - 1
    base = torch.from_numpy(synth_pair(H, W, pair_index=args.seed)[0]).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    frames = torch.empty((T, H, W), dtype=torch.float32, device=dev)
    for t in range(T):
        noise = torch.randn((H, W), generator=gen, device=dev) * 1.5
        frames[t] = torch.clamp(torch.roll(base, shifts=(t, 2 * t), dims=(0, 1)) + noise, 0.0, 255.0)
    prev, curr = frames[:-1].clone(), frames[1:].clone()
    out = {f: (torch.empty((B, H, W), dtype=torch.float32, device=dev), torch.empty((B, H, W), dtype=torch.float32, device=dev))
           for f in ("sequence", "pairs")}
    st = torch.cuda.current_stream().cuda_stream

    for mode, arith in MODES.items():
        plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
        plan.set_arithmetic(arith)

        def call(form):
            u, v = out[form]
            if form == "sequence":
                plan.pyramidal_sequence(frames.data_ptr(), u.data_ptr(), v.data_ptr(), st)
            else:
                plan.pyramidal(prev.data_ptr(), curr.data_ptr(), u.data_ptr(), v.data_ptr(), st)

        try:
            for _ in range(args.warmup):
                for form in ("sequence", "pairs"):
                    call(form)
            torch.cuda.synchronize()
            ms = {"sequence": [], "pairs": []}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for i in range(steps):
                for form in (("sequence", "pairs") if i % 2 == 0 else ("pairs", "sequence")):
                    e0.record()
                    call(form)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[form].append(e0.elapsed_time(e1))
            # kernel classes from the plan's own HIP-event brackets, in separate profiled calls
            pyr = {}
            for form in ("sequence", "pairs"):
                plan.set_profiling(True)
                for _ in range(3):
                    call(form)
                times = plan.kernel_times()
                plan.set_profiling(False)
                pyr[form] = sum(t["total_ms"] for n, t in times.items() if n.startswith("pyr_") or n == "blur") / 3
            equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out["sequence"], out["pairs"]))
            logs = {}
            for form in ("sequence", "pairs"):   # residual log, iteration counts and flags of each form
                call(form)
                logs[form] = plan.read_log(st) + (plan.read_uncertain(st),)
            equal = equal and all(np.array_equal(x, y) for x, y in zip(logs["sequence"], logs["pairs"]))
        finally:
            plan.close()
        line = {"tool": "seq_bench", "mode": mode, "frames": T, "pairs": B, "height": H, "width": W, "levels": 3, "window": 5,
                "iters": 3, "steps": steps, "outputs_byte_equal": bool(equal)}
        for form in ("sequence", "pairs"):
            m = statistics.median(ms[form])
            line[f"{form}_ms"] = round(m, 4)
            line[f"{form}_gpix_s"] = round(B * H * W / (m * 1e-3) / 1e9, 3)
            line[f"{form}_pyr_down_ms"] = round(pyr[form], 4)
        line["speedup"] = round(line["pairs_ms"] / line["sequence_ms"], 4)
        line["pyr_down_ratio"] = round(pyr["sequence"] / pyr["pairs"], 4) if pyr["pairs"] else None
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
