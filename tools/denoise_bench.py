#!/usr/bin/env python3
"""Temporal denoising on the dense flows: the sequence call host to host beside the forward-backward call a caller has today,
and the kernel alone (development tool, not part of the bench contract).

Host part: --frames frames of 1080p uint8 (a synthetic scene drifting by one row and two columns per frame, with seeded noise),
oflk_denoise_sequence_u8 at every radius of --radii (flow_median 9, beta 4.0, count asked for) against
oflk_pyramidal_sequence_fb_median_u8 with every output at the same median, wall time per call in rotating order in one
session: median, minimum and maximum over --steps calls of each.

Kernel part: the library has no device-pointer form of the denoising, so the kernel's time is read from a kernel trace.  Run
the host part under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/denoise_bench.py --only denoise`,
then `python tools/denoise_bench.py --trace DIR` with the same --frames, --radii, --steps and --warmup: the k_denoise launches
of the trace are taken in order, a call's launches are summed (the chunk walk launches once per chunk that lets frames out),
and the median, minimum and maximum per call and the time per frame are printed for every radius, beside the traffic of
reading every frame and flow plane once and writing every frame and count once at STREAM_RATE.

    python tools/denoise_bench.py [--frames 129] [--radii 1,2,4] [--steps 10] [--warmup 2] [--only denoise] [--trace DIR]
"""
import argparse
import csv
import glob
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))

STREAM_RATE = 4.3e12   # bytes / s: the middle of the 4.0 - 4.6 TB/s the streamed flow step reaches (README, status)
MEDIAN, ALPHA, BETA, STRENGTH = 9, 0.01, 4.0, 30.0


def chunk_pairs(B, H, W):
    """the library's chunk rule (chunk_pairs, oflk.hip)"""
    pair_out = H * W * 4
    C = max(1, (32 << 20) // max(pair_out, 1))
    return C if B >= 4 * C and B * pair_out >= (64 << 20) else B


def launches_per_call(T, H, W, R):
    """the k_denoise launches of one oflk_denoise_sequence call: one for every chunk after which frames come out"""
    B = T - 1
    C = chunk_pairs(B, H, W)
    n, nxt = 0, 0
    for b0 in range(0, B, C):
        top = b0 + min(C, B - b0)
        end = T if top == B else top - R + 1
        if end > nxt:
            n, nxt = n + (end - nxt + 65534) // 65535, end
    return n


def from_trace(args, radii):
    T, H, W = args.frames, args.height, args.width
    rows = []
    for f in glob.glob(args.trace + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_denoise<" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    calls = args.warmup + args.steps
    want = sum(launches_per_call(T, H, W, R) * calls for R in radii)
    if len(rows) != want:
        sys.exit(f"the trace holds {len(rows)} k_denoise launches, {want} expected for these settings")
    at = 0
    for R in radii:
        n = launches_per_call(T, H, W, R)
        per_call = [sum(d for _, d in rows[at + k * n:at + (k + 1) * n]) * 1e-6 for k in range(calls)][args.warmup:]
        at += n * calls
        traffic = T * H * W * (1 + 1 + 1) + (T - 1) * H * W * 16   # frames in, frames and counts out, four flow planes a pair
        med = statistics.median(per_call)
        print(json.dumps({"kernel": "k_denoise<unsigned char, true, false>", "radius": R, "frames": T, "launches_per_call": n,
                          "ms_median_min_max": [round(x, 3) for x in (med, min(per_call), max(per_call))],
                          "us_per_frame": round(med * 1e3 / T, 2), "traffic_bound_ms": round(traffic / STREAM_RATE * 1e3, 3),
                          "times_the_bound": round(med / (traffic / STREAM_RATE * 1e3), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--radii", default="1,2,4")
    ap.add_argument("--steps", type=int, default=10, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", choices=["denoise"], help="leave the forward-backward call out (for a kernel trace)")
    ap.add_argument("--trace", help="a directory with rocprofv3's *kernel_trace.csv of an --only denoise run: print the kernel's times")
    args = ap.parse_args()
    radii = [int(x) for x in args.radii.split(",")]
    if args.trace:
        return from_trace(args, radii)
    import numpy as np
    import torch

    import _oflk
    from oflk_synth import synth_pair

    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    base = torch.from_numpy(synth_pair(H, W, pair_index=args.seed)[0]).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    host = np.empty((T, H, W), np.uint8)
    for t in range(T):
        noise = torch.randn((H, W), generator=gen, device=dev) * 1.5
        host[t] = torch.round(torch.clamp(torch.roll(base, shifts=(t, 2 * t), dims=(0, 1)) + noise, 0.0, 255.0)).to(torch.uint8).cpu().numpy()
    del base
    torch.cuda.empty_cache()
    L = _oflk.lib()
    out, count = np.empty_like(host), np.empty_like(host)

    def denoise(R):
        def call():
            _oflk.check(L.oflk_denoise_sequence_u8(host.ctypes.data, T, H, W, 3, 5, 3, ALPHA, BETA, MEDIAN, R, STRENGTH, out.ctypes.data,
                                                   count.ctypes.data))
        return call

    forms = [(f"oflk_denoise_sequence_u8 radius {R}", denoise(R)) for R in radii]
    if args.only is None:
        fl = [np.empty((T - 1, H, W), np.float32) for _ in range(6)]
        ok = [np.empty((T - 1, H, W), np.uint8) for _ in range(2)]

        def fb():
            _oflk.check(L.oflk_pyramidal_sequence_fb_median_u8(host.ctypes.data, T, H, W, 3, 5, 3, ALPHA, BETA, MEDIAN, *(_oflk.ptr(a) for a in fl),
                                                               ok[0].ctypes.data, ok[1].ctypes.data))

        forms.append(("oflk_pyramidal_sequence_fb_median_u8, every output", fb))
        wall = {name: [] for name, _ in forms}
        for _ in range(args.warmup):   # plans, device buffers, the pages of the host arrays
            for _, f in forms:
                f()
        for k in range(args.steps):
            for name, f in (forms if k % 2 == 0 else forms[::-1]):
                t0 = time.perf_counter()
                f()
                wall[name].append((time.perf_counter() - t0) * 1e3)
    else:   # a call's launches must stay together in the trace: every radius in turn, warm-up calls included
        wall = {name: [] for name, _ in forms}
        for name, f in forms:
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                f()
                if k >= args.warmup:
                    wall[name].append((time.perf_counter() - t0) * 1e3)
    for name, ms in wall.items():
        print(json.dumps({"host": "1080p u8" if (H, W) == (1080, 1920) else f"{H} x {W} u8", "frames": T, "flow_median": MEDIAN, "call": name,
                          "ms_median_min_max": [round(x, 1) for x in (statistics.median(ms), min(ms), max(ms))],
                          "share_with_a_neighbour": round(float((count > 0).mean()), 3) if "denoise" in name else None}), flush=True)


if __name__ == "__main__":
    main()
