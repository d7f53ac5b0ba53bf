#!/usr/bin/env python3
"""The median filter of dense flows: the kernel beside the flow pass it follows, the host-to-host interpolation call with and
without it, and what it does to the interpolation of the pan scenes (development tool, not part of the bench contract).

Device part: the four flow planes of --pairs pairs of 1080p frames (a synthetic scene drifting by one row and two columns per
frame, with seeded noise; uint8), from one bidirectional plan pass whose time is taken too, then for every size of --sizes the
time of one oflk_flow_median call on all 4 * pairs planes: median, minimum and maximum over the steps, HIP events around each
call.  Beside it the traffic bound of one read and one write of every plane at STREAM_RATE, the rate the project's streaming
kernels reach, and the ratio to the flow pass.

Host part (--host-frames, 0 skips it): oflk_interpolate_sequence_u8 against oflk_interpolate_sequence_median_u8 at
flow_median = 5 and n = 1 on the same host frames, wall time per call, in rotating order.

Quality part: tests/interp_model.pan_scene at pans (3, 1) and (6, -2), lucas_kanade_pyramidal_sequence_interpolate at tau = 0.5
with flow_median 0, 5 and 9: the mean absolute error against the true middle frame and the share of status 3, 12 px inside
the border.

    python tools/flow_median_bench.py [--pairs 128] [--steps 10] [--warmup 2] [--sizes 3,5,7,9] [--host-frames 129] [--host-steps 3]
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

HBM_PEAK = 8.0e12      # bytes / s, MI355X
STREAM_RATE = 4.3e12   # bytes / s: the middle of the 4.0 - 4.6 TB/s the streamed flow step reaches (README, status)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=10, help="timed calls of each form (at most 100)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sizes", default="3,5,7,9")
    ap.add_argument("--host-frames", type=int, default=129)
    ap.add_argument("--host-steps", type=int, default=3)
    args = ap.parse_args()
    steps = max(1, min(args.steps, 100))
    import numpy as np
    import torch

    import _oflk
    import interp_model as M
    import lucas_kanade_pyramidal as P
    from oflk_synth import synth_pair

    dev = torch.device("cuda", 0)
    B, H, W = args.pairs, args.height, args.width
    base = torch.from_numpy(synth_pair(H, W, pair_index=args.seed)[0]).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)

    def video(T):
        f = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
        for t in range(T):
            noise = torch.randn((H, W), generator=gen, device=dev) * 1.5
            f[t] = torch.round(torch.clamp(torch.roll(base, shifts=(t, 2 * t), dims=(0, 1)) + noise, 0.0, 255.0)).to(torch.uint8)
        return f

    def timed(call):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    frames = video(B + 1)
    st = torch.cuda.current_stream().cuda_stream
    flows = torch.empty((4, B, H, W), dtype=torch.float32, device=dev)
    fp = [flows[i].data_ptr() for i in range(4)]
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    flow_ms = timed(lambda: plan.pyramidal_sequence_fb(frames.data_ptr(), *fp, st, u8=True))
    plan.resolve_uncertain_sequence_fb(frames.data_ptr(), *fp, st, u8=True)
    torch.cuda.synchronize()
    plan.close()
    print(json.dumps({"call": "oflk_plan_pyramidal_sequence_fb_u8", "pairs": B, "ms": [round(x, 3) for x in flow_ms]}), flush=True)
    out = torch.empty_like(flows)
    planes = 4 * B
    bound_ms = 2.0 * planes * H * W * 4 / STREAM_RATE * 1e3
    for size in (int(x) for x in args.sizes.split(",")):
        ms = timed(lambda: _oflk.flow_median(flows.data_ptr(), out.data_ptr(), planes, H, W, size, st))
        print(json.dumps({"kernel": f"k_flow_median<{size}>", "planes": planes, "ms_median_min_max": [round(x, 3) for x in ms],
                          "traffic_bound_ms": round(bound_ms, 3), "times_the_bound": round(ms[0] / bound_ms, 2),
                          "share_of_hbm_peak": round(2.0 * planes * H * W * 4 / (ms[0] * 1e-3) / HBM_PEAK, 4),
                          "share_of_the_flow_pass": round(ms[0] / flow_ms[0], 3),
                          "changed_share": round(float((out != flows).float().mean()), 4)}), flush=True)
    del frames, flows, out
    torch.cuda.empty_cache()

    T = args.host_frames
    if T >= 2:
        host = video(T).cpu().numpy()
        torch.cuda.empty_cache()
        L = _oflk.lib()
        new, status, taus = np.empty((T - 1, 1, H, W), np.uint8), np.empty((T - 1, 1, H, W), np.uint8), np.array([0.5])

        def plain():
            _oflk.check(L.oflk_interpolate_sequence_u8(host.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 2, _oflk._f64(taus), 1,
                                                       new.ctypes.data, status.ctypes.data))

        def median():
            _oflk.check(L.oflk_interpolate_sequence_median_u8(host.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 2, _oflk._f64(taus), 1, 5,
                                                              new.ctypes.data, status.ctypes.data))

        wall = {"plain": [], "median": []}
        forms = [("plain", plain), ("median", median)]
        for _, f in forms:   # warm-up: plans, device buffers, the pages of the host arrays
            f()
        for k in range(max(1, args.host_steps)):
            for name, f in (forms if k % 2 == 0 else forms[::-1]):
                t0 = time.perf_counter()
                f()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"host": "1080p u8", "frames": T, "n": 1,
                          "oflk_interpolate_sequence_u8_ms": [round(x, 1) for x in sorted(wall["plain"])],
                          "oflk_interpolate_sequence_median_u8_5_ms": [round(x, 1) for x in sorted(wall["median"])]}), flush=True)

    inner = (slice(12, -12), slice(12, -12))
    for pan in ((3, 1), (6, -2)):
        A, mid, B_ = M.pan_scene(*pan)
        row = {"pan": list(pan)}
        for k in (0, 5, 9):
            r = P.lucas_kanade_pyramidal_sequence_interpolate(np.stack([A, B_]), taus=[0.5], flow_median=k)
            row[f"median_{k}"] = [round(float(np.abs(r.new[0, 0] - mid)[inner].mean()), 3),
                                  round(float((r.status[0, 0][inner] == 3).mean()), 3)]
        print(json.dumps({"quality": "error / share of status 3", **row}), flush=True)


if __name__ == "__main__":
    main()
