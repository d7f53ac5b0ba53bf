#!/usr/bin/env python3
"""Frame interpolation on the dense flows: the kernel beside the forward-backward check, and the host-to-host sequence call
beside the forward-backward sequence call (development tool, not part of the bench contract).

Device part: B pairs of 1080p frames (a synthetic scene drifting by one row and two columns per frame, with seeded noise),
their flows from one bidirectional plan pass, then for every pixel type, n in --ns and refine in --refines the time of one
oflk_interpolate_frames call (median over the steps, HIP events around each call), per output frame, and the share of the
HBM peak that its unique bytes -- (16 B of flows + two pixels) / n + one pixel + one status byte per output pixel -- stand
for; beside it oflk_fb_consistency with every output on the same flows, per pair.

Host part (--host-frames, 0 skips it): oflk_interpolate_sequence_u8 at n = 1 against oflk_pyramidal_sequence_fb_u8 with every
output on the same host frames, wall time per call, alternating which goes first.

    python tools/interp_bench.py [--pairs 32] [--steps 10] [--warmup 2] [--ns 1,3] [--refines 1,2] [--pixels u8,f32]
                                 [--host-frames 129] [--host-steps 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=10, help="timed calls of each form (at most 100)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ns", default="1,3")
    ap.add_argument("--refines", default="1,2")
    ap.add_argument("--pixels", default="u8,f32")
    ap.add_argument("--host-frames", type=int, default=129)
    ap.add_argument("--host-steps", type=int, default=3)
    args = ap.parse_args()
    steps = max(1, min(args.steps, 100))
    import numpy as np
    import torch

    import _oflk
    import lucas_kanade_pyramidal as P
    from oflk_synth import synth_pair

    dev = torch.device("cuda", 0)
    B, H, W = args.pairs, args.height, args.width
    base = torch.from_numpy(synth_pair(H, W, pair_index=args.seed)[0]).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)

    def video(T):
        f = torch.empty((T, H, W), dtype=torch.float32, device=dev)
        for t in range(T):
            noise = torch.randn((H, W), generator=gen, device=dev) * 1.5
            f[t] = torch.clamp(torch.roll(base, shifts=(t, 2 * t), dims=(0, 1)) + noise, 0.0, 255.0)
        return f

    f32 = video(B + 1)
    frames = {"f32": f32, "u8": torch.round(f32).to(torch.uint8)}
    st = torch.cuda.current_stream().cuda_stream
    flows = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(4)]
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    plan.pyramidal_sequence_fb(frames["f32"].data_ptr(), *(t.data_ptr() for t in flows), st)
    plan.resolve_uncertain_sequence_fb(frames["f32"].data_ptr(), *(t.data_ptr() for t in flows), st)
    torch.cuda.synchronize()
    plan.close()
    fp = [t.data_ptr() for t in flows]

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
        return statistics.median(ms)

    chk = [torch.empty((B, H, W), dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.uint8, torch.uint8)]
    fb_ms = timed(lambda: _oflk.fb_consistency(*fp, B, H, W, 0.01, 0.5, *(t.data_ptr() for t in chk), st))
    print(json.dumps({"kernel": "k_fb_check", "pairs": B, "ms_per_pair": round(fb_ms / B, 5),
                      "ms_per_128_pairs": round(fb_ms / B * 128, 3)}), flush=True)
    for pix in args.pixels.split(","):
        px = 1 if pix == "u8" else 4
        for n in (int(x) for x in args.ns.split(",")):
            taus = [(j + 1) / (n + 1) for j in range(n)]
            out = torch.empty((B, n, H, W), dtype=frames[pix].dtype, device=dev)
            status = torch.empty((B, n, H, W), dtype=torch.uint8, device=dev)
            for refine in (int(x) for x in args.refines.split(",")):
                ms = timed(lambda: _oflk.interpolate_frames(frames[pix].data_ptr(), B, H, W, *fp, taus, out.data_ptr(),
                                                            status.data_ptr(), refine=refine, u8=pix == "u8", stream=st))
                per_frame = ms / (B * n)
                unique = ((16 + 2 * px) / n + px + 1) * H * W
                codes = torch.bincount(status.flatten().to(torch.int64), minlength=4).tolist()
                print(json.dumps({"kernel": "k_interp", "pixels": pix, "n": n, "refine": refine, "pairs": B,
                                  "ms_per_output_frame": round(per_frame, 5), "ms_per_pair": round(ms / B, 5),
                                  "unique_bytes_per_output_pixel": round(unique / (H * W), 2),
                                  "share_of_hbm_peak": round(unique / (per_frame * 1e-3) / HBM_PEAK, 4),
                                  "status_share": [round(c / status.numel(), 4) for c in codes]}), flush=True)
            del out, status
    del frames, f32, flows, chk
    torch.cuda.empty_cache()

    T = args.host_frames
    if T >= 2:
        host = torch.round(video(T)).to(torch.uint8).cpu().numpy()
        torch.cuda.empty_cache()
        outs = [np.empty((T - 1, H, W), np.float32) for _ in range(6)] + [np.empty((T - 1, H, W), np.uint8) for _ in range(2)]
        L = _oflk.lib()

        def fb():
            _oflk.check(L.oflk_pyramidal_sequence_fb_u8(host.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, *(_oflk.ptr(o) for o in outs[:6]),
                                                        outs[6].ctypes.data, outs[7].ctypes.data))

        def interp():
            P.lucas_kanade_pyramidal_sequence_interpolate(host, factor=2)

        def c_interp(new=np.empty((T - 1, 1, H, W), np.uint8), status=np.empty((T - 1, 1, H, W), np.uint8),
                     taus=np.array([0.5])):
            _oflk.check(L.oflk_interpolate_sequence_u8(host.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 2, _oflk._f64(taus), 1,
                                                       new.ctypes.data, status.ctypes.data))

        wall = {"fb": [], "interp": [], "interp_python": []}
        forms = [("fb", fb), ("interp", c_interp), ("interp_python", interp)]
        for f in (fb, c_interp):   # warm-up: plans, device buffers, the pages of the host arrays
            f()
        for k in range(max(1, args.host_steps)):
            for name, f in (forms if k % 2 == 0 else forms[::-1]):
                t0 = time.perf_counter()
                f()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in wall.items()}
        print(json.dumps({"host": "1080p u8", "frames": T, "n": 1,
                          "oflk_pyramidal_sequence_fb_u8_ms": round(med["fb"], 1),
                          "oflk_interpolate_sequence_u8_ms": round(med["interp"], 1),
                          "lucas_kanade_pyramidal_sequence_interpolate_ms": round(med["interp_python"], 1),
                          "bytes_down_fb": int((T - 1) * H * W * 26), "bytes_down_interp": int((T - 1) * H * W * 2),
                          "interp_not_slower": bool(med["interp"] <= med["fb"])}), flush=True)


if __name__ == "__main__":
    main()
