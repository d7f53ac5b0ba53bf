#!/usr/bin/env python3
"""Frame interpolation on colour and NV12 video beside what a caller had without it (development tool, not part of the bench
contract).

Device part: B pairs of 1080p frames (interp_bench.py's drifting scene), their flows from one bidirectional plan pass on
the grey scene, then, HIP events around each call, minimum, median and maximum over the steps:
  packed RGB   oflk_interpolate_frames_packed (C = 3) against three oflk_interpolate_frames (u8) calls on planes split
               beforehand, and C = 4 against four
  NV12         oflk_interpolate_frames_nv12 against oflk_interpolate_frames (u8) on the Y planes alone
Host part (--host-frames, 0 skips it): oflk_interpolate_sequence_packed and oflk_interpolate_sequence_nv12 host to host
against oflk_interpolate_sequence_u8 on the grey frames, wall time per call, in rotating order.

    python tools/interp_colour_bench.py [--pairs 128] [--steps 10] [--warmup 3] [--n 1] [--refine 2] [--host-frames 129]
                                        [--host-steps 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=10, help="timed calls of each form (at most 100)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--refine", type=int, default=2)
    ap.add_argument("--host-frames", type=int, default=129)
    ap.add_argument("--host-steps", type=int, default=3)
    args = ap.parse_args()
    steps = max(1, min(args.steps, 100))
    import numpy as np
    import torch

    import _oflk
    from oflk_synth import synth_pair

    dev = torch.device("cuda", 0)
    B, H, W, n = args.pairs, args.height, args.width, args.n
    base = torch.from_numpy(synth_pair(H, W, pair_index=args.seed)[0]).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)

    def video(T):
        f = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
        for t in range(T):
            noise = torch.randn((H, W), generator=gen, device=dev) * 1.5
            f[t] = torch.round(torch.clamp(torch.roll(base, shifts=(t, 2 * t), dims=(0, 1)) + noise, 0.0, 255.0)).to(torch.uint8)
        return f

    def colour(grey, C):   # channels that differ, from one scene
        return torch.stack([grey, 255 - grey, grey // 2 + 40, grey][:C], dim=-1).contiguous()

    def nv12(grey):        # Y is the scene, U and V its 2 x 2 subsampling under two gains
        sub = grey[:, ::2, ::2].to(torch.float32)
        uv = torch.stack([torch.round(0.6 * sub + 60), torch.round(0.75 * sub + 20)], dim=-1).to(torch.uint8)
        return torch.cat([grey, uv.reshape(grey.shape[0], H // 2, W)], dim=1).contiguous()

    grey = video(B + 1)
    st = torch.cuda.current_stream().cuda_stream
    flows = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(4)]
    plan = _oflk.Plan(0, B, H, W, 3, 5, 3)
    plan.pyramidal_sequence_fb(grey.data_ptr(), *(t.data_ptr() for t in flows), st, u8=True)
    plan.resolve_uncertain_sequence_fb(grey.data_ptr(), *(t.data_ptr() for t in flows), st, u8=True)
    torch.cuda.synchronize()
    plan.close()
    fp = [t.data_ptr() for t in flows]
    taus = [(j + 1) / (n + 1) for j in range(n)]

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
        return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}

    status = torch.empty((B, n, H, W), dtype=torch.uint8, device=dev)
    out_y = torch.empty((B, n, H, W), dtype=torch.uint8, device=dev)

    def grey_call(plane):
        _oflk.interpolate_frames(plane.data_ptr(), B, H, W, *fp, taus, out_y.data_ptr(), status.data_ptr(), refine=args.refine,
                                 u8=True, stream=st)

    for C in (3, 4):
        packed = colour(grey, C)
        planes = [packed[..., c].contiguous() for c in range(C)]   # split beforehand: not timed
        out = torch.empty((B, n, H, W, C), dtype=torch.uint8, device=dev)
        layout = _oflk.FrameLayout("_packed", (C,))
        one = timed(lambda: _oflk.interpolate_frames_layout(layout, packed.data_ptr(), B, H, W, *fp, taus, out.data_ptr(),
                                                            status.data_ptr(), refine=args.refine, stream=st))
        planar = timed(lambda: [grey_call(p) for p in planes])
        print(json.dumps({"layout": f"packed C={C}", "pairs": B, "n": n, "refine": args.refine,
                          "oflk_interpolate_frames_packed_ms": one, f"{C}_planar_u8_calls_ms": planar,
                          "ratio_of_medians": round(one["median"] / planar["median"], 3)}), flush=True)
        del packed, planes, out
    frames = nv12(grey)
    out = torch.empty((B, n, 3 * H // 2, W), dtype=torch.uint8, device=dev)
    ys = grey
    for siting in (0, 1):
        layout = _oflk.FrameLayout("_nv12", (siting,))
        one = timed(lambda: _oflk.interpolate_frames_layout(layout, frames.data_ptr(), B, H, W, *fp, taus, out.data_ptr(),
                                                            status.data_ptr(), refine=args.refine, stream=st))
        y_only = timed(lambda: grey_call(ys))
        print(json.dumps({"layout": f"nv12 siting={siting}", "pairs": B, "n": n, "refine": args.refine,
                          "oflk_interpolate_frames_nv12_ms": one, "y_planes_u8_call_ms": y_only,
                          "ratio_of_medians": round(one["median"] / y_only["median"], 3)}), flush=True)
    del frames, out, flows, status, out_y, grey
    torch.cuda.empty_cache()

    T = args.host_frames
    if T >= 2:
        g = video(T)
        host = {"grey": g.cpu().numpy(), "packed": colour(g, 3).cpu().numpy(), "nv12": nv12(g).cpu().numpy()}
        del g
        torch.cuda.empty_cache()
        cfg = _oflk.check_interp(0.01, 0.5, args.refine, [0.5])
        layouts = {"grey": _oflk.FrameLayout(), "packed": _oflk.FrameLayout("_packed", (3, 0)), "nv12": _oflk.FrameLayout("_nv12", (0,))}
        forms = [(k, lambda k=k: _oflk.interpolate_sequence_host(layouts[k], host[k], H, W, 3, 5, 3, cfg)) for k in host]
        wall = {k: [] for k in host}
        for _, f in forms:   # warm-up: plans, device buffers, the pages of the host arrays
            f()
        for k in range(max(1, args.host_steps)):
            for name, f in forms[k % 3:] + forms[:k % 3]:
                t0 = time.perf_counter()
                f()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"host": "1080p", "frames": T, "n": 1, "refine": args.refine,
                          "oflk_interpolate_sequence_u8_ms": [round(x, 1) for x in sorted(wall["grey"])],
                          "oflk_interpolate_sequence_packed_ms": [round(x, 1) for x in sorted(wall["packed"])],
                          "oflk_interpolate_sequence_nv12_ms": [round(x, 1) for x in sorted(wall["nv12"])]}), flush=True)


if __name__ == "__main__":
    main()
