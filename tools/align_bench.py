#!/usr/bin/env python3
"""Device time of direct image alignment (development tool, not part of the bench contract).

Legs, each in a process of its own under its own time limit (a leg that fails or runs out of time ends the run), one JSON line
each with the median and min - max over `--steps` windows of `--reps` back-to-back calls between two events:
  iteration   oflk_align_refine on S = 128 steps of 1080p, one level, with n = 2 and with n = 6 iterations: the difference over
              four is one iteration (k_align_reduce over the S frames and k_align_update), without the pyramid and the two
              residual passes.  uint8 and float32 frames, affine and homography.  Every step starts half a pixel from the
              truth, so that every iteration is accepted and none freezes
  copy        a device copy of the bytes an iteration must read (the S templates and the S images), uint8 and float32
  warp        oflk_warp_perspective of the same S images under the same maps: the nearest existing kernel
  photometric the same measurement of oflk_align_refine_photo (the kernels' PHOTO instantiations) and of the plain call
              in one process on the same steps, and their ratio.  uint8 and float32 frames, affine and homography
  robust      the same measurement of the four forms in one process on the same steps: plain, photometric, robust
              (oflk_align_refine_robust, the kernels' ROBUST instantiations, --delta grey levels) and robust +
              photometric, and the ratios of the robust forms over their bases.  uint8 and float32 frames, affine and homography
  accumulate  oflk_mosaic_accumulate and oflk_mosaic_accumulate_exposure of 32 frames of 1080p, 8 px apart, onto one canvas, mean
              and feather blends, uint8 and float32 frames, and their ratio
  sequence    the whole oflk_align_sequence (pyramids, L = 3, n = 5, both residual passes) on T = 129 resident uint8 frames,
              and oflk_tracks_homography on T rows of K = 1000 tracks with 256 hypotheses: the fit it refines
  chain       lucas_kanade_pyramidal_sequence_mosaic (host frames in, picture out) on 16 frames of 120 x 160 with
              refine_iterations = 0 and 5: the price of the refinement in the chain it joins, and the mean absolute difference
              between the mosaic and the image the frames were cut from (the scene of tests/test_gpu_mosaic.py's pan)

    python tools/align_bench.py [--steps 5] [--reps 2] [--S 128] [--limit 240] [--delta 4.0]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))

H, W = 1080, 1920
KINDS = {"affine": 0, "homography": 1}


def windows(run, steps, reps):
    import torch

    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), [round(min(ms), 3), round(max(ms), 3)]


def textured(n, dtype, device):
    """n frames of one smooth texture, frame f shifted by f pixels: (n, H, W) on the device"""
    import torch

    g = torch.Generator(device=device).manual_seed(0)
    t = torch.rand((1, 1, H + 16, W + n + 16), generator=g, device=device)
    k = torch.ones((1, 1, 9, 9), device=device) / 81.0
    t = torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, k), k)[0, 0]
    t = 255.0 * (t - t.min()) / (t.max() - t.min())
    frames = torch.stack([t[:H, f:f + W] for f in range(n)])
    return frames.round().to(torch.uint8).contiguous() if dtype == "u8" else frames.float().contiguous()


def leg(args):
    import numpy as np
    import torch

    import _oflk

    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    S, u8 = args.S, args.dtype == "u8"
    out = {"tool": "align_bench", "leg": args.leg, "S": S, "H": H, "W": W, "reps": args.reps, "steps": args.steps}
    if args.leg == "chain":
        sys.path.insert(0, str(ROOT / "tests"))
        import lucas_kanade_pyramidal as P
        import mosaic_model as M

        T, h, w, step = 16, 120, 160, 6
        image = M.smooth_field(h + 8, w + step * (T - 1) + 8, 17)
        frames, _ = M.pan_frames(image, T, h, w, step, 0, 4, 4)
        for n in (0, 5):
            P.lucas_kanade_pyramidal_sequence_mosaic(frames, max_corners=500, refine_iterations=n)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                got = P.lucas_kanade_pyramidal_sequence_mosaic(frames, max_corners=500, refine_iterations=n)
            ms = (time.perf_counter() - t0) * 1e3 / args.reps
            Hc, Wc = got.canvas.shape
            x0, y0 = got.origin
            ys, xs = np.arange(Hc) + y0 + 4, np.arange(Wc) + x0 + 4
            oy, ox = (ys >= 0) & (ys < image.shape[0]), (xs >= 0) & (xs < image.shape[1])
            src, known = np.zeros((Hc, Wc)), np.zeros((Hc, Wc), bool)
            src[np.ix_(oy, ox)] = image[np.ix_(ys[oy], xs[ox])]
            known[np.ix_(oy, ox)] = True
            core = (got.count > 0) & known
            cover = core.copy()
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    core &= np.roll(np.roll(cover, dy, 0), dx, 1)
            core[:2], core[-2:], core[:, :2], core[:, -2:] = False, False, False, False
            mad = float(np.abs(got.canvas.astype(np.float64) - src)[core].mean())
            print(json.dumps({**out, "S": T - 1, "H": h, "W": w, "refine_iterations": n, "host_ms": round(ms, 2),
                              "canvas": [Wc, Hc], "pixels": int(core.sum()), "mean_abs_difference": round(mad, 4)}), flush=True)
        return
    if args.leg == "sequence":
        T, code = S + 1, KINDS["homography"]
        frames = textured(T, "u8", d)
        model = torch.tensor([1, 0, -0.5, 0, 1, 0.3, 0, 0, 1], dtype=torch.float32, device=d).repeat(S, 1).contiguous()
        nbytes = _oflk.align_workspace(S, H, W, 3, code)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
        mo, so, ss = torch.empty_like(model), torch.empty(S, dtype=torch.int32, device=d), torch.empty((S, 4), dtype=torch.float64, device=d)
        med, mm = windows(lambda: _oflk.align_sequence(frames.data_ptr(), T, H, W, 3, 5, code, 0.25, model.data_ptr(), 0, ws.data_ptr(),
                                                       nbytes, mo.data_ptr(), so.data_ptr(), ss.data_ptr(), True, st), args.steps, args.reps)
        print(json.dumps({**out, "what": "oflk_align_sequence L=3 n=5 u8", "ms": round(med, 3), "ms_min_max": mm,
                          "ms_per_step": round(med / S, 4), "status_1": int((so == 1).sum().item()),
                          "workspace_MiB": round(nbytes / 2 ** 20, 1)}), flush=True)
        K, Hn = 1000, 256
        g = torch.Generator(device=d).manual_seed(1)
        row0 = torch.rand((K, 2), generator=g, device=d) * torch.tensor([W - 1.0, H - 1.0], device=d)
        tracks = torch.stack([row0 + torch.tensor([1.0 * t, 0.25 * t], device=d) for t in range(T)]).float().contiguous()
        vis = torch.ones((T, K), dtype=torch.uint8, device=d)
        wb = _oflk.homography_workspace(S, K, Hn)
        hws = torch.empty(wb, dtype=torch.uint8, device=d)
        hm, inl, cnt = torch.empty((S, 9), device=d), torch.empty((S, K), dtype=torch.uint8, device=d), torch.empty((S, 3), dtype=torch.int32, device=d)
        med, mm = windows(lambda: _oflk.tracks_homography(tracks.data_ptr(), vis.data_ptr(), 0, T, K, hws.data_ptr(), wb, hm.data_ptr(),
                                                          inl.data_ptr(), cnt.data_ptr(), Hn, 1.0, 0, 0, st), args.steps, args.reps)
        print(json.dumps({**out, "what": "oflk_tracks_homography K=1000 Hn=256", "ms": round(med, 3), "ms_min_max": mm,
                          "ms_per_step": round(med / S, 4)}), flush=True)
        return
    frames = textured(S + 1, args.dtype, d)
    a, b = frames[:-1], frames[1:]
    if args.leg == "copy":
        dst = torch.empty_like(frames)
        med, mm = windows(lambda: (dst[:-1].copy_(a), dst[1:].copy_(b)), args.steps, args.reps)
        nbytes = 2 * a.numel() * a.element_size()
        print(json.dumps({**out, "dtype": args.dtype, "ms": round(med, 3), "ms_min_max": mm, "bytes_read": nbytes,
                          "GB_per_s_read_plus_written": round(2 * nbytes / med / 1e6, 1)}), flush=True)
        return
    if args.leg == "warp":
        maps = torch.tensor([1, 0, -0.5, 0, 1, 0.3, 1e-7, -1e-7, 1], dtype=torch.float64, device=d).repeat(S, 1).contiguous()
        dst = torch.empty_like(b)
        med, mm = windows(lambda: _oflk.warp_perspective(b.data_ptr(), S, H, W, maps.data_ptr(), dst.data_ptr(), 0, u8, st),
                          args.steps, args.reps)
        print(json.dumps({**out, "dtype": args.dtype, "ms": round(med, 3), "ms_min_max": mm, "ns_per_pixel": round(med * 1e6 / (S * H * W), 4)}),
              flush=True)
        return
    if args.leg == "accumulate":
        F, dx = 32, 8
        Hc, Wc = H, W + dx * (F - 1)
        fr = frames[:F].contiguous()
        maps = torch.tensor([[1, 0, -dx * f, 0, 1, 0, 0, 0, 1] for f in range(F)], dtype=torch.float64, device=d).contiguous()
        expo = torch.tensor([[1.0 + 0.01 * f, -0.5 * f] for f in range(F)], dtype=torch.float64, device=d).contiguous()
        sb = _oflk.mosaic_state_bytes(Hc, Wc)
        state = torch.zeros(sb, dtype=torch.uint8, device=d)
        for blend in ("mean", "feather"):
            code = _oflk.MOSAIC_BLENDS[blend]
            res = {}
            for name, ex in (("plain", None), ("exposure", expo.data_ptr())):
                res[name] = windows(lambda: _oflk.mosaic_accumulate(fr.data_ptr(), F, H, W, maps.data_ptr(), 0, 0, 0, Hc, Wc, code,
                                                                    state.data_ptr(), sb, u8, st, ex), args.steps, args.reps)
            print(json.dumps({**out, "S": F, "dtype": args.dtype, "blend": blend, "canvas": [Wc, Hc], "ms_plain": round(res["plain"][0], 3),
                              "ms_min_max_plain": res["plain"][1], "ms_exposure": round(res["exposure"][0], 3),
                              "ms_min_max_exposure": res["exposure"][1], "ratio": round(res["exposure"][0] / res["plain"][0], 3)}), flush=True)
        return
    code = KINDS[args.kind]
    nc = 9 if code else 6
    m0 = [1, 0, -0.5, 0, 1, 0.3, 0, 0, 1][:nc]   # the truth is (-1, 0)
    model = torch.tensor(m0, dtype=torch.float32, device=d).repeat(S, 1).contiguous()
    mo, so, ss = torch.empty_like(model), torch.empty(S, dtype=torch.int32, device=d), torch.empty((S, 8), dtype=torch.float64, device=d)
    po = torch.empty((S, 2), dtype=torch.float32, device=d)

    def iteration(photo, delta=None):
        """(ms per iteration, the two windows' results) of the plain or the photometric call, or with delta of their robust forms"""
        nbytes = _oflk.align_workspace(S, H, W, 1, code, photo, robust=delta is not None)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
        res = {}
        for n in (2, 6):
            res[n] = windows(lambda: _oflk.align_refine(a.data_ptr(), b.data_ptr(), S, H, W, 1, n, code, 0.25, model.data_ptr(), 0, ws.data_ptr(),
                                                        nbytes, mo.data_ptr(), so.data_ptr(), ss.data_ptr(), u8, st,
                                                        po.data_ptr() if photo else None, delta), args.steps, args.reps)
            accepted = ss.view(-1)[:S * (8 if delta is not None else 4)].view(S, -1)[:, 3].cpu().numpy()
            assert (accepted == n).all(), f"not every iteration was accepted: {accepted}"
        return (res[6][0] - res[2][0]) / 4.0, res

    per, res = iteration(False)
    row = {**out, "dtype": args.dtype, "kind": args.kind, "ms_n2": round(res[2][0], 3), "ms_n6": round(res[6][0], 3),
           "ms_min_max_n2": res[2][1], "ms_min_max_n6": res[6][1], "ms_per_iteration": round(per, 3),
           "ns_per_pixel": round(per * 1e6 / (S * H * W), 4), "status_1": int((so == 1).sum().item())}
    if args.leg == "photometric":
        pper, pres = iteration(True)
        row.update({"photo_ms_n2": round(pres[2][0], 3), "photo_ms_n6": round(pres[6][0], 3), "photo_ms_min_max_n2": pres[2][1],
                    "photo_ms_min_max_n6": pres[6][1], "photo_ms_per_iteration": round(pper, 3),
                    "photo_ns_per_pixel": round(pper * 1e6 / (S * H * W), 4), "photo_status_1": int((so == 1).sum().item()),
                    "photo_over_plain": round(pper / per, 3)})
    if args.leg == "robust":
        pper, pres = iteration(True)
        rper, rres = iteration(False, args.delta)
        weight = float(ss[:, 7].mean().item())
        qper, qres = iteration(True, args.delta)
        for name, x, r in (("photo", pper, pres), ("robust", rper, rres), ("robust_photo", qper, qres)):
            row.update({f"{name}_ms_n2": round(r[2][0], 3), f"{name}_ms_n6": round(r[6][0], 3), f"{name}_ms_min_max_n2": r[2][1],
                        f"{name}_ms_min_max_n6": r[6][1], f"{name}_ms_per_iteration": round(x, 3),
                        f"{name}_ns_per_pixel": round(x * 1e6 / (S * H * W), 4)})
        row.update({"photo_over_plain": round(pper / per, 3), "robust_over_plain": round(rper / per, 3),
                    "robust_photo_over_photo": round(qper / pper, 3), "robust_delta": args.delta,
                    "robust_mean_weight": round(weight, 4)})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--S", type=int, default=128)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--leg", choices=["iteration", "photometric", "robust", "accumulate", "copy", "warp", "sequence", "chain"], help="run this one leg in this process")
    ap.add_argument("--dtype", choices=["u8", "f32"], default="u8")
    ap.add_argument("--kind", choices=sorted(KINDS), default="homography")
    ap.add_argument("--delta", type=float, default=4.0, help="robust_delta of the robust leg, grey levels")
    ap.add_argument("--only", help="comma-separated legs: run these alone")
    args = ap.parse_args()
    if args.leg:
        import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

        leg(args)
        return 0
    legs = [("iteration", dt, k) for dt in ("u8", "f32") for k in ("homography", "affine")]
    legs += [("photometric", dt, k) for dt in ("u8", "f32") for k in ("homography", "affine")]
    legs += [("robust", dt, k) for dt in ("u8", "f32") for k in ("homography", "affine")]
    legs += [("accumulate", dt, "homography") for dt in ("u8", "f32")]
    legs += [("copy", dt, "homography") for dt in ("u8", "f32")] + [("warp", dt, "homography") for dt in ("u8", "f32")]
    legs += [("sequence", "u8", "homography"), ("chain", "u8", "homography")]
    if args.only:
        legs = [x for x in legs if x[0] in args.only.split(",")]
    for lg, dt, kind in legs:
        cmd = [sys.executable, __file__, "--leg", lg, "--dtype", dt, "--kind", kind, "--steps", str(args.steps), "--reps", str(args.reps),
               "--S", str(args.S), "--delta", str(args.delta)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"tool": "align_bench", "leg": lg, "dtype": dt, "kind": kind, "error": f"no result within {args.limit} s"}), flush=True)
            return 1
        if rc != 0:   # nothing more is started on the device after a leg that failed
            print(json.dumps({"tool": "align_bench", "leg": lg, "dtype": dt, "kind": kind, "error": f"exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
