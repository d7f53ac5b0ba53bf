#!/usr/bin/env python3
"""Sparse against dense point tracks on one workload: frames in, tracks out, host to host (development tool, not part of
the bench contract).

Host arrays, seeded content: T uint8 frames of 1080p (tools/track_bench.py's scene: a synthetic texture drifting by one row
and two columns per frame, with seeded noise), 3/5/3.  Queries: Shi-Tomasi corners of frame 0 (good_features_to_track),
about 1 000 and about 10 000 of them.  For each query set, alternating which goes first:
  (a) oflk_pyramidal_sequence_tracks_u8         dense: both flows of every pair, then the track kernel
  (b) oflk_pyramidal_sequence_sparse_tracks_u8  sparse: pyramids, then one wave per point
One JSON line per query set: ms per call (median, min, max over the steps), the share of tracks alive on the last frame for
both, how far the two trackers' common survivors are apart, and the peak device memory of a chunk of each call (the cached
plan's workspace as oflk_plan_workspace_bytes reports it for a plan of the chunk's size after one pass of that kind, plus
the call's own frame, flow and row buffers, computed from the shapes).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats` (--only sparse keeps the trace short).

--replenish times the replenished KLT instead, on the same frames: K = max_corners in (1 000, 10 000) and detect_every in
(1, 4, 16), alternating which goes first:
  (a) oflk_pyramidal_sequence_klt_replenish_u8         dense flows, track kernel, detections
  (b) oflk_pyramidal_sequence_klt_sparse_replenish_u8  pyramids, one sparse track launch per segment, detections
One JSON line per (K, detect_every): ms per call (median, min, max), the points detected and the share of slots alive on the
last frame for both.  --only sparse under rocprofv3 gives the split into pyramid, track and detection kernels.

--online times the online tracker on the same frames and (K, detect_every) grid, alternating which goes first:
  (a) oflk_pyramidal_sequence_klt_sparse_replenish_u8  one call on the T host frames
  (b) oflk_tracker_push                                T synchronous host pushes on one tracker (reset before each round)
and, from events around single calls on the T frames already on the device, the device time of a non-detecting and of a
detecting oflk_tracker_push_device in the steady state (frames 8 .. T-1; the JSON line gives each median's sample count, and
with detect_every 1 there is no non-detecting push).  One JSON line per (K, detect_every); it also checks that the pushes' rows
are the call's.

    python tools/sparse_bench.py [--frames 129] [--steps 5] [--warmup 1] [--only sparse|dense] [--replenish | --online]
                                 [--budgets 1000,10000] [--every 1,4,16]
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


def plan_bytes(C, H, W, sparse):
    """workspace of a plan of C pairs after one sparse pass (sparse) or one bidirectional dense pass"""
    import torch

    import _oflk

    dev = torch.device("cuda", 0)
    frames = torch.zeros((C + 1, H, W), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    plan = _oflk.Plan(0, C, H, W, 3, 5, 3)
    try:
        if sparse:
            q = torch.zeros((1, 2), dtype=torch.float32, device=dev)
            tr = torch.empty((C + 1, 1, 2), dtype=torch.float32, device=dev)
            vis = torch.empty((C + 1, 1), dtype=torch.uint8, device=dev)
            _oflk.sparse_tracks(plan, frames.data_ptr(), q.data_ptr(), 1, tr.data_ptr(), vis.data_ptr(), u8=True, stream=st)
        else:
            d = [torch.empty((C, H, W), dtype=torch.float32, device=dev) for _ in range(4)]
            plan.pyramidal_sequence_fb(frames.data_ptr(), *(t.data_ptr() for t in d), st, u8=True)
        torch.cuda.synchronize()
        return plan.workspace_bytes
    finally:
        plan.close()


def replenish_leg(args, frames, forms, steps):
    """the replenished KLT, dense against sparse, host to host"""
    import numpy as np

    import _oflk

    L = _oflk.lib()
    T, H, W = frames.shape
    for K, md in zip(args.budgets, (10.0, 4.0) if len(args.budgets) == 2 else [4.0] * len(args.budgets)):
        for D in args.every:
            out = {f: (np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8), np.empty((T, K), np.uint8), np.empty(T, np.int32))
                   for f in forms}
            res = np.empty((T, K), np.float32)

            def call(form):
                tr, vis, born, det = out[form]
                if form == "dense":
                    _oflk.check(L.oflk_pyramidal_sequence_klt_replenish_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 0.01, md, K,
                                                                           D, _oflk.ptr(tr), vis.ctypes.data, born.ctypes.data,
                                                                           det.ctypes.data_as(_oflk._i32p)))
                else:
                    _oflk.check(L.oflk_pyramidal_sequence_klt_sparse_replenish_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 4.0,
                                                                                  0.01, md, K, D, _oflk.ptr(tr), vis.ctypes.data,
                                                                                  born.ctypes.data, det.ctypes.data_as(_oflk._i32p),
                                                                                  _oflk.ptr(res)))

            for _ in range(args.warmup):
                for f in forms:
                    call(f)
            ms = {f: [] for f in forms}
            for i in range(steps):
                for f in (forms if i % 2 == 0 else forms[::-1]):
                    t0 = time.perf_counter()
                    call(f)
                    ms[f].append((time.perf_counter() - t0) * 1e3)
            line = {"tool": "sparse_bench", "leg": "replenish", "pixels": "u8", "frames": T, "height": H, "width": W, "levels": 3,
                    "window": 5, "iters": 3, "steps": steps, "K": K, "min_distance": md, "detect_every": D}
            for f in forms:
                line[f"{f}_ms"] = round(statistics.median(ms[f]), 3)
                line[f"{f}_ms_min_max"] = [round(min(ms[f]), 3), round(max(ms[f]), 3)]
                line[f"{f}_detected"] = int(out[f][3].sum())
                line[f"{f}_alive_last"] = round(float(out[f][1][-1].mean()), 4)
            if len(forms) == 2:
                line["speedup"] = round(line["dense_ms"] / line["sparse_ms"], 3)
            print(json.dumps(line), flush=True)


def online_leg(args, frames, steps):
    """the online tracker against the sequence call, host to host, and the device time of single pushes"""
    import numpy as np
    import torch

    import _oflk

    L = _oflk.lib()
    T, H, W = frames.shape
    d_frames = torch.from_numpy(frames).to("cuda:0")   # every frame: each device median below states its count
    st = torch.cuda.current_stream().cuda_stream
    for K, md in zip(args.budgets, (10.0, 4.0) if len(args.budgets) == 2 else [4.0] * len(args.budgets)):
        for D in args.every:
            tr, vis, born = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8), np.empty((T, K), np.uint8)
            det, res = np.empty(T, np.int32), np.empty((T, K), np.float32)
            ptr, pvis, pborn = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8), np.empty((T, K), np.uint8)
            pdet, pres, birth = np.empty(T, np.int32), np.empty((T, K), np.float32), np.empty(K, np.int32)
            tk = _oflk.Tracker(0, H, W, True, K, D, 3, 5, 3, 0.01, 0.5, 4.0, 0.01, md)

            def call(form):
                if form == "sequence":
                    _oflk.check(L.oflk_pyramidal_sequence_klt_sparse_replenish_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 4.0,
                                                                                  0.01, md, K, D, _oflk.ptr(tr), vis.ctypes.data,
                                                                                  born.ctypes.data, det.ctypes.data_as(_oflk._i32p),
                                                                                  _oflk.ptr(res)))
                    return
                tk.reset()
                for t in range(T):
                    _oflk.check(L.oflk_tracker_push(tk._h, frames[t].ctypes.data, _oflk.ptr(ptr[t]), pvis[t].ctypes.data,
                                                    pborn[t].ctypes.data, birth.ctypes.data_as(_oflk._i32p), _oflk.ptr(pres[t]),
                                                    pdet[t:].ctypes.data_as(_oflk._i32p)))

            forms = ["sequence", "pushes"]
            try:
                for _ in range(args.warmup):
                    for f in forms:
                        call(f)
                ms = {f: [] for f in forms}
                for i in range(steps):
                    for f in (forms if i % 2 == 0 else forms[::-1]):
                        t0 = time.perf_counter()
                        call(f)
                        ms[f].append((time.perf_counter() - t0) * 1e3)
                same = all(np.array_equal(a[:T - 1], b[:T - 1], equal_nan=a.dtype == np.float32)
                           for a, b in ((ptr, tr), (pvis, vis), (pborn, born), (pdet, det), (pres, res)))
                # device time of single pushes in the steady state: events around one push_device each
                tk.reset()
                dev_ms = {"detecting": [], "plain": []}
                for t in range(d_frames.shape[0]):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    tk.push_device(d_frames[t].data_ptr(), st)
                    b.record()
                    b.synchronize()
                    if t >= 8:   # past frame 0's detection, where every slot is free
                        dev_ms["detecting" if D > 0 and t % D == 0 else "plain"].append(a.elapsed_time(b))
            finally:
                tk.close()
            line = {"tool": "sparse_bench", "leg": "online", "pixels": "u8", "frames": T, "height": H, "width": W, "levels": 3,
                    "window": 5, "iters": 3, "steps": steps, "K": K, "min_distance": md, "detect_every": D,
                    "rows_equal_the_call": bool(same)}
            for f in forms:
                line[f"{f}_ms"] = round(statistics.median(ms[f]), 3)
                line[f"{f}_ms_min_max"] = [round(min(ms[f]), 3), round(max(ms[f]), 3)]
            line["pushes_over_sequence"] = round(line["pushes_ms"] / line["sequence_ms"], 3)
            line["push_ms_per_frame"] = round(line["pushes_ms"] / T, 4)
            for k, v in dev_ms.items():
                line[f"push_device_{k}_ms"] = round(statistics.median(v), 4) if v else None
                line[f"push_device_{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)] if v else None
                line[f"push_device_{k}_samples"] = len(v)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=5, help="timed calls of each form (at most 20)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", choices=["sparse", "dense"], default=None)
    ap.add_argument("--replenish", action="store_true", help="time the replenished KLT calls instead of the plain tracks")
    ap.add_argument("--online", action="store_true", help="time the online tracker's pushes against the replenished sparse call")
    ap.add_argument("--budgets", type=lambda v: [int(x) for x in v.split(",")], default=[1000, 10000], help="--replenish: max_corners")
    ap.add_argument("--every", type=lambda v: [int(x) for x in v.split(",")], default=[1, 4, 16], help="--replenish: detect_every")
    args = ap.parse_args()
    steps = max(1, min(args.steps, 20))
    import numpy as np
    import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

    import _oflk
    import lucas_kanade_core as C
    from oflk_synth import synth_pair

    T, H, W = args.frames, args.height, args.width
    B = T - 1
    base = synth_pair(H, W, pair_index=args.seed)[0].astype(np.float32)
    rng = np.random.default_rng(args.seed)
    frames = np.empty((T, H, W), np.uint8)
    for t in range(T):
        f = np.roll(base, (t, 2 * t), axis=(0, 1)) + rng.normal(0.0, 1.5, (H, W)).astype(np.float32)
        frames[t] = np.rint(np.clip(f, 0.0, 255.0)).astype(np.uint8)
    L = _oflk.lib()
    forms = [f for f in ("dense", "sparse") if args.only in (None, f)]
    if args.online:
        online_leg(args, frames, steps)
        return
    if args.replenish:
        replenish_leg(args, frames, forms, steps)
        return
    # chunk sizes of the two host calls at this frame size (chunk_pairs / sparse_chunk_pairs in oflk.hip)
    c_dense = max(1, (32 << 20) // (H * W * 4))
    c_dense = c_dense if B >= 4 * c_dense and B * H * W * 4 >= (64 << 20) else B
    c_sparse = min(B, 64, max(1, (128 << 20) // (H * W * 4)))
    ws = {"dense": plan_bytes(c_dense, H, W, False), "sparse": plan_bytes(c_sparse, H, W, True)}

    for want, md in ((1000, 10.0), (10000, 4.0)):
        xy, _ = C.good_features_to_track(frames[0], want, 0.01, md, 5)
        q = np.ascontiguousarray(xy, np.float32)
        N = len(q)
        out = {f: (np.empty((T, N, 2), np.float32), np.empty((T, N), np.uint8)) for f in forms}

        def call(form):
            tr, vis = out[form]
            if form == "dense":
                _oflk.check(L.oflk_pyramidal_sequence_tracks_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, None, _oflk.ptr(q), N,
                                                                _oflk.ptr(tr), vis.ctypes.data))
            else:
                _oflk.check(L.oflk_pyramidal_sequence_sparse_tracks_u8(frames.ctypes.data, T, H, W, 3, 5, 3, 0.01, 0.5, 4.0, None,
                                                                       _oflk.ptr(q), N, _oflk.ptr(tr), vis.ctypes.data))

        for _ in range(args.warmup):
            for f in forms:
                call(f)
        ms = {f: [] for f in forms}
        for i in range(steps):
            for f in (forms if i % 2 == 0 else forms[::-1]):
                t0 = time.perf_counter()
                call(f)
                ms[f].append((time.perf_counter() - t0) * 1e3)
        line = {"tool": "sparse_bench", "pixels": "u8", "frames": T, "pairs": B, "height": H, "width": W, "levels": 3, "window": 5,
                "iters": 3, "steps": steps, "N": N, "min_distance": md}
        rows = 9 * N   # a row: float2 + uint8 per query
        call_bytes = {"dense": (c_dense + 1) * H * W + 4 * c_dense * H * W * 4 + (c_dense + 1) * rows,
                      "sparse": (c_sparse + 1) * H * W + (c_sparse + 1) * rows}
        for f in forms:
            line[f"{f}_ms"] = round(statistics.median(ms[f]), 3)
            line[f"{f}_ms_min_max"] = [round(min(ms[f]), 3), round(max(ms[f]), 3)]
            line[f"{f}_alive_last"] = round(float(out[f][1][-1].mean()), 4)
            line[f"{f}_chunk_pairs"] = {"dense": c_dense, "sparse": c_sparse}[f]
            line[f"{f}_plan_workspace_MB"] = round(ws[f] / 2 ** 20, 1)
            line[f"{f}_peak_device_MB"] = round((ws[f] + call_bytes[f]) / 2 ** 20, 1)
        if len(forms) == 2:
            line["speedup"] = round(line["dense_ms"] / line["sparse_ms"], 3)
            both = (out["dense"][1][-1] & out["sparse"][1][-1]).astype(bool)
            d = np.abs(out["dense"][0][-1][both] - out["sparse"][0][-1][both]).max(1)
            line["common_survivors"] = int(both.sum())
            line["apart_px_median_max"] = [round(float(np.median(d)), 3), round(float(d.max()), 3)] if both.any() else None
            # the scene's ground truth: (2, 1) px per frame, wrapped: compare where the point has not wrapped
            truth = q + np.float32(B) * np.asarray([2.0, 1.0], np.float32)
            for f in forms:
                v = out[f][1][-1].astype(bool)
                e = np.abs(out[f][0][-1][v] - truth[v]).max(1) if v.any() else np.zeros(0)
                line[f"{f}_error_px_median"] = round(float(np.median(e)), 3) if e.size else None
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
