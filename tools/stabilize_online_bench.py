#!/usr/bin/env python3
"""Device time of the online stabiliser's trajectory kernel and of its push (development tool, not part of the bench contract).

Leg 1, the trajectory of one frame (default): oflk_stabilize_trajectory_ring (k_stab_online, n = 1, an open stream) at r = 15
and r = 64 on a full ring, against oflk_stabilize_trajectory (k_stab_trajectory) launched with T = 2 r + 1, whose centre
thread runs the same window as one serial chain.  The two take turns; a pair of events around every single launch, the median
of `--launches` launches, and next to it the time per launch of `--launches` launches enqueued back to back.  One JSON line
per radius.

Leg 2 (--push): oflk_stabilizer_push_device in steady state at 1080p uint8, K = 1000, D = 4, r = 15, similarity, against
oflk_tracker_push_device with motion on at the same shape, the two taking turns: events around `--pushes` pushes (a multiple
of D, so each window holds the same number of detections), the median over `--steps` windows.  Then, separately, what the
stabiliser adds to a push: one device-to-device copy of a frame, one oflk_warp_affine of one frame and one k_stab_online
launch at r = 15, each as events around `--pushes` back-to-back calls.  One JSON line.

    python tools/stabilize_online_bench.py [--launches 200] [--push] [--steps 9] [--pushes 32]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


def _timed(fn, reps):
    """microseconds per call of `reps` back-to-back calls, by events on the current stream"""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernel_leg(args):
    import numpy as np
    import torch

    import _oflk
    import motion_model as MM
    import stabilize_model as SM

    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    for r in (15, 64):
        w = _oflk.stabilize_weights(r)
        T, cap = 2 * r + 1, 2 * r
        model = SM.noisy_models(T - 1, MM.SIMILARITY, r)
        counts = np.tile(np.int32([30, 40, 1]), (T - 1, 1))
        t_model, t_counts = torch.from_numpy(model).to(d), torch.from_numpy(counts).to(d)
        corr_a, map_a = torch.zeros((T, 6), device=d), torch.zeros((T, 6), dtype=torch.float64, device=d)
        corr_b, map_b = torch.zeros((1, 6), device=d), torch.zeros((1, 6), dtype=torch.float64, device=d)

        def serial():
            _oflk.stabilize_trajectory(t_model.data_ptr(), t_counts.data_ptr(), T, w, corr_a.data_ptr(), map_a.data_ptr(), 0, st)

        def ring():   # frame r of the same steps: step s sits at slot s % cap = s
            _oflk.stabilize_trajectory_ring(t_model.data_ptr(), t_counts.data_ptr(), cap, r, 1, -1, w, corr_b.data_ptr(),
                                            map_b.data_ptr(), st)

        for fn in (serial, ring):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        same = bool((corr_a[r].view(torch.int32) == corr_b[0].view(torch.int32)).all() and
                    (map_a[r].view(torch.int64) == map_b[0].view(torch.int64)).all())
        single = {"serial": [], "ring": []}
        for i in range(args.launches):
            for k, fn in ((("serial", serial), ("ring", ring)) if i % 2 == 0 else (("ring", ring), ("serial", serial))):
                single[k].append(_timed(fn, 1))
        batch = {"serial": [], "ring": []}
        for i in range(7):
            for k, fn in ((("serial", serial), ("ring", ring)) if i % 2 == 0 else (("ring", ring), ("serial", serial))):
                batch[k].append(_timed(fn, args.launches))
        q = lambda v: [round(x, 2) for x in statistics.quantiles(v, n=4)]   # noqa: E731
        print(json.dumps({"tool": "stabilize_online_bench", "leg": "trajectory", "radius": r, "launches": args.launches,
                          "same_bits": same,
                          "k_stab_online_us_median": round(statistics.median(single["ring"]), 2),
                          "k_stab_trajectory_us_median": round(statistics.median(single["serial"]), 2),
                          "k_stab_online_us_quartiles": q(single["ring"]), "k_stab_trajectory_us_quartiles": q(single["serial"]),
                          "k_stab_online_us_back_to_back": round(statistics.median(batch["ring"]), 2),
                          "k_stab_trajectory_us_back_to_back": round(statistics.median(batch["serial"]), 2),
                          "back_to_back_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in batch.items()}}), flush=True)


def push_leg(args):
    import numpy as np
    import torch

    import _oflk
    from stabilize_bench import scene

    H, W, K, D, r, hyps = 1080, 1920, 1000, 4, 15, 256
    assert args.pushes % D == 0
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    N = 32
    frames = torch.from_numpy(scene(N, H, W)).to(d)
    out = torch.empty((H, W), dtype=torch.uint8, device=d)
    w = _oflk.stabilize_weights(r)
    stab = _oflk.Stabilizer(0, H, W, True, K, D, 1, w, hyps, 1.0, 0)
    trk = _oflk.Tracker(0, H, W, True, K, D)
    trk.set_motion(1, hyps, 1.0, 0)
    n = {"stab": 0, "trk": 0}

    def push_stab():
        stab.push_device(frames[n["stab"] % N].data_ptr(), out.data_ptr(), 0, st)
        n["stab"] += 1

    def push_trk():
        trk.push_device(frames[n["trk"] % N].data_ptr(), st)
        n["trk"] += 1

    for _ in range(2 * N):   # steady state: the delay line and the ring are full, every push emits
        push_stab()
        push_trk()
    torch.cuda.synchronize()
    us = {"stab": [], "trk": []}
    for step in range(args.steps):
        for k, fn in ((("stab", push_stab), ("trk", push_trk)) if step % 2 == 0 else (("trk", push_trk), ("stab", push_stab))):
            us[k].append(_timed(fn, args.pushes))
    # the parts, with the parent's entry points
    th = np.deg2rad(0.5)
    t_map = torch.from_numpy(np.float64([[np.cos(th), -np.sin(th), 3.5, np.sin(th), np.cos(th), -2.25]])).to(d)
    slot = torch.empty((H, W), dtype=torch.uint8, device=d)
    ring_model = torch.from_numpy(np.tile(np.float32([1, 0, 1.5, 0, 1, -0.5]), (2 * r, 1))).to(d)
    ring_counts = torch.ones((2 * r, 3), dtype=torch.int32, device=d)
    corr, mp = torch.zeros((1, 6), device=d), torch.zeros((1, 6), dtype=torch.float64, device=d)
    parts = {"copy": lambda: slot.copy_(frames[3]),
             "warp": lambda: _oflk.warp_affine(frames[3].data_ptr(), 1, H, W, t_map.data_ptr(), out.data_ptr(), 0, True, st),
             "ring": lambda: _oflk.stabilize_trajectory_ring(ring_model.data_ptr(), ring_counts.data_ptr(), 2 * r, 100, 1, -1, w,
                                                             corr.data_ptr(), mp.data_ptr(), st)}
    pus = {k: [] for k in parts}
    for fn in parts.values():
        fn()
    torch.cuda.synchronize()
    for step in range(args.steps):
        for k, fn in parts.items():
            pus[k].append(_timed(fn, args.pushes))
    med = {k: statistics.median(v) for k, v in {**us, **pus}.items()}
    print(json.dumps({"tool": "stabilize_online_bench", "leg": "push", "H": H, "W": W, "pixels": "uint8", "K": K, "detect_every": D,
                      "radius": r, "model": "similarity", "hypotheses": hyps, "pushes_per_window": args.pushes, "steps": args.steps,
                      "stabilizer_push_us": round(med["stab"], 1), "tracker_push_us": round(med["trk"], 1),
                      "added_us": round(med["stab"] - med["trk"], 1),
                      "frame_copy_us": round(med["copy"], 1), "warp_one_frame_us": round(med["warp"], 1),
                      "k_stab_online_us": round(med["ring"], 1), "parts_sum_us": round(med["copy"] + med["warp"] + med["ring"], 1),
                      "min_max_us": {k: [round(min(v), 1), round(max(v), 1)] for k, v in {**us, **pus}.items()},
                      "stabilizer_workspace_MB": round(stab.workspace_bytes / 1e6, 1),
                      "tracker_workspace_MB": round(trk.workspace_bytes / 1e6, 1)}), flush=True)
    stab.close()
    trk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--push", action="store_true", help="time the push in steady state instead")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--pushes", type=int, default=32)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

    if args.push:
        push_leg(args)
    else:
        kernel_leg(args)


if __name__ == "__main__":
    main()
