#!/usr/bin/env python3
"""Device time of the fused NV12 warp, host-to-host time of the NV12 sequence call and the NV12 stabiliser's push
(development tool, not part of the bench contract).  Every leg alternates its candidates in one process, device events (or a
wall clock around a synchronous call) around `--reps` back-to-back calls, and prints one JSON line with the median over
`--steps` batches and the spread.  Outputs are compared byte for byte before anything is timed.

Leg "warp" (default): F = 64 NV12 frames of 1080p under a 2 degree rotation (affine) and under a mild homography
(perspective).  Three candidates take turns:
    nv12            one oflk_warp_*_nv12 call on the frames: both planes, one launch
    planar          three oflk_warp_affine / oflk_warp_perspective u8 calls on planes split beforehand, Y at 1080p and U, V at
                    540p under the chroma map formed on the host: what a caller has without the fused kernel; the split, the
                    128 fill and the re-join are not counted
    packed          oflk_warp_*_packed on RGB frames of the same size, for scale: NV12 moves half the bytes
The fused call is accepted when its median is no slower than `planar`.

Leg "sequence" (--sequence): oflk_stabilize_sequence_nv12 host to host on `--frames` frames of 1080p against
oflk_stabilize_sequence_u8 on the Y planes and oflk_stabilize_sequence_packed on RGB frames.  Reported only.

Leg "push" (--push): oflk_stabilizer_push_device in steady state at 1080p, K = 1000, D = 4, r = 15, similarity, of a grey, a
packed RGB and an NV12 stabiliser taking turns: events around `--pushes` pushes (a multiple of D), the median over `--steps`
windows.

    python tools/nv12_bench.py [--steps 7] [--reps 5] [--sequence [--frames 129] | --push [--pushes 32]]
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
sys.path.insert(0, str(ROOT / "tools"))

CHROMA_GAINS = ((0.6, 60), (0.75, 20))
SITING = {0: (0.0, 0.5), 1: (0.5, 0.5)}


def nv12_scene(T, H, W):
    """stabilize_bench's grey scene as NV12 frames (T, 3H/2, W): Y is the scene, U and V its 2 x 2 subsampling under a gain and
    an offset each"""
    import numpy as np

    from stabilize_bench import scene

    grey = scene(T, H, W)
    out = np.empty((T, 3 * H // 2, W), np.uint8)
    out[:, :H] = grey
    uv = out[:, H:].reshape(T, H // 2, W // 2, 2)
    sub = grey[:, ::2, ::2].astype(np.float32)
    for c, (a, b) in enumerate(CHROMA_GAINS):
        uv[..., c] = np.rint(a * sub + b).astype(np.uint8)
    return out


def chroma_map(m, siting):
    """the statement's chroma map (tests/nv12_model.py) of one luma map, formed on the host in float64"""
    import numpy as np

    m = np.float64(m)
    sx, sy = (np.float64(v) for v in SITING[siting])
    c2, c5 = (m[0] * sx + m[1] * sy) + m[2], (m[3] * sx + m[4] * sy) + m[5]
    if m.size == 6:
        return np.array([m[0], m[1], 0.5 * (c2 - sx), m[3], m[4], 0.5 * (c5 - sy)])
    c8 = (m[6] * sx + m[7] * sy) + m[8]
    return np.array([m[0] - sx * m[6], m[1] - sx * m[7], 0.5 * (c2 - sx * c8), m[3] - sy * m[6], m[4] - sy * m[7],
                     0.5 * (c5 - sy * c8), 2.0 * m[6], 2.0 * m[7], c8])


def warp_leg(args):
    import numpy as np
    import torch

    import _oflk
    from colour_bench import colour_scene, summary, take_turns

    F, H, W, siting = 64, 1080, 1920, 0
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    th = np.deg2rad(2.0)
    c, s = np.cos(th), np.sin(th)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    rot = [c, -s, cx - (c * cx - s * cy) + 3.5, s, c, cy - (s * cx + c * cy) + 3.5]
    maps = {"affine": rot, "perspective": [1.01, 0.004, -6.0, -0.003, 0.995, 4.0, 4e-6, -3e-6, 1.0]}
    host = nv12_scene(F, H, W)
    nv12 = torch.from_numpy(host).to(d)
    uv = nv12[:, H:].reshape(F, H // 2, W // 2, 2)
    planes = [nv12[:, :H].contiguous(), uv[..., 0].contiguous(), uv[..., 1].contiguous()]
    out_nv12 = torch.empty_like(nv12)
    out_planes = [torch.empty_like(p) for p in planes]
    ins_planes = [torch.empty_like(p) for p in planes[1:]]
    rgb = torch.from_numpy(colour_scene(F, H, W, 3)).to(d)
    out_rgb = torch.empty_like(rgb)
    for kind, m in maps.items():
        t_map = torch.from_numpy(np.tile(np.float64(m), (F, 1))).to(d)
        t_mc = torch.from_numpy(np.tile(chroma_map(m, siting), (F, 1))).to(d)
        warp_nv12 = _oflk.warp_affine_nv12 if kind == "affine" else _oflk.warp_perspective_nv12
        warp_plane = _oflk.warp_affine if kind == "affine" else _oflk.warp_perspective
        warp_packed = _oflk.warp_affine_packed if kind == "affine" else _oflk.warp_perspective_packed

        def run_nv12():
            warp_nv12(nv12.data_ptr(), F, H, W, t_map.data_ptr(), out_nv12.data_ptr(), 0, siting, st)

        def run_planar(inside=False):
            warp_plane(planes[0].data_ptr(), F, H, W, t_map.data_ptr(), out_planes[0].data_ptr(), 0, True, st)
            for k in (1, 2):
                warp_plane(planes[k].data_ptr(), F, H // 2, W // 2, t_mc.data_ptr(), out_planes[k].data_ptr(),
                           ins_planes[k - 1].data_ptr() if inside else 0, True, st)

        def run_packed():
            warp_packed(rgb.data_ptr(), F, H, W, 3, t_map.data_ptr(), out_rgb.data_ptr(), 0, st)

        run_nv12()
        run_planar(inside=True)
        torch.cuda.synchronize()
        fill = torch.tensor(128, dtype=torch.uint8, device=d)
        ch = [torch.where(ins_planes[k] != 0, out_planes[k + 1], fill) for k in range(2)]
        joined = torch.cat([out_planes[0], torch.stack(ch, dim=-1).reshape(F, H // 2, W)], dim=1)
        same = bool(torch.equal(joined, out_nv12))
        us = take_turns({"nv12": run_nv12, "planar": run_planar, "packed": run_packed}, args.steps, args.reps, F)
        r = summary(us)
        print(json.dumps({"tool": "nv12_bench", "leg": "warp", "kind": kind, "F": F, "H": H, "W": W, "siting": "left",
                          "unit": "us per frame", **r,
                          "nv12_over_planar": round(r["nv12"]["median_us"] / r["planar"]["median_us"], 3),
                          "nv12_over_packed_rgb": round(r["nv12"]["median_us"] / r["packed"]["median_us"], 3),
                          "accepted": r["nv12"]["median_us"] <= r["planar"]["median_us"], "bytes_equal": same,
                          "reps": args.reps, "steps": args.steps}), flush=True)


def sequence_leg(args):
    import numpy as np

    import _oflk
    from colour_bench import colour_scene

    T, H, W, K, D = args.frames, 1080, 1920, 1000, 4
    frames = nv12_scene(T, H, W)
    grey = np.ascontiguousarray(frames[:, :H])
    rgb = colour_scene(T, H, W, 3)
    L = _oflk.lib()
    w = _oflk.stabilize_weights(15)
    out = {"nv12": np.empty_like(frames), "grey": np.empty_like(grey), "rgb": np.empty_like(rgb)}
    res = {k: (np.empty((T, 6), np.float32), np.empty((T - 1, 6), np.float32), np.empty((T - 1, 3), np.int32), np.empty(T - 1, np.uint8))
           for k in out}
    tail = (3, 5, 3, 0.01, 0.5, 4.0, 0.01, 10.0, K, D, 1, 256, 1.0, 0, _oflk._f64(w), 15)

    def outs(k):
        corr, model, counts, held = res[k]
        return (out[k].ctypes.data, _oflk.ptr(corr), _oflk.ptr(model), counts.ctypes.data_as(_oflk._i32p), held.ctypes.data)

    calls = {"nv12": lambda: _oflk.check(L.oflk_stabilize_sequence_nv12(frames.ctypes.data, T, H, W, 0, *tail, *outs("nv12"))),
             "grey": lambda: _oflk.check(L.oflk_stabilize_sequence_u8(grey.ctypes.data, T, H, W, *tail, *outs("grey"))),
             "rgb": lambda: _oflk.check(L.oflk_stabilize_sequence_packed(rgb.ctypes.data, T, H, W, 3, 0, *tail, *outs("rgb")))}
    for fn in calls.values():
        fn()
    same = all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(res["nv12"], res["grey"]))
    same = same and np.array_equal(out["nv12"][:, :H], out["grey"])
    names = list(calls)
    ms = {k: [] for k in names}
    for step in range(args.steps):
        for k in names[step % 3:] + names[:step % 3]:
            t0 = time.perf_counter()
            calls[k]()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"tool": "nv12_bench", "leg": "sequence", "frames": T, "H": H, "W": W, "K": K, "detect_every": D, "radius": 15,
                      "nv12_ms": round(med["nv12"], 1), "grey_ms": round(med["grey"], 1), "rgb_ms": round(med["rgb"], 1),
                      "added_over_grey_ms": round(med["nv12"] - med["grey"], 1),
                      "nv12_ms_per_frame": round(med["nv12"] / T, 3),
                      "min_max_ms": {k: [round(min(v), 1), round(max(v), 1)] for k, v in ms.items()}, "steps": args.steps,
                      "trajectory_and_y_equal_the_grey_call": bool(same), "fitted_steps": int(res["nv12"][2][:, 2].sum())}), flush=True)


def push_leg(args):
    import torch

    import _oflk
    from colour_bench import colour_scene
    from stabilize_online_bench import _timed

    H, W, K, D, r, hyps, N = 1080, 1920, 1000, 4, 15, 256, 32
    assert args.pushes % D == 0
    d = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    w = _oflk.stabilize_weights(r)
    frames = {"nv12": torch.from_numpy(nv12_scene(N, H, W)).to(d), "rgb": torch.from_numpy(colour_scene(N, H, W, 3)).to(d)}
    frames["grey"] = frames["nv12"][:, :H].contiguous()
    outs = {k: torch.empty_like(v[0]) for k, v in frames.items()}
    stabs = {"grey": _oflk.Stabilizer(0, H, W, True, K, D, 1, w, hyps, 1.0, 0),
             "rgb": _oflk.Stabilizer(0, H, W, True, K, D, 1, w, hyps, 1.0, 0, channels=3),
             "nv12": _oflk.Stabilizer(0, H, W, True, K, D, 1, w, hyps, 1.0, 0, nv12=True)}
    n = {k: 0 for k in stabs}

    def push(k):
        stabs[k].push_device(frames[k][n[k] % N].data_ptr(), outs[k].data_ptr(), 0, st)
        n[k] += 1

    for _ in range(2 * N):   # steady state: the delay lines and the rings are full, every push emits
        for k in stabs:
            push(k)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["nv12"][:H], outs["grey"]))
    names = list(stabs)
    us = {k: [] for k in names}
    for step in range(args.steps):
        for k in names[step % 3:] + names[:step % 3]:
            us[k].append(_timed(lambda: push(k), args.pushes))
    print(json.dumps({"tool": "nv12_bench", "leg": "push", "H": H, "W": W, "K": K, "detect_every": D, "radius": r,
                      "model": "similarity", "pushes_per_window": args.pushes, "steps": args.steps,
                      "push_us": {k: round(statistics.median(v), 1) for k, v in us.items()},
                      "min_max_us": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
                      "workspace_MB": {k: round(s.workspace_bytes / 1e6, 1) for k, s in stabs.items()},
                      "y_equals_the_grey_stabiliser": same}), flush=True)
    for s in stabs.values():
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--pushes", type=int, default=32)
    ap.add_argument("--sequence", action="store_true", help="time the sequence calls host to host instead")
    ap.add_argument("--push", action="store_true", help="time the online stabilisers' pushes instead")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: liboflk binds to the HIP runtime torch has loaded)

    if args.sequence:
        sequence_leg(args)
    elif args.push:
        push_leg(args)
    else:
        warp_leg(args)


if __name__ == "__main__":
    main()
