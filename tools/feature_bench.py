#!/usr/bin/env python3
"""Shi-Tomasi corners and detect-then-track (development tool, not part of the bench contract).

Seeded content: 1080p frames of the synthetic scene with noise (as tools/track_bench.py).  Device times are torch events
around device-form calls on one stream (median of --steps after --warmup); host times are host to host.
  (a) score + candidate kernels of a batch of --batch frames: oflk_good_features with q = 1 (no pixel passes S > M, so
      the select kernel returns at once), and oflk_corner_score alone.  Reported as us and as the fraction of 8 TB/s on
      the algorithmic bytes (frame in, S out, S in again: 12 B/px float32, 9 B/px uint8; score alone 8 / 5 B/px).
  (b) the select kernel: oflk_good_features at md = 10, q = 0.01, for K = 1 000 and 10 000, minus (a): ms per batch and
      per frame (the frames of a batch run concurrently, one workgroup each).
  (c) oflk_pyramidal_sequence_klt against oflk_pyramidal_sequence_tracks on the points it detected, host to host,
      --frames frames (3/5/3), K = 10 000; both results are compared byte for byte.
With --replenish it measures the replenished KLT instead (K = 10 000, md 10, q 0.01):
  (d) one oflk_replenish_features call by torch events: on frame 0 with every slot free and no seeds, and in the steady
      state -- frame 1, the slots of frame 0's detection alive at its points but every tenth, which is free;
  (e) oflk_pyramidal_sequence_klt_replenish for detect_every 4 and 16 against oflk_pyramidal_sequence_klt on the same
      frames, host to host, alternating which goes first.
It prints one JSON line per measurement.

    python tools/feature_bench.py [--batch 128] [--frames 129] [--steps 5] [--warmup 1] [--pixels f32,u8] [--replenish]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "optical-flow-fpga_amd" / "python"))

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=5, help="timed calls of each form (at most 20)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pixels", default="f32,u8")
    ap.add_argument("--skip-klt", action="store_true")
    ap.add_argument("--replenish", action="store_true", help="parts (d) and (e) only")
    args = ap.parse_args()
    steps = max(1, min(args.steps, 20))
    import numpy as np
    import torch

    import _oflk
    from oflk_synth import synth_pair

    F, T, H, W = args.batch, args.frames, args.height, args.width
    n = T if args.replenish else max(F, T)
    base = synth_pair(H, W, pair_index=0)[0].astype(np.float32)
    rng = np.random.default_rng(0)
    f32 = np.empty((n, H, W), np.float32)
    for t in range(n):
        f32[t] = np.clip(np.roll(base, (t, 2 * t), axis=(0, 1)) + rng.normal(0.0, 1.5, (H, W)).astype(np.float32), 0.0, 255.0)
    frames = {"f32": f32, "u8": np.rint(f32).astype(np.uint8)}
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    for pix in args.pixels.split(",") if args.replenish else ():
        u8 = pix == "u8"
        K, q, md = 10000, 0.01, 10.0
        # (d) one detection
        d_f = torch.from_numpy(frames[pix][:2]).to(dev)
        nbytes = _oflk.replenish_features_workspace(H, W, 5, md, K)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        xy = torch.full((K, 2), float("nan"), dtype=torch.float32, device=dev)
        vis = torch.zeros((K,), dtype=torch.uint8, device=dev)
        qt = torch.full((K,), -1, dtype=torch.int32, device=dev)
        qxy = torch.full((K, 2), float("nan"), dtype=torch.float32, device=dev)
        born = torch.empty((K,), dtype=torch.uint8, device=dev)
        det = torch.empty((1,), dtype=torch.int32, device=dev)

        def detect(f, t):
            _oflk.replenish_features(d_f[f].data_ptr(), H, W, t, xy.data_ptr(), vis.data_ptr(), ws.data_ptr(), nbytes,
                                     qt.data_ptr(), qxy.data_ptr(), born.data_ptr(), det.data_ptr(), K, q, md, 5, u8=u8,
                                     stream=st.cuda_stream)

        first_ms = timed(lambda: detect(0, 0))
        first_n = int(det.cpu()[0])
        xy.copy_(qxy)   # the steady state: frame 0's points alive, every tenth slot free
        vis.copy_(born)
        vis[::10] = 0
        free = int((vis == 0).sum().cpu())
        steady_ms = timed(lambda: detect(1, 1))
        print(json.dumps({"tool": "feature_bench", "part": "d", "pixels": pix, "height": H, "width": W, "K": K, "md": md, "q": q,
                          "steps": steps, "frame0_all_free_ms": round(first_ms, 3), "frame0_detected": first_n,
                          "steady_free_slots": free, "steady_ms": round(steady_ms, 3), "steady_detected": int(det.cpu()[0])}),
              flush=True)
        del d_f, ws
        torch.cuda.empty_cache()
        # (e) host to host
        fr = np.ascontiguousarray(frames[pix][:T])
        L = _oflk.lib()
        src = fr.ctypes.data if u8 else _oflk.ptr(fr)
        klt_fn = L.oflk_pyramidal_sequence_klt_u8 if u8 else L.oflk_pyramidal_sequence_klt
        rep_fn = L.oflk_pyramidal_sequence_klt_replenish_u8 if u8 else L.oflk_pyramidal_sequence_klt_replenish
        cnt = np.zeros(1, np.int32)
        kxy, ksc = np.empty((K, 2), np.float32), np.empty(K, np.float32)
        ktr, kvis = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
        rtr, rvis, rborn = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8), np.empty((T, K), np.uint8)
        rdet = np.empty(T, np.int32)

        def klt():
            _oflk.check(klt_fn(src, T, H, W, 3, 5, 3, 0.01, 0.5, q, md, K, cnt.ctypes.data_as(_oflk._i32p), _oflk.ptr(kxy),
                               _oflk.ptr(ksc), _oflk.ptr(ktr), kvis.ctypes.data))

        def rep(D):
            _oflk.check(rep_fn(src, T, H, W, 3, 5, 3, 0.01, 0.5, q, md, K, D, _oflk.ptr(rtr), rvis.ctypes.data, rborn.ctypes.data,
                               rdet.ctypes.data_as(_oflk._i32p)))

        for D in (4, 16):
            forms = (("klt", klt), ("replenish", lambda: rep(D)))
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            ms = {"klt": [], "replenish": []}
            for i in range(steps):
                for name, fn in (forms if i % 2 == 0 else forms[::-1]):
                    t0 = time.perf_counter()
                    fn()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            a, b = statistics.median(ms["replenish"]), statistics.median(ms["klt"])
            nd = len(range(0, T - 1, D))
            print(json.dumps({"tool": "feature_bench", "part": "e", "pixels": pix, "frames": T, "height": H, "width": W, "K": K,
                              "detect_every": D, "detections": nd, "steps": steps, "replenish_ms": round(a, 3),
                              "klt_ms": round(b, 3), "ratio": round(a / b, 3),
                              "ms_per_later_detection": round((a - b) / max(nd - 1, 1), 3),
                              "born_after_frame0": int(rdet[1:].sum()), "visible_last_klt": int(kvis[-1].sum()),
                              "visible_last_replenish": int(rvis[-1].sum())}), flush=True)
    for pix in () if args.replenish else args.pixels.split(","):
        u8 = pix == "u8"
        d_f = torch.from_numpy(frames[pix][:F]).to(dev)
        px = F * H * W
        in_b = 1 if u8 else 4
        d_s = torch.empty((F, H, W), dtype=torch.float32, device=dev)
        score_ms = timed(lambda: _oflk.corner_score(d_f.data_ptr(), F, H, W, d_s.data_ptr(), 5, u8=u8, stream=st.cuda_stream))
        outs = {}

        def gf(K, q):
            nbytes = _oflk.good_features_workspace(F, H, W, 5, 10.0, K)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            cnt = torch.empty((F,), dtype=torch.int32, device=dev)
            xy = torch.empty((F, K, 2), dtype=torch.float32, device=dev)
            sc = torch.empty((F, K), dtype=torch.float32, device=dev)
            ms = timed(lambda: _oflk.good_features(d_f.data_ptr(), F, H, W, ws.data_ptr(), nbytes, cnt.data_ptr(), xy.data_ptr(),
                                                   sc.data_ptr(), K, q, 10.0, 5, u8=u8, stream=st.cuda_stream))
            outs[(K, q)] = cnt.cpu().numpy()
            del ws
            return ms

        sc_ms = gf(1, 1.0)
        line = {"tool": "feature_bench", "part": "a", "pixels": pix, "frames": F, "height": H, "width": W, "window": 5,
                "score_us": round(score_ms * 1e3, 1), "score_frac_peak": round((in_b + 4) * px / (score_ms * 1e-3) / PEAK, 3),
                "score_cand_us": round(sc_ms * 1e3, 1),
                "score_cand_frac_peak": round((in_b + 8) * px / (sc_ms * 1e-3) / PEAK, 3)}
        print(json.dumps(line), flush=True)
        for K in (1000, 10000):
            ms = gf(K, 0.01)
            sel = ms - sc_ms
            print(json.dumps({"tool": "feature_bench", "part": "b", "pixels": pix, "frames": F, "K": K, "md": 10.0, "q": 0.01,
                              "good_features_ms": round(ms, 3), "select_ms_per_batch": round(sel, 3),
                              "select_us_per_frame_serial_equiv": round(sel * 1e3 / F, 2),
                              "min_count": int(outs[(K, 0.01)].min())}), flush=True)
        del d_f, d_s
        torch.cuda.empty_cache()
        if args.skip_klt:
            continue
        # (c) host to host
        fr = np.ascontiguousarray(frames[pix][:T])
        K = 10000
        L = _oflk.lib()
        src = fr.ctypes.data if u8 else _oflk.ptr(fr)
        klt_fn = L.oflk_pyramidal_sequence_klt_u8 if u8 else L.oflk_pyramidal_sequence_klt
        tr_fn = L.oflk_pyramidal_sequence_tracks_u8 if u8 else L.oflk_pyramidal_sequence_tracks
        cnt = np.zeros(1, np.int32)
        kxy, ksc = np.empty((K, 2), np.float32), np.empty(K, np.float32)
        ktr, kvis = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)
        ttr, tvis = np.empty((T, K, 2), np.float32), np.empty((T, K), np.uint8)

        def klt():
            _oflk.check(klt_fn(src, T, H, W, 3, 5, 3, 0.01, 0.5, 0.01, 10.0, K, cnt.ctypes.data_as(_oflk._i32p), _oflk.ptr(kxy),
                               _oflk.ptr(ksc), _oflk.ptr(ktr), kvis.ctypes.data))

        def tracks():
            _oflk.check(tr_fn(src, T, H, W, 3, 5, 3, 0.01, 0.5, None, _oflk.ptr(kxy), K, _oflk.ptr(ttr), tvis.ctypes.data))

        klt()
        for _ in range(args.warmup):
            tracks()
        ms = {"klt": [], "tracks": []}
        for i in range(steps):
            for name, fn in ((("klt", klt), ("tracks", tracks)) if i % 2 == 0 else (("tracks", tracks), ("klt", klt))):
                t0 = time.perf_counter()
                fn()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(ktr, ttr, equal_nan=True) and np.array_equal(kvis, tvis))
        a, b = statistics.median(ms["klt"]), statistics.median(ms["tracks"])
        print(json.dumps({"tool": "feature_bench", "part": "c", "pixels": pix, "frames": T, "height": H, "width": W, "K": K,
                          "count": int(cnt[0]), "klt_ms": round(a, 3), "tracks_same_points_ms": round(b, 3),
                          "ratio": round(a / b, 4), "equal": same}), flush=True)
        if not same:
            sys.exit(f"feature_bench: the KLT call differs from detection + tracks ({pix})")


if __name__ == "__main__":
    main()
