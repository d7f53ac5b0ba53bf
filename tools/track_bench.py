#!/usr/bin/env python3
"""Point tracks through a frame sequence: frames in, tracks out, against the forward-backward call with every output
(development tool, not part of the bench contract).

Host arrays, seeded content: T frames of 1080p (a synthetic scene drifting by one row and two columns per frame, with
seeded noise).  For each pixel type, host to host, alternating which goes first, for a bounded number of steps:
  (a) oflk_pyramidal_sequence_fb with every output (four flows, two error planes, two masks);
  (b) oflk_pyramidal_sequence_tracks for N queries at frame 0 in raster order: N = 10 000 (the first 10 000 pixels of an
      evenly spaced grid), H*W/16 (every 4th pixel of every 4th row) and H*W (every pixel).
It prints one JSON line per (pixel type, N) with ms per call (median over the steps) and whether the tracks equal the
statement of tests/track_model.py applied to (a)'s flows (on every 16th query for N = H*W: tracks are independent per
query).  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`.

    python tools/track_bench.py [--frames 129] [--steps 3] [--warmup 1] [--pixels f32,u8] [--no-check]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=3, help="timed calls of each form (at most 20)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pixels", default="f32,u8")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the statement")
    args = ap.parse_args()
    if args.frames < 2:
        ap.error("--frames must be >= 2")
    steps = max(1, min(args.steps, 20))
    import numpy as np

    import _oflk
    from oflk_synth import synth_pair

    T, H, W = args.frames, args.height, args.width
    B = T - 1
    base = synth_pair(H, W, pair_index=args.seed)[0].astype(np.float32)
    rng = np.random.default_rng(args.seed)
    f32 = np.empty((T, H, W), np.float32)
    for t in range(T):
        f32[t] = np.clip(np.roll(base, (t, 2 * t), axis=(0, 1)) + rng.normal(0.0, 1.5, (H, W)).astype(np.float32), 0.0, 255.0)
    frames = {"f32": f32, "u8": np.rint(f32).astype(np.uint8)}
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    every = np.stack([xx.ravel(), yy.ravel()], 1)
    sub16 = np.ascontiguousarray(np.stack([xx[::4, ::4].ravel(), yy[::4, ::4].ravel()], 1))
    k = max(1, int(np.sqrt(H * W / 10000)))
    sparse = np.ascontiguousarray(np.stack([xx[::k, ::k].ravel(), yy[::k, ::k].ravel()], 1)[:10000])
    query_sets = [("10000", sparse), ("HW/16", sub16), ("HW", every)]
    L = _oflk.lib()
    fb_out = [np.empty((B, H, W), np.float32) for _ in range(6)] + [np.empty((B, H, W), np.uint8) for _ in range(2)]

    for pix in args.pixels.split(","):
        fr = frames[pix]
        u8 = pix == "u8"
        src = fr.ctypes.data if u8 else _oflk.ptr(fr)
        fb_fn = L.oflk_pyramidal_sequence_fb_u8 if u8 else L.oflk_pyramidal_sequence_fb
        tr_fn = L.oflk_pyramidal_sequence_tracks_u8 if u8 else L.oflk_pyramidal_sequence_tracks
        outs = {}
        for name, q in query_sets:
            N = len(q)
            outs[name] = (np.empty((T, N, 2), np.float32), np.empty((T, N), np.uint8))

        def call(form):
            if form == "fb":
                _oflk.check(fb_fn(src, T, H, W, 3, 5, 3, 0.01, 0.5, *(_oflk.ptr(o) for o in fb_out[:6]), fb_out[6].ctypes.data,
                                  fb_out[7].ctypes.data))
                return
            q = dict(query_sets)[form]
            tr, vis = outs[form]
            _oflk.check(tr_fn(src, T, H, W, 3, 5, 3, 0.01, 0.5, None, _oflk.ptr(q), len(q), _oflk.ptr(tr), vis.ctypes.data))

        forms = ["fb"] + [n for n, _ in query_sets]
        for _ in range(args.warmup):
            for form in forms:
                call(form)
        ms = {f: [] for f in forms}
        for i in range(steps):
            order = forms if i % 2 == 0 else forms[::-1]
            for form in order:
                t0 = time.perf_counter()
                call(form)
                ms[form].append((time.perf_counter() - t0) * 1e3)
        call("fb")   # the flows the statement is applied to
        fb_ms = statistics.median(ms["fb"])
        for name, q in query_sets:
            tr, vis = outs[name]
            line = {"tool": "track_bench", "pixels": pix, "frames": T, "pairs": B, "height": H, "width": W, "levels": 3,
                    "window": 5, "iters": 3, "steps": steps, "queries": name, "N": len(q),
                    "tracks_ms": round(statistics.median(ms[name]), 3), "fb_all_outputs_ms": round(fb_ms, 3)}
            line["speedup"] = round(line["fb_all_outputs_ms"] / line["tracks_ms"], 3)
            line["visible_last_row"] = round(float(vis[-1].mean()), 4)
            if not args.no_check:
                import track_model as M

                sel = slice(None, None, 16) if name == "HW" else slice(None)
                want_tr, want_vis = M.track(*fb_out[:4], None, q[sel])
                got_tr, got_vis = tr[:, sel], vis[:, sel]
                line["checked_queries"] = int(got_vis.shape[1])
                line["equals_statement"] = bool(np.array_equal(got_vis, want_vis) and
                                                np.array_equal(got_tr, want_tr, equal_nan=True))
            print(json.dumps(line), flush=True)
            if not args.no_check and not line["equals_statement"]:
                sys.exit(f"track_bench: tracks differ from the statement ({pix}, N={len(q)})")


if __name__ == "__main__":
    main()
