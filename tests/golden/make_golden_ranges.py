#!/usr/bin/env python3
"""Reference values on frames outside the 8-bit value range (the scenes of tests/range_scenes.py), by IMPORTING THE
REFERENCE (build container only; the output is data).  Output: tests/golden/reference_ranges.npz, about 0.6 MB.

Every flow, stage output and warp is recorded as range_scenes.digest (NaN read as one quiet NaN, -0 as +0, then sha256)
with its NaN and non-zero counts; the float32 values themselves are kept for the 3-level / 5x5 / 3-iteration flows of
the scenes whose flows are finite (the tolerant mode's grade needs them).  Recorded per scene on crop `tm` (96 x 128):
  * compute_gradients, build_gaussian_pyramid (3 levels) of the first frame, warp_image of the second frame with a flow
    that holds NaN, +-inf, +-1e30, -0 and targets exactly on the last row and column;
  * lucas_kanade_single_scale at windows 3, 5, 7, 13;
  * lucas_kanade_pyramidal at (levels, window, iterations) = (3,5,3), (2,7,2), (1,5,1), (4,5,3), (3,5,2), (1,5,2): the
    flow, every residual
    mean the reference compares with 0.01 (np.mean(np.abs(d)) of what its lucas_kanade_single_scale returns, float32)
    and the iterations run per level;
on crops `rs` (96 x 128) and `odd` (45 x 61): window 5 and the tolerant mode's four cells (3,5,3), (3,5,2), (1,5,1),
(1,5,2) only.  Once: upsample_flow of coarse flows holding
NaN and +-inf, the reference's stdout of (3,5,3) on `unit` and `big`, and the numpy / scipy versions (map_coordinates
returns cval for NaN and +-inf coordinates: that behaviour is SciPy's).

Re-running reproduces the file byte for byte (sorted members, fixed zip timestamps).
Usage:  python tests/golden/make_golden_ranges.py      (about 3 min)
"""
from __future__ import annotations

import contextlib
import io
import json
import re
import sys
import zipfile
from pathlib import Path

import numpy as np
import scipy

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, "/root/reference/python")
import lucas_kanade_core as R_core  # noqa: E402  (reference)
import lucas_kanade_pyramidal as R_pyr  # noqa: E402  (reference)
import range_scenes as S  # noqa: E402

R_pyr.visualize_pyramid_level = lambda *a, **k: None   # the PNG side effect is not wanted here

SINGLE = (3, 5, 7, 13)
PYRAMIDAL = ((3, 5, 3), (2, 7, 2), (1, 5, 1), (4, 5, 3), (3, 5, 2), (1, 5, 2))
ENVELOPE = ((3, 5, 3), (3, 5, 2), (1, 5, 1), (1, 5, 2))   # the tolerant mode's cells: recorded on every crop
KEEP = (3, 5, 3)   # the configuration whose flows are stored as values (finite scenes)
STDOUT = ("unit", "big")


def record(meta, key, a):
    a = np.asarray(a, np.float32)
    meta[key] = {"sha256": S.digest(a), "nan": int(np.isnan(a).sum()), "nonzero": int(np.count_nonzero(a)),
                 "shape": list(a.shape)}


def pyramidal(p, c, levels, win, iters):
    """(u, v, means[levels, iters, 2] float32 (0 where not run), iters_run[levels], stdout)"""
    means = []
    inner = R_pyr.lucas_kanade_single_scale

    def wrapped(a, b, window_size=5):
        du, dv = inner(a, b, window_size)
        means.append((np.mean(np.abs(du)), np.mean(np.abs(dv))))
        return du, dv

    R_pyr.lucas_kanade_single_scale = wrapped
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            u, v = R_pyr.lucas_kanade_pyramidal(p, c, levels, win, iters)
    finally:
        R_pyr.lucas_kanade_single_scale = inner
    runs = np.zeros(levels, np.int32)
    level = -1
    for line in buf.getvalue().splitlines():
        m = re.search(r"Processing pyramid level (\d+)/", line)
        if m:
            level = int(m.group(1))
        m = re.search(r"Iteration (\d+)/", line)
        if m:
            runs[level] = int(m.group(1))
    assert int(runs.sum()) == len(means), (runs, len(means))
    log = np.zeros((levels, iters, 2), np.float32)
    i = 0
    for l in range(levels):
        for k in range(runs[l]):
            assert means[i][0].dtype == np.float32 and means[i][1].dtype == np.float32
            log[l, k] = means[i]
            i += 1
    return np.asarray(u, np.float32), np.asarray(v, np.float32), log, runs, buf.getvalue()


def main():
    meta = {"numpy": np.__version__, "scipy": scipy.__version__, "single": list(SINGLE),
            "pyramidal": [list(t) for t in PYRAMIDAL], "stdout": {}}
    arrays = {}
    np.seterr(all="ignore")
    for h, w, seed in ((24, 32, 1), (23, 31, 2)):
        fu, fv = S.coarse_flow(h, w, seed), S.coarse_flow(h, w, seed + 10)
        for H, W in ((48, 64), (45, 61), (96, 128)):
            uu, uv = R_pyr.upsample_flow(fu, fv, (H, W))
            record(meta, f"upsample/{h}x{w}/{H}x{W}/u", uu)
            record(meta, f"upsample/{h}x{w}/{H}x{W}/v", uv)
    for name in S.SCENES:
        for base in S.BASES:
            p, c = S.scene(name, base)
            key = f"{name}/{base}"
            record(meta, f"{key}/prev", p)
            record(meta, f"{key}/curr", c)
            full = base == "tm"
            if full:
                for nm, a in zip(("Ix", "Iy", "It"), R_core.compute_gradients(p, c)):
                    record(meta, f"{key}/grad/{nm}", np.asarray(a, np.float32))
                for l, a in enumerate(R_pyr.build_gaussian_pyramid(p, 3)):
                    record(meta, f"{key}/pyr/{l}", np.asarray(a, np.float32))
                su, sv = S.special_flow(*p.shape)
                record(meta, f"{key}/warp", R_pyr.warp_image(c, su, sv))
            for win in (SINGLE if full else (5,)):
                u, v = R_core.lucas_kanade_single_scale(p, c, win)
                record(meta, f"{key}/single/{win}/u", u)
                record(meta, f"{key}/single/{win}/v", v)
            for cfg in (PYRAMIDAL if full else ENVELOPE):
                u, v, log, runs, out = pyramidal(p, c, *cfg)
                ck = f"{key}/pyr_{cfg[0]}_{cfg[1]}_{cfg[2]}"
                record(meta, f"{ck}/u", u)
                record(meta, f"{ck}/v", v)
                arrays[f"{ck}/log"] = log
                arrays[f"{ck}/runs"] = runs
                if cfg == KEEP and name in S.FINITE:
                    arrays[f"{ck}/u"], arrays[f"{ck}/v"] = u, v
                if cfg == KEEP and full and name in STDOUT:
                    meta["stdout"][name] = out
            print(key, flush=True)
    arrays["meta"] = np.array(json.dumps(meta, indent=0, sort_keys=True))
    out = HERE / "reference_ranges.npz"
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
