#!/usr/bin/env python3
"""The reference's masked metrics on the scenes of tests/metrics_scenes.py, by IMPORTING THE REFERENCE (build container
only; the output is data).  Output: tests/golden/reference_metrics.json, numbers, digests and scene names only.

Per scene: metrics_scenes.digest of its arrays, B, the region's pixel count, and per pair the five numbers of the reference's
compute_all_metrics(u, v, float(ut), float(vt), mask) with the boolean mask[y0:y1, x0:x1] = True (NaN and +-inf as the
strings "nan", "inf", "-inf").  The truths are float32-representable, so the Python floats the reference gets are the numbers
the device gets.  Of the B = 65 537 scene the pairs metrics_scenes.MANY_SAMPLE are recorded.

Once: the NumPy version, and `arccos_deg_term_error`: the largest |np.rad2deg(np.arccos(c)) in float32 - arccos(float64(c)) *
57.29577951308232| over every clipped cosine c of every scene's region (a property of NumPy's float32 arccos / rad2deg, not
of the code under test; tests allow twice it per term of the angular mean).

Re-running reproduces the file byte for byte.
Usage:  python tests/golden/make_golden_metrics.py      (about 2 min)
"""
from __future__ import annotations

import json
import math
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, "/root/reference/python")
import flow_metrics as R  # noqa: E402  (reference)
import metrics_model as M  # noqa: E402
import metrics_scenes as S  # noqa: E402

assert "compute_all_metrics_gpu" not in dir(R), "this is the product's flow_metrics, not the reference's"


def word(x: float):
    x = float(x)
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return x


def term_error(u, v, ut, vt, rect) -> float:
    y0, y1, x0, x1 = rect
    if M.count(rect) == 0:
        return 0.0
    c = M.pixel_terms(u[y0:y1, x0:x1].reshape(-1), v[y0:y1, x0:x1].reshape(-1), ut, vt)[4]
    c = c[~np.isnan(c)]
    if c.size == 0:
        return 0.0
    lo = np.rad2deg(np.arccos(c))
    assert lo.dtype == np.float32
    return float(np.max(np.abs(lo.astype(np.float64) - np.arccos(c.astype(np.float64)) * M.RAD2DEG)))


def main():
    np.seterr(all="ignore")
    warnings.simplefilter("ignore")   # the mean of an empty slice
    scenes, worst = {}, 0.0
    for name in S.SCENES:
        sc = S.scene(name)
        u, v, ut, vt, region = sc
        B, H, W = u.shape
        rect = M.rectangle(region, H, W)
        mask = np.zeros((H, W), bool)
        mask[region[0]:region[1], region[2]:region[3]] = True
        assert int(mask.sum()) == M.count(rect)
        pairs = list(S.MANY_SAMPLE) if name == S.MANY else list(range(B))
        rows = []
        for b in pairs:
            m = R.compute_all_metrics(u[b], v[b], float(ut[b]), float(vt[b]), mask)
            rows.append([word(m[k]) for k in M.KEYS])
            worst = max(worst, term_error(u[b], v[b], ut[b], vt[b], rect))
        scenes[name] = {"sha256": S.digest(sc), "B": B, "n": M.count(rect), "metrics": rows}
        if name == S.MANY:
            scenes[name]["pairs"] = pairs
        print(name, flush=True)
    doc = {"numpy": np.__version__, "keys": list(M.KEYS), "arccos_deg_term_error": worst, "scenes": scenes}
    out = HERE / "reference_metrics.json"
    out.write_text(json.dumps(doc, indent=0, sort_keys=True) + "\n")
    print(out, out.stat().st_size, "bytes; arccos term error", worst)


if __name__ == "__main__":
    main()
