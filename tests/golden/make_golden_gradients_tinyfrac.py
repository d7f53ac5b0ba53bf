#!/usr/bin/env python3
"""The reference's compute_gradients on subnormal frames off the 2^9-ulp grid, by IMPORTING THE REFERENCE (build container
only; the output is data).  Output: tests/golden/reference_gradients_tinyfrac.npz, about 22 KB.

Input: the `odd` 45 x 61 crop of tests/range_scenes.py under the gradient scenes of tests/range_feature_scenes.py:
`tinyfrac`, f32((x + 1/3) * 2^-140), and `tinyulp`, x * 2^-149 (the one on which a Sobel product lands on a rounding tie when
the frame's values are integers).  Recorded per scene: <scene>/Ix, <scene>/Iy, <scene>/It as float32, the reference's own
arrays.  tests/golden/reference_ranges.npz is not touched.

Re-running reproduces the file byte for byte (sorted members, fixed zip timestamps).
Usage:  python tests/golden/make_golden_gradients_tinyfrac.py <the reference's python directory>
"""
from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def main(reference_python: str):
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, reference_python)
    import lucas_kanade_core as R_core  # the reference
    import range_feature_scenes as F

    assert Path(R_core.__file__).resolve().parent == Path(reference_python).resolve(), R_core.__file__
    np.seterr(all="ignore")
    arrays = {}
    for name in F.GRADIENT_SCENES:
        p, c = F.gradient_pair(name)
        for nm, a in zip(("Ix", "Iy", "It"), R_core.compute_gradients(p, c)):
            a = np.asarray(a)
            assert a.dtype == np.float32 and a.shape == p.shape, (name, nm, a.dtype, a.shape)
            arrays[f"{name}/{nm}"] = a
    out = HERE / "reference_gradients_tinyfrac.npz"
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
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
