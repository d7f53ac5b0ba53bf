"""Frame pairs outside the 8-bit value range, and the one rule by which flows on them are compared (test infrastructure).

Every scene applies one transform to both frames of a crop of the committed 13-pattern frames
(tests/golden/patterns_320x240.npz) and rounds to float32:

    unit     x / 255                          the |det| > 1e-4 cut-off is active: many windows sit between 1e-4 and 1e-3
    signed   (x - 128) / 128                  negative pixels through the pyramid and the warp
    u16      x * 257, rows 0..47 a            integers above 255 in whole 64 x 24 tiles (with their margins) whose
             low-texture ramp with a          windows all keep Sxx, Syy below 2^16: only the [0, 255] half of the
             temporal step of 25 000          streaming kernel's exactness test sends those tiles to the exact redo
    big      x * 1e9                          window products overflow: NaN flows from finite frames, NaN residual means
    steep    2^42 + 2^21 x, and -2^42 +       det stays finite while a numerator overflows: a +inf flow with no NaN
             2^21 x in the second frame       beside it, so the reference's residual mean is +inf
    huge     x * 1e12, two pixels near        products and p + q overflow: zero and NaN flows
             +-3e38
    tiny     x * 2^-140                       subnormal pixels and non-zero subnormal gradients
    small    x * 1e-20                        normal pixels whose products underflow
    holes    8-bit, NaN / +inf / -inf pixels  non-finite pixels inside, on row 0, on the last row and in the last two columns

Bases: `tm` and `rs` are 96 x 128 crops of translate_medium and rotate_small, `odd` a 45 x 61 crop of translate_medium.

The comparison rule (`same`): NaN positions equal, every other value equal as a value (-0 == +0: the project's +0.0
convention).  np.array_equal calls NaN unequal and is not used on these outputs.  `digest` is the
same rule as a hash: -0 is read as +0 and every NaN as the one quiet NaN.
"""
from __future__ import annotations

import hashlib
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
SCENES = ("unit", "signed", "u16", "big", "steep", "huge", "tiny", "small", "holes")
BASES = {
    "tm": ("translate_medium", (slice(60, 156), slice(80, 208))),
    "rs": ("rotate_small", (slice(60, 156), slice(80, 208))),
    "odd": ("translate_medium", (slice(100, 145), slice(150, 211))),
}
# scenes whose flows are finite at every configuration the fixture records
FINITE = ("unit", "signed", "u16", "tiny", "small")


def base_pair(base: str):
    name, crop = BASES[base]
    z = np.load(GOLDEN / "patterns_320x240.npz")
    p = np.ascontiguousarray(z["frame_0"][crop].astype(np.float32))
    c = np.ascontiguousarray(z[f"frame_1__{name}"][crop].astype(np.float32))
    return p, c


def _u16(x: np.ndarray, prev: bool) -> np.ndarray:
    y = x.astype(np.float64) * 257.0
    # rows 0..47, every column: a 30 / 20 per-pixel ramp with a little integer texture in each frame (|Ix| <= 34, so Sxx,
    # Syy < 2^16 even over a 7x7 window) and a temporal step of 25 000 between the frames: every product with It is far
    # past 2^24, so the order of the window sums matters
    H, W = x.shape
    h = min(48, H)
    yy, xx = np.mgrid[0:h, 0:W]
    tex = np.random.default_rng(7 if prev else 8).integers(0, 4, (h, W))
    y[:h] = 20000.0 + 30.0 * xx + 20.0 * yy + tex + (0.0 if prev else 25000.0)
    return y


def transform(scene: str, x: np.ndarray, prev: bool) -> np.ndarray:
    """the scene's values from the 8-bit frame x (float32 in [0, 255])"""
    x = x.astype(np.float64)
    if scene == "unit":
        y = x / 255.0
    elif scene == "signed":
        y = (x - 128.0) / 128.0
    elif scene == "u16":
        y = _u16(x, prev)
    elif scene == "big":
        y = x * 1e9
    elif scene == "steep":
        y = (2.0 ** 42 if prev else -2.0 ** 42) + 2.0 ** 21 * x   # exact in float32
    elif scene == "huge":
        y = x * 1e12
        H, W = x.shape
        y[H // 3, W // 4] = 3.0e38          # p + q overflows to +inf, and so does every product with its gradient
        y[H // 2, W // 2] = -3.1e38 if prev else -2.9e38
    elif scene == "tiny":
        y = x * 2.0 ** -140
    elif scene == "small":
        y = x * 1e-20
    elif scene == "holes":
        y = x.copy()
        H, W = x.shape
        if prev:
            y[H // 2, W // 3] = np.nan
            y[0, W // 5] = np.inf
            y[H - 1, W // 2] = -np.inf
            y[H // 4, W - 2] = np.nan
            y[3 * H // 4, W - 1] = np.inf
        else:
            y[H // 3, 2 * W // 3] = -np.inf
            y[0, W // 2 + 3] = np.nan
            y[H - 1, W // 4] = np.nan
            y[H // 2 + 5, W - 2] = -np.inf
            y[H // 5, W - 1] = np.nan
    else:
        raise KeyError(scene)
    return np.ascontiguousarray(y.astype(np.float32))


def scene(name: str, base: str = "tm"):
    """(prev, curr) float32 of scene `name` on crop `base`"""
    p, c = base_pair(base)
    return transform(name, p, True), transform(name, c, False)


def special_flow(H, W):
    """a flow whose coordinates are NaN, +-inf, +-1e30, -0, and land exactly on the last row / column"""
    rng = np.random.default_rng(11)
    u = rng.uniform(-2.5, 2.5, (H, W)).astype(np.float32)
    v = rng.uniform(-2.5, 2.5, (H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    u[::7, ::5] = np.nan
    v[3::11, 2::9] = np.nan
    u[1::13, ::4] = np.inf
    u[2::13, 1::4] = -np.inf
    v[4::13, 2::6] = np.inf
    v[5::13, 3::6] = -np.inf
    u[6::17, ::3] = np.float32(1e30)
    v[7::17, 1::3] = np.float32(-1e30)
    u[8::9, 4::7] = np.float32(-0.0)
    v[8::9, 4::7] = np.float32(-0.0)
    last_x = (xx % 6 == 1) & (yy % 5 == 2)
    u[last_x] = (W - 1 - xx[last_x]).astype(np.float32)       # x + u == W - 1 exactly
    last_y = (xx % 6 == 4) & (yy % 5 == 3)
    v[last_y] = (H - 1 - yy[last_y]).astype(np.float32)       # y + v == H - 1 exactly
    corner = (xx % 8 == 3) & (yy % 7 == 6)
    u[corner] = (W - 1 - xx[corner]).astype(np.float32)
    v[corner] = (H - 1 - yy[corner]).astype(np.float32)
    return u, v


def coarse_flow(h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 2.0, (h, w)).astype(np.float32)
    f[1, 2] = np.nan
    f[h // 2, w // 2] = np.inf
    f[h - 1, w - 1] = -np.inf
    f[0, w - 1] = np.nan
    return f


def canonical(a) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32) + np.float32(0.0)   # -0 -> +0
    a[np.isnan(a)] = np.float32(np.nan)
    return a


def digest(a) -> str:
    return hashlib.sha256(canonical(a).tobytes()).hexdigest()


def same(a, b) -> bool:
    """the comparison rule: same shape, NaN at the same positions, every other element equal as a value"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.all(a[~na] == b[~nb]))


def differ(a, b) -> str:
    """a short account of where `same` fails"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return f"shapes {a.shape} vs {b.shape}"
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a != b))
    idx = np.argwhere(bad)
    first = tuple(int(i) for i in idx[0]) if len(idx) else None
    return (f"{int(bad.sum())} of {a.size} differ (NaN {int(na.sum())} vs {int(nb.sum())}); first at {first}: "
            f"{a[first] if first else None} vs {b[first] if first else None}")


def assert_same(a, b, what: str = "") -> None:
    assert same(a, b), f"{what}: {differ(a, b)}"
