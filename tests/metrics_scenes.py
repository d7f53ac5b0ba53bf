"""Scenes for the masked flow metrics (test infrastructure).  Each scene is built for one kind of mistake a reduction kernel
makes and returns (u, v, ut, vt, region): float32 (B, H, W) predictions, float32 (B,) truths, slice bounds (y0, y1, x0, x1).

Everything is generated from integer hashing (64-bit wrap-around products, exact float64 steps), never from a library's
random stream, so the arrays are the same bytes on every machine; tests/golden/reference_metrics.json holds a sha256 of each
scene and the tests compare it before anything else.

Families (SCENES maps name -> builder; FAMILY maps name -> family):
  edges     rectangle off by one: prediction = truth except power-of-two spikes on the region's four inner corners and on
            their eight neighbours just outside, over 12 regions x 6 frames
  once      an element dropped, doubled or misplaced by the e / rw, e % rw unflattening or the 64 x 256 grid stride; a
            truth or plane of another pair (blockIdx.y addressing)
  values    NaN, +-inf, overflow, subnormals, the "nothing moves" branch, the cosine's clip
  sizes     long sums and many pairs
  noise     the fields of tests/test_gpu_metrics.py (truth + noise)
"""
from __future__ import annotations

import hashlib

import numpy as np

def hash64(idx, seed: int):
    """splitmix64 finaliser of (idx + seed * golden ratio), uint64 arrays, wrap-around arithmetic"""
    with np.errstate(over="ignore"):
        z = np.asarray(idx, np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise(shape, seed: int, sigma: float):
    """float64 field, mean 0, standard deviation sigma: the sum of two 24-bit uniforms (a triangle), every step exact or a
    single IEEE rounding"""
    n = int(np.prod(shape))
    h = hash64(np.arange(n, dtype=np.uint64), seed)
    a = (h >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    b = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return ((a + b - 1.0) * (sigma * 2.449489742783178)).reshape(shape)


def noisy(shape, seed, truth, su=1.5, sv=0.7):
    """(u, v) float32 of one pair: truth + noise"""
    return ((truth[0] + noise(shape, seed, su)).astype(np.float32), (truth[1] + noise(shape, seed + 1000, sv)).astype(np.float32))


def pack(u, v, ut, vt, region):
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    if u.ndim == 2:
        u, v = u[None], v[None]
    ut = np.ascontiguousarray(np.broadcast_to(np.asarray(ut, np.float32), (u.shape[0],)))
    vt = np.ascontiguousarray(np.broadcast_to(np.asarray(vt, np.float32), (u.shape[0],)))
    return u, v, ut, vt, tuple(int(r) for r in region)


def digest(scene) -> str:
    """sha256 over the scene's shapes, region and raw bytes (the NaN scenes hold the one quiet NaN np.nan gives)"""
    u, v, ut, vt, region = scene
    h = hashlib.sha256()
    h.update(repr((u.shape, region)).encode())
    for a in (u, v, ut, vt):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


def clipped(region, H, W):
    """NumPy's own word on the rectangle (independent of metrics_model.rectangle): (y0, y1, x0, x1), y1 = y0 if empty"""
    ys, xs = range(H)[region[0]:region[1]], range(W)[region[2]:region[3]]
    return ys.start, ys.start + len(ys), xs.start, xs.start + len(xs)


# ---- edges -------------------------------------------------------------------------------------------------------------
EDGE_FRAMES = ((1, 1), (1, 37), (41, 1), (67, 91), (240, 320), (1081, 1923))
EDGE_TRUTH = (2.0, -1.0)


def edge_regions(H, W):
    return {
        "whole": (0, H, 0, W),
        "pixel": (H // 2, H // 2 + 1, W // 2, W // 2 + 1),
        "row": (H // 3, H // 3 + 1, W // 5, W - W // 5),
        "col": (H // 5, H - H // 5, W // 3, W // 3 + 1),
        "verifier": (10, -10, 10, -10),
        "beyond": (-H - 3, H + 5, -W - 1, W + 2),
        "negative": (-H + 1, -1, 1 - W, -1),
        "halfout": (H // 2, H + 7, -W - 4, W // 2 + 1),
        "reversed": (H // 2 + 3, H // 2 - 3, 0, W),
        "reversed_neg": (-2, 2, 0, W),
        "zero_width": (0, H, W // 2, W // 2),
        "zeros": (0, 0, 0, 0),
    }


EDGE_REGIONS = tuple(edge_regions(8, 8))


def edges(H, W, which):
    """Rectangle off by one on any side, clipping or negative bounds wrong, an empty slice not empty.  Prediction = truth
    except spikes 2^4 .. 2^15 (u) and 2^15 .. 2^4 (v): the four inner corners of the region, then the eight pixels next to
    them just outside it (those inside the frame).  Every spike is a distinct power of two, so each mean names the set of
    pixels that were summed.  An empty region gets spikes on the frame's corners and centre, which must not be read."""
    region = edge_regions(H, W)[which]
    y0, y1, x0, x1 = clipped(region, H, W)
    u = np.full((H, W), EDGE_TRUTH[0], np.float32)
    v = np.full((H, W), EDGE_TRUTH[1], np.float32)
    if y1 > y0 and x1 > x0:
        cells = [(y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1)]
        for cy, dy in ((y0, -1), (y1 - 1, 1)):
            for cx, dx in ((x0, -1), (x1 - 1, 1)):
                cells += [(cy + dy, cx), (cy, cx + dx)]
    else:
        cells = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
    for k, (y, x) in enumerate(cells):
        inner = k < 4 and y1 > y0 and x1 > x0
        if 0 <= y < H and 0 <= x < W and (inner or not (y0 <= y < y1 and x0 <= x < x1)):
            u[y, x] = EDGE_TRUTH[0] + 2.0 ** (4 + k)
            v[y, x] = EDGE_TRUTH[1] - 2.0 ** (15 - k)
    return pack(u, v, *EDGE_TRUTH, region)


# ---- every element once ------------------------------------------------------------------------------------------------
ONCE_FRAME, ONCE_REGION = (150, 211), (3, 143, 5, 206)   # 140 x 201 = 28 140 elements: more than one 16 384 grid stride


def once_positions():
    n = (ONCE_REGION[1] - ONCE_REGION[0]) * (ONCE_REGION[3] - ONCE_REGION[2])
    fixed = [0, 255, 256, 16383, 16384, 16385, n - 1]
    hashed = [int(x) for x in hash64(np.arange(16, dtype=np.uint64), 77) % np.uint64(n)]
    return fixed + hashed


def once_spikes():
    """One spike per pair, at flattened region positions 0, 255, 256, 16 383, 16 384, 16 385, n - 1 and sixteen hashed ones,
    all 23 pairs in one call, every pair with its own truth: a pair that loses its pixel reads 0, one that reads another
    pair's truth or plane reads that truth's difference everywhere."""
    H, W = ONCE_FRAME
    y0, y1, x0, x1 = ONCE_REGION
    rw = x1 - x0
    pos = once_positions()
    B = len(pos)
    ut = (0.25 * np.arange(B) - 2.0).astype(np.float32)
    vt = (1.0 - 0.125 * np.arange(B)).astype(np.float32)
    u = np.broadcast_to(ut[:, None, None], (B, H, W)).copy()
    v = np.broadcast_to(vt[:, None, None], (B, H, W)).copy()
    for b, e in enumerate(pos):
        u[b, y0 + e // rw, x0 + e % rw] += np.float32(2.0 ** (5 + b % 8))
        v[b, y0 + e // rw, x0 + e % rw] -= np.float32(2.0 ** (3 + b % 5))
    return pack(u, v, ut, vt, ONCE_REGION)


ONCE_COUNTS = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (1, 257), 16383: (129, 127), 16384: (128, 128),
               16385: (145, 113), 32769: (9, 3641)}


def once_count(n):
    """A region of exactly n elements (rh x rw) with integer errors (i mod 7) + 1 in u and (3 i mod 7) + 1 in v at element
    i, errors of 1000 everywhere outside: an element dropped or doubled moves a mean by at least 1 / (7 n) > 4e-6 relative."""
    rh, rw = ONCE_COUNTS[n]
    assert rh * rw == n
    H, W = rh + 3, rw + 5
    ut, vt = 0.5, -0.25
    u = np.full((H, W), ut + 1000.0, np.float32)
    v = np.full((H, W), vt - 1000.0, np.float32)
    i = np.arange(n).reshape(rh, rw)
    u[1:1 + rh, 2:2 + rw] = ut + (i % 7 + 1)
    v[1:1 + rh, 2:2 + rw] = vt - (3 * i % 7 + 1)
    return pack(u, v, ut, vt, (1, 1 + rh, 2, 2 + rw))


# ---- values ------------------------------------------------------------------------------------------------------------
VAL_FRAME, VAL_REGION, VAL_TRUTH = (20, 20), (2, 18, 3, 17), (1.5, -0.75)
SPECIALS = (("u", np.nan), ("u", np.inf), ("u", -np.inf), ("v", np.nan), ("v", np.inf), ("v", -np.inf),
            ("u", 3e19), ("v", -3e19), ("u", 1e-40), ("v", -1e-40))
F32_BELOW = np.nextafter(np.float32(1e-6), np.float32(0))    # float32(1e-6) = 9.99999997e-07 is itself below 1e-6
F32_AT = np.float32(1e-6)
F32_ABOVE = np.nextafter(np.float32(1e-6), np.float32(1))
COS_OVER_ONE = (-18.897636, 12.139991)    # (up*ut + vp*vt + 1) / (norm_p * norm_t) rounds to 1.0000001 for up = ut, vp = vt
COS_BELOW_ONE = (2.5, 0.5)                # ... and to 0.99999994 here (test_metrics_cpu.py checks both)


def special_values(inside: bool):
    """One pair per special value (NaN, +-inf: the cosine is NaN; 3e19: squares overflow, cosine 0; 1e-40: subnormal) put on
    one pixel of a noise field, inside the region (each changes the outputs' class as the reference says) or on two pixels
    just outside it (nothing changes).  fmaxf / fminf clips and fmax reductions drop the NaN."""
    H, W = VAL_FRAME
    us, vs = [], []
    for k, (plane, val) in enumerate(SPECIALS):
        u, v = noisy((H, W), 300 + k, VAL_TRUTH)
        a = u if plane == "u" else v
        if inside:
            a[9, 9 + k % 3] = val
        else:
            a[1, 9] = val
            a[10, 17] = val
        us.append(u)
        vs.append(v)
    return pack(np.stack(us), np.stack(vs), *VAL_TRUTH, VAL_REGION)


def zero_truth():
    """Truth (0, 0): the "nothing moves and nothing was predicted" branch.  Pairs: 0 all zero (0.0); 1 one NaN pixel inside
    (aae NaN: a max that drops NaN gives 0.0); 2 the NaN outside (0.0); 3 every |pred| one float32 step below 1e-6 (0.0);
    4 as 3 with one pixel one step above (the general formula); 5 as 3 with one pixel at float32(1e-6) itself, which is
    below the reference's 1e-6 only because NumPy compares in float32 (the general formula)."""
    H, W = VAL_FRAME
    z = np.zeros((H, W), np.float32)
    below = np.full((H, W), F32_BELOW, np.float32)
    us = [z.copy(), z.copy(), z.copy(), below.copy(), below.copy(), below.copy()]
    vs = [z.copy() for _ in us]
    us[1][7, 8] = np.nan
    us[2][1, 8] = np.nan
    vs[2][7, 17] = np.nan
    us[4][5, 6] = F32_ABOVE
    vs[5][16, 16] = F32_AT
    us[5][16, 16] = 0.0
    return pack(np.stack(us), np.stack(vs), 0.0, 0.0, VAL_REGION)


def truth_threshold(empty: bool):
    """Truth magnitude one float32 step either side of 1e-6 (pairs 0, 1: along u; 2, 3: along v), prediction zero.  On a
    non-empty region both sides give aae = 0 (the cosine rounds to 1); on an EMPTY region the side below gives 0.0 and the
    side above the mean of nothing, NaN: that is where the threshold shows."""
    H, W = VAL_FRAME
    z = np.zeros((4, H, W), np.float32)
    ut = np.array([F32_AT, F32_ABOVE, 0, 0], np.float32)
    vt = np.array([0, 0, -F32_AT, -F32_ABOVE], np.float32)
    return pack(z, z.copy(), ut, vt, (5, 5, 0, W) if empty else VAL_REGION)


def cosine_clip():
    """Prediction equal to the truth.  Pair 0: the float32 cosine rounds to 1.0000001, which only the clip brings back to
    1 (angle 0; without it arccos gives NaN).  Pair 1: the cosine rounds to 0.99999994 and the angle is 0.0198 degrees on
    every pixel although the error is zero: the reference's value, kept."""
    H, W = VAL_FRAME
    ut = np.array([COS_OVER_ONE[0], COS_BELOW_ONE[0]], np.float32)
    vt = np.array([COS_OVER_ONE[1], COS_BELOW_ONE[1]], np.float32)
    u = np.broadcast_to(ut[:, None, None], (2, H, W)).copy()
    v = np.broadcast_to(vt[:, None, None], (2, H, W)).copy()
    return pack(u, v, ut, vt, VAL_REGION)


# ---- sizes and noise ---------------------------------------------------------------------------------------------------
def whole_frame(H, W, seed, truth):
    """Whole-frame truth + noise: n up to 3.3e7, where the reference's float32 pairwise mean is furthest from the exact one
    and where a 32-bit element index or plane offset would wrap"""
    u, v = noisy((H, W), seed, truth)
    return pack(u, v, *truth, (0, H, 0, W))


def many_pairs(B, H, W, seed):
    """B pairs with hashed truths and small-integer errors: pair addressing beyond a handful of pairs, and beyond the 65 535
    grid rows one launch can have"""
    k = hash64(np.arange(B, dtype=np.uint64), seed)
    ut = ((k & np.uint64(31)).astype(np.float64) * 0.25 - 4.0).astype(np.float32)
    vt = (((k >> np.uint64(8)) & np.uint64(31)).astype(np.float64) * 0.125 - 2.0).astype(np.float32)
    e = hash64(np.arange(B * H * W, dtype=np.uint64), seed + 1).reshape(B, H, W)
    u = (ut[:, None, None] + ((e & np.uint64(7)).astype(np.float32) - 3.0)).astype(np.float32)
    v = (vt[:, None, None] + (((e >> np.uint64(8)) & np.uint64(7)).astype(np.float32) - 4.0) * np.float32(0.5)).astype(np.float32)
    return pack(u, v, ut, vt, (0, H, 0, W) if B > 1000 else (1, -1, 2, -3))


NOISE_CASES = {   # the shapes, regions and truths of tests/test_gpu_metrics.py, and the verifier's region at 1080p
    "noise/240x320_border": ((240, 320), (10, -10, 10, -10), (2.0, 0.0)),
    "noise/240x320_crop": ((240, 320), (70, 170, 110, 210), (0.0, 0.0)),
    "noise/67x91_whole": ((67, 91), (0, 67, 0, 91), (-1.5, 0.75)),
    "noise/33x40_row": ((33, 40), (5, 6, 7, 39), (15.0, -3.0)),
    "noise/1080x1920_border": ((1080, 1920), (10, -10, 10, -10), (-3.25, 1.5)),
}


def noise_case(name):
    """truth + noise over a rectangle: the fields the first metrics tests used"""
    shape, region, truth = NOISE_CASES[name]
    u, v = noisy(shape, sum(shape), truth)
    return pack(u, v, *truth, region)


# ---- registry ----------------------------------------------------------------------------------------------------------
SCENES = {}
FAMILY = {}


def _add(name, family, fn, *args):
    SCENES[name] = lambda: fn(*args)
    SCENES[name].__doc__ = fn.__doc__
    FAMILY[name] = family


for _H, _W in EDGE_FRAMES:
    for _r in EDGE_REGIONS:
        _add(f"edges/{_H}x{_W}/{_r}", "edges", edges, _H, _W, _r)
_add("once/spikes", "once", once_spikes)
for _n in ONCE_COUNTS:
    _add(f"once/count_{_n}", "once", once_count, _n)
_add("values/special_inside", "values", special_values, True)
_add("values/special_outside", "values", special_values, False)
_add("values/zero_truth", "values", zero_truth)
_add("values/truth_threshold", "values", truth_threshold, False)
_add("values/truth_threshold_empty", "values", truth_threshold, True)
_add("values/cosine_clip", "values", cosine_clip)
_add("sizes/2160x3840", "sizes", whole_frame, 2160, 3840, 4, (1.0, -2.0))
_add("sizes/4320x7680", "sizes", whole_frame, 4320, 7680, 8, (-0.5, 0.25))
_add("sizes/B300_33x40", "sizes", many_pairs, 300, 33, 40, 5)
_add("sizes/B65537_2x3", "sizes", many_pairs, 65537, 2, 3, 6)
for _name in NOISE_CASES:
    _add(_name, "noise", noise_case, _name)

BIG = ("sizes/2160x3840", "sizes/4320x7680")          # scenes a test builds one at a time and lets go of
MANY = "sizes/B65537_2x3"
MANY_SAMPLE = tuple(range(0, 65537, 257)) + (65534, 65535, 65536)   # the pairs the reference fixture records of MANY


def scene(name):
    return SCENES[name]()


def fixture():
    """tests/golden/reference_metrics.json: the reference's numbers for these scenes"""
    import json
    from pathlib import Path

    return json.loads((Path(__file__).resolve().parent / "golden" / "reference_metrics.json").read_text())


def checked_scene(name, fix):
    """the scene, after its digest was compared with the fixture's: a scene that drifted fails here, loudly"""
    sc = scene(name)
    assert digest(sc) == fix["scenes"][name]["sha256"], f"scene {name} is not the one the reference was run on"
    return sc


def fixture_pairs(name, fix):
    """the pair indices the fixture's rows of `name` stand for"""
    return fix["scenes"][name].get("pairs", list(range(fix["scenes"][name]["B"])))
