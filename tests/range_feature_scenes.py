"""Frames outside the 8-bit value range for the calls beyond the dense flow paths (test infrastructure): sparse LK and the
tracks, the warps, frame interpolation, the mosaic, direct alignment and its weights.

Every family keeps its own builder of float32 frames in [0, 255] (test_gpu_sparse._smooth / _shifted, align_model.planted_pair,
fb_model.occluder_scene, mosaic_model.pan_frames); range_scenes.transform is applied to what they give, unchanged, for
`signed`, `big`, `huge`, `tiny`, `small` and `holes`.  Two scenes are added:

    u16        x * 257                         plain: range_scenes._u16's ramp is a device for the streaming flow kernel
    tinyfrac   f32((x + 1/3) * 2^-140)         subnormal pixels off the 2^9-ulp grid of range_scenes' `tiny`: a Sobel product
                                               a * 0.125f rounds, so a fused multiply-add differs from convolve2d on ties

    tinyulp    x * 2^-149                      gradients only: integer multiples of the subnormal ulp

The builders' frames are not integers, so `tiny` and `tinyfrac` applied to them are off that grid at arbitrary multiples of the
ulp.  On an INTEGER frame (the committed 8-bit crops) `tinyfrac` is not enough: f32((x + 1/3) * 2^-140) is 512 x + 171 ulps, every
pixel and every frame average is 3 mod 8 ulps, and a product by 1/8 or 1/4 never lands on a tie, which is the only place where one
rounding and two differ.  `tinyulp` is the scene that separates the two orders on the integer crops: a pixel of x ulps ties under
1/8 where x = 4 mod 8 and under 1/4 where x = 2 mod 4.

In a sequence, frame t takes transform's `prev` placement of the holes for even t and the `curr` placement for odd t.

Two placements of holes go beyond transform's: `ring_points` (sparse LK: a hole that lies only on the outer ring of a point's
(w+2)^2 patch) and `holes_unsampled` (alignment: holes that no counted pixel reads).
"""
from __future__ import annotations

import numpy as np

import range_scenes as S

SCENES = ("signed", "u16", "big", "huge", "tiny", "tinyfrac", "small", "holes")
SUBNORMAL = ("tiny", "tinyfrac")


def transform(scene: str, x: np.ndarray, prev: bool) -> np.ndarray:
    """the scene's values from the frame x (float32 in [0, 255])"""
    if scene == "u16":
        return np.ascontiguousarray((x.astype(np.float64) * 257.0).astype(np.float32))
    if scene == "tinyfrac":
        return np.ascontiguousarray(((x.astype(np.float64) + 1.0 / 3.0) * 2.0 ** -140).astype(np.float32))
    if scene == "tinyulp":
        return np.ascontiguousarray((x.astype(np.float64) * 2.0 ** -149).astype(np.float32))
    return S.transform(scene, x, prev)


def frames_of(scene: str, frames) -> np.ndarray:
    """transform of every frame of a sequence (T, H, W): `prev` for even t (for every t where the frame has fewer than 12
    rows, which the `curr` placement of the holes needs)"""
    tall = np.shape(frames)[1] >= 12
    return np.stack([transform(scene, np.asarray(f, np.float32), t % 2 == 0 or not tall) for t, f in enumerate(frames)])


def assert_same(got, want, what: str = "") -> None:
    """range_scenes.assert_same's rule in the arrays' own type: one shape and dtype; floating point: NaN at the same
    positions, every other element equal as a value (float64 stays float64); anything else: equal"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.dtype}{g.shape} against {w.dtype}{w.shape}"
    if g.dtype.kind != "f":
        bad = g != w
        assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} differ, first at {np.argwhere(bad)[0].tolist()}: " \
                              f"{g[bad][:4]} vs {w[bad][:4]}"
        return
    ng, nw = np.isnan(g), np.isnan(w)
    bad = (ng != nw) | (~ng & ~nw & (g != w))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} differ (NaN {int(ng.sum())} vs {int(nw.sum())}), first at " \
                          f"{np.argwhere(bad)[0].tolist()}: {g[bad][:4]} vs {w[bad][:4]}"


GRADIENT_SCENES = ("tinyfrac", "tinyulp")


def gradient_pair(scene: str):
    """(prev, curr) of the committed `odd` crop (45 x 61) under a gradient scene: the input of
    tests/golden/reference_gradients_tinyfrac.npz"""
    p, c = S.base_pair("odd")
    return transform(scene, p, True), transform(scene, c, False)


def hole_positions(frame) -> list:
    """(x, y) of every pixel that is not finite"""
    ys, xs = np.nonzero(~np.isfinite(frame))
    return [(int(x), int(y)) for x, y in zip(xs, ys)]


# ---- sparse LK -------------------------------------------------------------------------------------------------------
def sparse_frames(H, W, T=2):
    """a textured frame and its shifts by 1 px per frame in x (the 8-bit base of every sparse scene)"""
    from test_gpu_sparse import _shifted, _smooth

    a = _smooth(H, W, H * 7 + W)
    return np.stack([a] + [_shifted(a, float(t), 0.0) for t in range(1, T)])


def ring_points(holes, H, W, w) -> np.ndarray:
    """for every hole (hx, hy) and the half-window h of w, the query points inside the frame among
        (hx, hy + h + 1)          the hole is the top middle of the (w+2)^2 patch's ring: a zero tap of Ix and a 1/4 tap of Iy
                                  of one window element
        (hx + h + 1, hy)          the mirror case: a zero tap of Iy
        (hx + h + 1, hy + h + 1)  the ring's corner
        (hx + 1, hy)              the window holds the hole
        (hx + w + 3, hy)          more than w + 2 away: the patch does not see it"""
    h = w // 2
    out = []
    for hx, hy in holes:
        for dx, dy in ((0, h + 1), (h + 1, 0), (h + 1, h + 1), (1, 0), (w + 3, 0)):
            x, y = hx + dx, hy + dy
            if 0 <= x <= W - 1 and 0 <= y <= H - 1:
                out.append((x, y))
    return np.array(out, np.float32).reshape(-1, 2)


def sparse_points(frame, w, n=60, seed=3) -> np.ndarray:
    """n query points (N, 2) float32: a grid of non-integer positions, with ring_points of the frame's holes in front"""
    H, W = frame.shape
    ring = ring_points(hole_positions(frame), H, W, w)[:n // 2]
    rng = np.random.default_rng(seed)
    k = n - len(ring)
    pts = np.stack([rng.uniform(2.0, W - 3.0, k), rng.uniform(2.0, H - 3.0, k)], 1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([ring, pts]), np.float32)


# ---- warps, interpolation, mosaic ------------------------------------------------------------------------------------
def warp_frames(scene: str, H, W):
    """two float32 frames (2, H, W) of the scene: the textured frame of the sparse scenes and its 1 px shift"""
    return frames_of(scene, sparse_frames(H, W))


def warp_maps(H, W, perspective: bool) -> dict:
    """name -> map (6,) or (9,) float64.  identity: integer source positions, so the weight-0 tap of a sample falls on the
    next pixel -- a hole, or past the last column and row; half: a (0.5, 0.5) translation; rotation: 0.05 rad about the centre;
    projective (perspective only): the rotation with a third row that is not (0, 0, 1); behind (perspective only): the
    half-pixel translation with all nine coefficients negated -- every source position lies inside the frame and every
    divisor is negative, so the whole output is outside and no hole may reach it"""
    c, s = np.cos(0.05), np.sin(0.05)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    rot = [c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy]
    maps = {"identity": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], "half": [1.0, 0.0, 0.5, 0.0, 1.0, 0.5], "rotation": rot}
    if perspective:
        maps = {k: v + [0.0, 0.0, 1.0] for k, v in maps.items()}
        maps["projective"] = rot + [2e-3, -1e-3, 1.0]
        maps["behind"] = [-v for v in maps["half"]]
    return {k: np.array(v, np.float64) for k, v in maps.items()}


def interp_frames(scene: str, B, H, W):
    """B + 1 frames of fb_model.occluder_scene scaled to the frame size"""
    import fb_model

    frames, _ = fb_model.occluder_scene(B + 1, H, W, size=min(H, W) // 3, step=(1, 1))
    return frames_of(scene, frames)


def unit_flows(B, H, W):
    """(uf, vf, ub, vb): +1 px forward in x and y, -1 px backward"""
    one = np.ones((B, H, W), np.float32)
    return [one, one.copy(), -one, -one]


MOSAIC = dict(F=3, H=20, W=28, margin=3)


def mosaic_scene(scene: str, projective: bool, behind: bool = False):
    """(frames (3, 20, 28) float32, maps (3, 9) float64, origin (x0, y0), canvas shape (Hc, Wc)): a pan of 4 px per frame seen
    from a canvas three pixels larger on every side, under a half-pixel translation or a mild homography on top of the pan.
    behind: frame 1's nine coefficients negated -- its source positions stay inside the frame and its divisor is negative,
    so it covers nothing and none of its holes may reach the canvas"""
    import mosaic_model as MM

    F, H, W, m = MOSAIC["F"], MOSAIC["H"], MOSAIC["W"], MOSAIC["margin"]
    frames, maps = MM.pan_frames(MM.smooth_field(H + 8, W + 4 * (F - 1) + 8, 5), F, H, W, 4, 0, 4, 4)
    maps = maps.copy()
    maps[:, 2] += 4.5
    maps[:, 5] += 4.5
    if projective:
        maps[:, 1], maps[:, 3] = 0.01, -0.02
        maps[:, 6], maps[:, 7] = 3e-4, -2e-4
    if behind:
        maps[1] = -maps[1]
    return frames_of(scene, frames.astype(np.float32)), maps, (-m, -m), (H + 2 * m, W + 4 * (F - 1) + 2 * m)


EXPOSURES = np.array([[1.0, 0.0], [1.1, -3.0], [0.9, 1e30]], np.float64)


# ---- alignment -------------------------------------------------------------------------------------------------------
def align_pair(scene: str, H, W, kind, seed=None):
    """(a, b (1, H, W) float32, model (1, nc) float32) of align_model.planted_pair under the scene: the planted map pushed by
    half a pixel at the corners"""
    import align_model as AM

    A, B, planted = AM.planted_pair(H, W, H + W if seed is None else seed, kind, move=2.0)
    return transform(scene, A, True)[None], transform(scene, B, False)[None], AM.pushed(planted, H, W, kind, 0.5)[None]


def holes_unsampled(H, W, kind, holes: bool = True):
    """(a, b (1, H, W) float32, model (1, nc) float32) for levels = 1: b is a seen 10 px further left, the model a shift of
    9.6 px in x, so that columns 0 .. 8 of b are never a tap; NaN and +inf go into those columns of b, and a NaN into a at a
    pixel whose sample, and those of its eight neighbours, leave b.  holes=False: the same pair without them."""
    import align_model as AM

    wide = AM.view(AM.texture(H, W + 10, 21), H, W + 10, AM.IDENTITY[AM.HOMOGRAPHY])
    a, b = np.ascontiguousarray(wide[:, 10:]), np.ascontiguousarray(wide[:, :W])
    model = AM.IDENTITY[kind].copy()
    model[2] = 9.6
    if holes:
        b[H // 2, 3] = np.nan
        b[0, 0] = np.inf
        b[H - 1, 7] = np.nan
        b[H // 3, 8] = np.inf
        a[H // 2, W - 3] = np.nan
    return a[None], b[None], model[None]
