"""The statement of colour video (include/oflk.h repeats it): what oflk_luma_u8, oflk_warp_affine_packed,
oflk_warp_perspective_packed, oflk_stabilize_sequence_packed and a stabiliser made by oflk_stabilizer_create_packed return,
byte for byte.  Plain NumPy, no library call.

Layout.  Colour frames are interleaved uint8, [F][H][W][C] with C = 3 or 4 ("packed").  float32 colour is not offered.
`order` says where R, G and B sit: "rgb" (OFLK_ORDER_RGB = 0) means R, G, B at bytes 0, 1, 2; "bgr" (OFLK_ORDER_BGR = 1)
means B, G, R.  The byte at index 3 when C = 4 is a fourth channel: luma ignores it, every warp resamples it like the others.

Luma.  Y = (77 R + 150 G + 29 B + 128) >> 8 in integers.  The weights sum to 256, so grey input (R = G = B = g) gives
(256 g + 128) >> 8 = g, and Y <= (256 * 255 + 128) >> 8 = 255: Y never leaves [0, 255].  There is no float arithmetic and
nothing to round.

Packed warps.  For every channel c, out[f][y][x][c] is the byte that oflk_warp_affine / oflk_warp_perspective writes at
[f][y][x] for the plane frames[f][:, :, c] under map[f]: (unsigned char) rintf(sample), 0 outside the frame.
inside[f][y][x] is that call's inside: one byte per pixel, not per channel.  The model is therefore stabilize_model.warp /
homography_model.warp applied per plane and stacked.

Colour stabilisation, by statement, byte for byte: (1) the luma of every frame; (2) oflk_stabilize_sequence_u8 on the luma
frames for correction, model_out, counts_out and held; (3) the packed affine warp of the colour frames under the maps of
that trajectory.  The online form: the frames and corrections of T pushes and a flush equal the offline colour call on the
same T frames.
"""
import numpy as np

import homography_model as HM
import stabilize_model as SM

ORDERS = {"rgb": 0, "bgr": 1}
CHANNELS = (3, 4)
WEIGHTS = (77, 150, 29)   # of R, G, B; they sum to 256


def luma(frames, order="rgb"):
    """frames (..., C) uint8, C = 3 or 4 -> (...) uint8"""
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.shape[-1] in CHANNELS and order in ORDERS
    r, g, b = (f[..., 0], f[..., 1], f[..., 2]) if order == "rgb" else (f[..., 2], f[..., 1], f[..., 0])
    y = (77 * r.astype(np.int64) + 150 * g.astype(np.int64) + 29 * b.astype(np.int64) + 128) >> 8
    return y.astype(np.uint8)


def _per_plane(warp, frames, maps):
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] in CHANNELS
    planes = [warp(frames[..., c], maps) for c in range(frames.shape[-1])]
    return np.stack([p[0] for p in planes], axis=-1), planes[0][1]


def warp_affine(frames, maps):
    """frames (F, H, W, C) uint8, maps (F, 6) float64 -> (out like frames, inside (F, H, W) uint8)"""
    return _per_plane(SM.warp, frames, maps)


def warp_perspective(frames, maps):
    """frames (F, H, W, C) uint8, maps (F, 9) float64 -> (out like frames, inside (F, H, W) uint8)"""
    return _per_plane(HM.warp, frames, maps)


def stabilize(frames, order, K, D, q, md, family, hyps, thr, seed, w, **kw):
    """the chain of statements on colour frames (T, H, W, C): returns (out, correction, model, counts, held)"""
    grey = luma(frames, order)
    _, corr, model, counts, held = SM.sequence(grey, K, D, q, md, family, hyps, thr, seed, w, **kw)
    mp = SM.trajectory(model, counts, len(grey), w)[1]
    return warp_affine(frames, mp)[0], corr, model, counts, held


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
GAINS = ((0.9, 10), (0.6, 60), (0.75, 0), (0.5, 100))   # (gain, offset) of channel c: every plane differs from every other


def coloured(grey, channels, order="rgb"):
    """grey uint8 frames (..., H, W) as colour frames (..., H, W, channels): plane c is rint(gain_c grey + offset_c), so the
    planes differ and the luma is none of them.  `order` only names the planes: plane 0 is R for "rgb" and B for "bgr"."""
    g = np.asarray(grey).astype(np.float64)
    out = np.stack([np.rint(GAINS[c][0] * g + GAINS[c][1]) for c in range(channels)], axis=-1)
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8))


def random_frames(F, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W, C), dtype=np.uint8)


def rotation(H, W, degrees, scale):
    """the 2 x 3 map of a rotation about the frame's centre with a scale: (6,) float64"""
    a = np.deg2rad(degrees)
    c, s = scale * np.cos(a), scale * np.sin(a)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy])


def affine_maps(H, W):
    """named 2 x 3 maps, (6,) float64 each: what the packed affine warp is tested under"""
    return {
        "identity": np.array([1.0, 0, 0, 0, 1, 0]),
        "integer shift": np.array([1.0, 0, 1, 0, 1, -1]),
        "half-pixel shift": np.array([1.0, 0, 0.5, 0, 1, 0.5]),
        "rotation 7 deg, scale 1.1": rotation(H, W, 7.0, 1.1),
        "all outside": np.array([1.0, 0, 4.0 * W, 0, 1, 0]),
        "NaN coefficient": np.array([1.0, np.nan, 0, 0, 1, 0]),
    }


def as_homography(m6):
    return np.concatenate([np.asarray(m6, np.float64), [0.0, 0.0, 1.0]])


def perspective_maps(H, W):
    """named 3 x 3 maps, (9,) float64 each: the affine ones with the third row (0, 0, 1), a mild homography, and one whose w
    changes sign inside the frame (w = 1 - 2 x / (W - 1): positive on the left half, zero or negative on the right)"""
    maps = {f"affine: {k}": as_homography(v) for k, v in affine_maps(H, W).items()}
    maps["mild homography"] = np.array([1.02, 0.01, -0.3, -0.015, 0.99, 0.4, 2e-3 / W, -1e-3 / H, 1.0])
    maps["w changes sign"] = np.array([1.0, 0, 0, 0, 1, 0, -2.0 / (W - 1), 0, 1.0])
    return maps
