"""The statement of NV12 video (include/oflk.h repeats it): what oflk_warp_affine_nv12, oflk_warp_perspective_nv12,
oflk_stabilize_sequence_nv12 and a stabiliser made by oflk_stabilizer_create_nv12 return, byte for byte.  Plain NumPy, built
on stabilize_model.warp and homography_model.warp; no library call.

Layout.  An NV12 frame is H W 3 / 2 bytes: Y[H][W] first, then UV[H/2][W/2][2] with U at byte 0 and V at byte 1.  H and W are
even and at least 4.  Frames are contiguous, [F][H W 3 / 2]; here they are (F, 3H/2, W) uint8 arrays, the same bytes.
Pitched surfaces and separate plane pointers are not offered.

Siting.  Chroma sample (column i, row j) sits at luma x = 2 i + sx, y = 2 j + sy.  "left" (OFLK_SITING_LEFT = 0) means
(sx, sy) = (0, 0.5), the H.264 / HEVC default; "center" (OFLK_SITING_CENTER = 1) means (0.5, 0.5), as in JPEG and MPEG-1.

The chroma map.  float64, each operation rounded on its own, in this order:
    c2 = (m0 sx + m1 sy) + m2,  c5 = (m3 sx + m4 sy) + m5,  perspective only: c8 = (m6 sx + m7 sy) + m8
    affine:      mc = [m0, m1, 0.5 (c2 - sx);  m3, m4, 0.5 (c5 - sy)]
    perspective: mc = [m0 - sx m6, m1 - sx m7, 0.5 (c2 - sx c8);  m3 - sy m6, m4 - sy m7, 0.5 (c5 - sy c8);  2 m6, 2 m7, c8]
This is the luma map conjugated by the siting: a chroma sample is fetched from where its own luma position is fetched from.

The warp.  The Y plane of out[f] is the bytes the planar u8 warp writes for Y[f] under map[f], and inside[f] (H, W) is that
call's inside.  U and V of out[f] are, per channel, the bytes the same planar warp writes for the H/2 x W/2 plane
UV[f][:, :, c] under mc, and where that warp's own inside is 0 the chroma byte is 128, not 0: zero chroma is saturated green,
Y = 0 with U = V = 128 is black.  Nothing else differs from the planar statement.

NV12 stabilisation, by statement, byte for byte: (1) oflk_stabilize_sequence_u8 on the Y planes for correction, model_out,
counts_out and held; (2) the NV12 affine warp of the frames under the maps of that trajectory.  The online form: the frames
and corrections of T pushes and a flush equal the NV12 sequence call on the same T frames.
"""
import numpy as np

import homography_model as HM
import stabilize_model as SM

SITINGS = {"left": (0.0, 0.5), "center": (0.5, 0.5)}
SITING_CODES = {"left": 0, "center": 1}
FILL = 128   # the chroma byte where the chroma plane's own warp is outside


def planes(frames):
    """(F, 3H/2, W) uint8 -> views y (F, H, W), uv (F, H/2, W/2, 2)"""
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[1] % 3 == 0
    F, R, W = f.shape
    H = 2 * R // 3
    assert H % 2 == 0 and W % 2 == 0 and H >= 4 and W >= 4
    return f[:, :H, :], f[:, H:, :].reshape(F, H // 2, W // 2, 2)


def from_planes(y, uv):
    """y (F, H, W), uv (F, H/2, W/2, 2) uint8 -> (F, 3H/2, W)"""
    F, H, W = y.shape
    assert uv.shape == (F, H // 2, W // 2, 2)
    return np.ascontiguousarray(np.concatenate([y, uv.reshape(F, H // 2, W)], axis=1))


def chroma_map(m, siting="left"):
    """one luma map, (6,) or (9,) float64 -> the map of the chroma plane, same length"""
    m = np.asarray(m, np.float64).reshape(-1)
    sx, sy = (np.float64(s) for s in SITINGS[siting])
    with np.errstate(all="ignore"):
        c2 = (m[0] * sx + m[1] * sy) + m[2]
        c5 = (m[3] * sx + m[4] * sy) + m[5]
        if m.size == 6:
            return np.array([m[0], m[1], 0.5 * (c2 - sx), m[3], m[4], 0.5 * (c5 - sy)])
        assert m.size == 9
        c8 = (m[6] * sx + m[7] * sy) + m[8]
        return np.array([m[0] - sx * m[6], m[1] - sx * m[7], 0.5 * (c2 - sx * c8),
                         m[3] - sy * m[6], m[4] - sy * m[7], 0.5 * (c5 - sy * c8),
                         2.0 * m[6], 2.0 * m[7], c8])


def chroma_maps(maps, siting="left"):
    maps = np.asarray(maps, np.float64)
    return np.stack([chroma_map(m, siting) for m in maps.reshape(len(maps), -1)])


def _warp(planar, frames, maps, siting):
    y, uv = planes(frames)
    out_y, inside = planar(y, maps)
    mc = chroma_maps(maps, siting)
    ch = []
    for c in range(2):
        o, ins = planar(np.ascontiguousarray(uv[..., c]), mc)
        ch.append(np.where(ins != 0, o, np.uint8(FILL)).astype(np.uint8))
    return from_planes(out_y, np.stack(ch, axis=-1)), inside


def warp_affine(frames, maps, siting="left"):
    """frames (F, 3H/2, W) uint8, maps (F, 6) float64 -> (out like frames, inside (F, H, W) uint8)"""
    return _warp(SM.warp, frames, np.asarray(maps, np.float64).reshape(len(frames), 6), siting)


def warp_perspective(frames, maps, siting="left"):
    """frames (F, 3H/2, W) uint8, maps (F, 9) float64 -> (out like frames, inside (F, H, W) uint8)"""
    return _warp(HM.warp, frames, np.asarray(maps, np.float64).reshape(len(frames), 9), siting)


def stabilize(frames, siting, K, D, q, md, family, hyps, thr, seed, w, **kw):
    """the chain of statements on NV12 frames (T, 3H/2, W): returns (out, correction, model, counts, held)"""
    grey = np.ascontiguousarray(planes(frames)[0])
    _, corr, model, counts, held = SM.sequence(grey, K, D, q, md, family, hyps, thr, seed, w, **kw)
    mp = SM.trajectory(model, counts, len(grey), w)[1]
    return warp_affine(frames, mp, siting)[0], corr, model, counts, held


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
CHROMA_GAINS = ((0.6, 60), (0.75, 20))   # (gain, offset) of U and V: the two differ from each other and from Y


def from_grey(grey):
    """grey uint8 frames (F, H, W) as NV12 frames: Y is the frames, U and V are grey[:, ::2, ::2] under two gains and offsets"""
    g = np.asarray(grey)
    sub = g[:, ::2, ::2].astype(np.float64)
    uv = np.stack([np.rint(a * sub + b) for a, b in CHROMA_GAINS], axis=-1)
    assert uv.min() >= 0 and uv.max() <= 255
    return from_planes(np.ascontiguousarray(g), uv.astype(np.uint8))


def random_frames(F, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, 3 * H // 2, W), dtype=np.uint8)


def rotation(H, W, degrees, scale):
    """the 2 x 3 map of a rotation about the frame's centre with a scale: (6,) float64"""
    a = np.deg2rad(degrees)
    c, s = scale * np.cos(a), scale * np.sin(a)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy])


def affine_maps(H, W):
    """named pairs of 2 x 3 maps, (2, 6) float64: a different map for each of F = 2 frames"""
    return {
        "rotation with scale": np.stack([rotation(H, W, 7.0, 1.1), rotation(H, W, -11.0, 0.9)]),
        "shear, sub-pixel translation": np.array([[1.0, 0.2, 0.3, 0.05, 1.0, -0.7], [1.0, -0.15, 1.25, 0.1, 0.95, 0.4]]),
        "mostly outside": np.array([[1.0, 0.0, 0.75 * W, 0.0, 1.0, 0.6 * H], [1.0, 0.0, -0.8 * W + 0.5, 0.0, 1.0, -0.5]]),
    }


def as_homography(m6):
    m6 = np.asarray(m6, np.float64)
    return np.concatenate([m6, np.broadcast_to([0.0, 0.0, 1.0], m6.shape[:-1] + (3,))], axis=-1)


def perspective_maps(H, W):
    """named pairs of 3 x 3 maps, (2, 9) float64: the affine ones under a projective third row each"""
    rows = np.array([[2e-3 / W, -1e-3 / H, 1.0], [-1.5e-3 / W, 2e-3 / H, 1.02]])
    return {k: np.concatenate([v, rows], axis=-1) for k, v in affine_maps(H, W).items()}
