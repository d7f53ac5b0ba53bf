"""Scenes of the colour and NV12 interpolation tests (test infrastructure): a colour pan with a known middle frame and its
NV12 form."""
import numpy as np

import interp_model as M
import nv12_model as NM


def colour_pan(dx, dy, H=96, W=128):
    """(A, middle, B) float32 (H, W, 3): three interp_model.pan_scene textures (seeds 0, 1, 2) as R, G, B under one pan"""
    per = [M.pan_scene(dx, dy, H, W, seed=s) for s in range(3)]
    return tuple(np.stack([per[c][k] for c in range(3)], axis=-1) for k in range(3))


def bt601(rgb):
    """float (…, H, W, 3) RGB in [0, 255] -> (Y (…, H, W), U, V (…, H/2, W/2)) float64, BT.601 limited range, the chroma
    box-averaged over its 2 x 2 luma pixels"""
    r, g, b = (np.asarray(rgb, np.float64)[..., c] for c in range(3))
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0

    def box(p):
        s = p.shape
        return p.reshape(s[:-2] + (s[-2] // 2, 2, s[-1] // 2, 2)).mean(axis=(-3, -1))

    return y, box(u), box(v)


def to_nv12(rgb):
    """float (F, H, W, 3) RGB -> (NV12 frames (F, 3H/2, W) uint8, the unrounded (Y, U, V) of bt601)"""
    y, u, v = bt601(rgb)
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    return NM.from_planes(q(y), np.stack([q(u), q(v)], axis=-1)), (y, u, v)
