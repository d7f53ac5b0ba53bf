"""The statement of the median filter of dense flows (oflk_flow_median, its host form and the flow_median setting of the
sequence calls) in NumPy.

Test infrastructure: the product never imports this file.  The kernel (k_flow_median, csrc/oflk_flowmedian.hpp) is held to it
byte for byte, a NaN equal to a NaN.

The window is size x size, size in {3, 5, 7, 9}, r = size // 2.  A plane p is (H, W) float32.  Output pixel (y, x)
1. takes the size^2 values p[clamp(y + j, 0, H-1), clamp(x + i, 0, W-1)], i, j in -r .. r: the border is replicated;
2. orders them by mosaic_median_model.key: -NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN, taken on the bits;
3. returns the value of rank size^2 // 2.
size^2 is odd, so the result is always one of the inputs: nothing is averaged and nothing is rounded.  Equal keys are equal
bytes, so the selection method cannot show in the result.  Every plane is filtered on its own: of a flow this is the
component-wise median of u and of v, not a vector median.
"""
import numpy as np

from mosaic_median_model import key, unkey

SIZES = (3, 5, 7, 9)


def window_keys(p, size):
    """(size^2, H, W) uint32: the keys of every pixel's window, row by row"""
    assert size in SIZES
    p = np.ascontiguousarray(p, np.float32)
    assert p.ndim == 2
    H, W = p.shape
    r = size // 2
    k = key(p)
    ys, xs = np.arange(H), np.arange(W)
    return np.stack([k[np.clip(ys + j, 0, H - 1)][:, np.clip(xs + i, 0, W - 1)] for j in range(-r, r + 1) for i in range(-r, r + 1)])


def median_plane(p, size):
    """the statement on one (H, W) plane: float32 (H, W)"""
    k = window_keys(p, size)
    k.sort(axis=0)
    return unkey(k[size * size // 2])


def median(planes, size):
    """the statement on every plane of a float32 array (..., H, W): the same shape"""
    a = np.ascontiguousarray(planes, np.float32)
    flat = a.reshape((-1,) + a.shape[-2:])
    return np.stack([median_plane(p, size) for p in flat]).reshape(a.shape)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000],
                    np.uint32).view(np.float32)   # +NaN, -NaN, two more NaNs of either sign, +inf, -inf, +0, -0


def special_planes(P, H, W, seed, share=0.3):
    """(P, H, W) float32: small values of both signs with `share` of the pixels one of SPECIALS, every one of them present when
    the planes have room, dense enough for windows whose middle is a special value"""
    rng = np.random.default_rng(seed)
    a = ((rng.random((P, H, W)) * 2 - 1) * 3).astype(np.float32)
    n = a.size
    idx = rng.permutation(n)[:max(min(n, len(SPECIALS)), int(share * n))]
    a.reshape(-1)[idx] = SPECIALS[np.arange(len(idx)) % len(SPECIALS)]
    return a


def quantised_planes(P, H, W, seed, levels=4):
    """(P, H, W) float32 of `levels` distinct values: heavy ties"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (P, H, W)).astype(np.float32) - np.float32(1.5)) * np.float32(0.75)
