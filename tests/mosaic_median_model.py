"""The statement of the temporal-median mosaic (oflk_mosaic_median and its host forms) in NumPy.

Test infrastructure: the product never imports this file.  The kernel (k_mosaic_median, csrc/oflk_mosaic.hpp) is held to it
byte for byte, a NaN equal to a NaN.

Canvas pixel coordinates, w, xs, ys, inside and the float32 bilinear sample s of frame f are mosaic_model.accumulate's
(mosaic_model.coordinates, track_model.sample).  Frames with skip[f] != 0 take no part.

1. The value that enters.  e = s.  With an exposure, e = f32(eg_f * f64(s) + eb_f): the product is rounded, then the sum, then
   the result is rounded to float32.
2. The order (`key`).  Ascending by the uint32 key of e's bits b: key = ~b when the sign bit is set, else b ^ 0x80000000.  That
   gives -NaN < -inf < negatives < -0 < +0 < positives < +inf < +NaN.  Equal keys are equal bytes, so ties cannot show, and the
   result does not depend on the frame order, on the selection method or on the launch geometry.
3. The value (`median`).  n is the number of covering frames and e_(0) <= ... <= e_(n-1).  n odd: v = e_((n-1)/2).  n even:
   v = f32((f64(e_(n/2-1)) + f64(e_(n/2))) * 0.5), so inf + -inf is a NaN.  n == 0: 0.
4. The store.  float32 frames store v; uint8 frames store mosaic_model.saturate(v).  count = n.

The sign of a NaN that an operation makes of other values (inf * 0 inside the bilinear sample, where an infinite tap has the
weight 0; inf - inf) is the processor's own: x86 sets the sign bit, gfx950 does not.  A NaN that enters with a frame or with an
exposure keeps its sign through every operation that has no second NaN operand.  The tests therefore plant NaNs and
infinities at pixel (0, 0) of a frame, which is only ever the first tap of a sample and has a positive weight there.
"""
import numpy as np

import mosaic_model as MM
from track_model import sample as bilinear


def key(e):
    """the uint32 sort keys of float32 values"""
    b = np.ascontiguousarray(e, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    """the float32 values of uint32 sort keys"""
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def select(e):
    """the statement's value of the float32 samples e (1-D, any order): float32"""
    e = np.ascontiguousarray(e, np.float32).reshape(-1)
    n = e.size
    if n == 0:
        return np.float32(0)
    s = unkey(np.sort(key(e)))
    if n & 1:
        return s[(n - 1) // 2]
    with np.errstate(all="ignore"):
        return np.float32((np.float64(s[n // 2 - 1]) + np.float64(s[n // 2])) * 0.5)


def samples(frames, maps, skip, exposure, x0, y0, Hc, Wc):
    """(e (F, Hc, Wc) float32, inside (F, Hc, Wc) bool): what every frame offers every canvas pixel"""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    maps = np.asarray(maps, np.float64).reshape(F, 9)
    e = np.zeros((F, Hc, Wc), np.float32)
    inside = np.zeros((F, Hc, Wc), bool)
    for f in range(F):
        if skip is not None and skip[f]:
            continue
        xs, ys, w = MM.coordinates(maps[f], x0, y0, Hc, Wc)
        with np.errstate(invalid="ignore"):
            ins = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        if not ins.any():
            continue
        with np.errstate(all="ignore"):
            s = bilinear(frames[f].astype(np.float32), xs[ins], ys[ins])
            if exposure is not None:
                eg, eb = np.asarray(exposure, np.float64).reshape(F, 2)[f]
                s = (eg * s.astype(np.float64) + eb).astype(np.float32)
        e[f][ins] = s
        inside[f] = ins
    return e, inside


def median(frames, maps, skip, x0, y0, Hc, Wc, exposure=None):
    """-> (out (Hc, Wc) float32 or uint8, count (Hc, Wc) int32)"""
    frames = np.asarray(frames)
    e, inside = samples(frames, maps, skip, exposure, x0, y0, Hc, Wc)
    count = inside.sum(0).astype(np.int32)
    # keys of the frames that do not cover a pixel sort last (as uint64 above every uint32), so the first n of a column are its own
    k = np.where(inside, key(e).astype(np.uint64), np.uint64(1) << np.uint64(32))
    k.sort(axis=0)
    F = k.shape[0]
    lo = np.clip((count - 1) // 2, 0, F - 1)[None]
    hi = np.clip(count // 2, 0, F - 1)[None]
    e_lo = unkey(np.take_along_axis(k, lo, 0)[0].astype(np.uint32))
    e_hi = unkey(np.take_along_axis(k, hi, 0)[0].astype(np.uint32))
    with np.errstate(all="ignore"):
        mid = ((e_lo.astype(np.float64) + e_hi.astype(np.float64)) * 0.5).astype(np.float32)
    v = np.where(count == 0, np.float32(0), np.where(count & 1, e_lo, mid)).astype(np.float32)
    return (MM.saturate(v) if frames.dtype == np.uint8 else v), count


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def mover_scene(F=16, H=48, W=64, dx=6, image_shape=(56, 168), step=(5, 1), start=(4, 10), patch=(16, 20)):
    """a pan over smooth_field(image_shape, 3) with an object of its own pasted into every frame: the patch 255 -
    smooth_field(patch, 9) at column start[0] + step[0] f, row start[1] + step[1] f of frame f, wherever it fits, which in image
    coordinates moves by dx + step[0] pixels a frame.  -> (image, frames (F, H, W) uint8, maps (F, 9))"""
    img = MM.smooth_field(image_shape[0], image_shape[1], 3)
    frames, maps = MM.pan_frames(img, F, H, W, dx)
    frames = frames.copy()
    obj = (255 - MM.smooth_field(patch[0], patch[1], 9)).astype(np.uint8)
    for f in range(F):
        c, r = start[0] + step[0] * f, start[1] + step[1] * f
        if c + patch[1] <= W and r + patch[0] <= H:
            frames[f, r:r + patch[0], c:c + patch[1]] = obj
    return img, frames, maps
