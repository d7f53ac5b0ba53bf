"""The statement of the exposure chain and the exposure-compensated mosaic (oflk_exposure_chain_host,
oflk_mosaic_accumulate_exposure and the composite calls made of it) in NumPy.

Test infrastructure: the product never imports this file.  The code (csrc/oflk_mosaic.hpp, csrc/oflk.hip) is held to it byte for
byte, a NaN equal to a NaN.  Every operation is float64 and rounded on its own.

1. The chain (`exposure_chain`).  photo [T-1][2] float32: step t's (g_t, b_t) of the photometric alignment, "frame t + 1 looks
   like g_t frame t + b_t"; status [T-1] or None; an anchor in [0, T-1].  The float32 values are widened first.  A step is
   held, that is taken as (1, 0), when its status is 0, when g or b is not finite, or when g <= 0.  (eg_f, eb_f) takes frame
   f's values to the anchor's exposure, v_anchor = eg_f v_f + eb_f:
       E_anchor = (1, 0)
       forwards, t = anchor .. T-2:     eg_{t+1} = eg_t / g_t;      eb_{t+1} = eb_t - eg_{t+1} b_t
       backwards, t = anchor-1 .. 0:    eg_t = eg_{t+1} g_t;        eb_t = eg_{t+1} b_t + eb_{t+1}
2. Accumulation (`accumulate`): mosaic_model.accumulate with one change: the float32 sample s of frame f enters the blend as
   eg_f * f64(s) + eb_f, one multiply and one add, each rounded.  The cull, the four blends, the counts and the resolve are
   mosaic_model's.
"""
import numpy as np

import mosaic_model as MM
from track_model import sample as bilinear


def exposure_chain(photo, status, T, anchor):
    """-> (T, 2) float64 (eg, eb)"""
    assert T >= 1 and 0 <= anchor < T
    p = np.asarray(photo, np.float32).reshape(T - 1, 2).astype(np.float64)
    steps = []
    for t in range(T - 1):
        g, b = p[t]
        held = (status is not None and status[t] == 0) or not (np.isfinite(g) and np.isfinite(b)) or not g > 0
        steps.append((np.float64(1.0), np.float64(0.0)) if held else (g, b))
    E = np.zeros((T, 2))
    E[anchor] = (1.0, 0.0)
    with np.errstate(all="ignore"):
        for t in range(anchor, T - 1):
            g, b = steps[t]
            eg = E[t, 0] / g
            E[t + 1] = (eg, E[t, 1] - eg * b)
        for t in range(anchor - 1, -1, -1):
            g, b = steps[t]
            eg = E[t + 1, 0]
            E[t] = (eg * g, eg * b + E[t + 1, 1])
    return E


def accumulate(state, frames, maps, skip, exposure, x0, y0, blend):
    """adds the F frames, each taken to the anchor's exposure, to the state, in place; returns it"""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    maps = np.asarray(maps, np.float64).reshape(F, 9)
    exposure = np.asarray(exposure, np.float64).reshape(F, 2)
    S, Ws, C = state["sum"], state["wsum"], state["count"]
    Hc, Wc = S.shape
    for f in range(F):
        if skip is not None and skip[f]:
            continue
        xs, ys, w = MM.coordinates(maps[f], x0, y0, Hc, Wc)
        with np.errstate(invalid="ignore"):
            ins = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        if not ins.any():
            continue
        with np.errstate(all="ignore"):
            s = exposure[f, 0] * bilinear(frames[f].astype(np.float32), xs[ins], ys[ins]).astype(np.float64) + exposure[f, 1]
            if blend == MM.MEAN:
                S[ins] = S[ins] + s
                Ws[ins] = Ws[ins] + 1.0
            elif blend == MM.FEATHER:
                g = np.minimum(np.minimum(xs[ins], (W - 1.0) - xs[ins]), np.minimum(ys[ins], (H - 1.0) - ys[ins])) + 1.0
                S[ins] = S[ins] + g * s
                Ws[ins] = Ws[ins] + g
            elif blend == MM.FIRST:
                new = C[ins] == 0
                S[ins] = np.where(new, s, S[ins])
                Ws[ins] = np.where(new, 1.0, Ws[ins])
            elif blend == MM.LAST:
                S[ins] = s
                Ws[ins] = 1.0
            else:
                raise ValueError(blend)
        C[ins] = C[ins] + 1
    return state


def composite(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend, cuts=()):
    """accumulate (cut into calls at the frame indices `cuts`) and resolve: (out, count)"""
    frames = np.asarray(frames)
    F = frames.shape[0]
    maps = np.asarray(maps, np.float64).reshape(F, 9)
    exposure = np.asarray(exposure, np.float64).reshape(F, 2)
    st = MM.empty_state(Hc, Wc)
    edges = [0, *cuts, F]
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi > lo:
            accumulate(st, frames[lo:hi], maps[lo:hi], None if skip is None else skip[lo:hi], exposure[lo:hi], x0, y0, blend)
    return MM.resolve(st, frames.dtype == np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def source_error(canvas, count, origin, truth, at):
    """(mean, largest) absolute difference between a canvas and `truth` (the source at the anchor's exposure) over the pixels
    that a frame reaches; canvas pixel (0, 0) + origin is the anchor's pixel, which lies at `at` = (x, y) of the source"""
    Hc, Wc = canvas.shape
    x0, y0 = at[0] + origin[0], at[1] + origin[1]
    ys, xs = np.mgrid[:Hc, :Wc]
    ok = (count > 0) & (ys + y0 >= 0) & (ys + y0 < truth.shape[0]) & (xs + x0 >= 0) & (xs + x0 < truth.shape[1])
    d = np.abs(canvas[ok].astype(np.float64) - truth[ys[ok] + y0, xs[ok] + x0])
    return float(d.mean()), float(d.max())
