"""Scenes for the uint8 outputs at and beyond the byte range (test infrastructure; plain NumPy, nothing here touches the GPU).

The mosaic's resolve is the one place where a value outside [0, 255] reaches a uint8 store: an exposure takes a sample anywhere
and a state accumulated from float32 frames can be resolved to bytes.  Its rule (mosaic_model.saturate): 0 for a NaN, otherwise
rint, half to even, held to [0, 255].  The shapes are the smallest mosaic cases of tests/test_gpu_mosaic_exposure.py:

    CASES[0]   frames 9 x 13 on a 19 x 68 canvas at (-7, 3): the row length is a multiple of 4 (a lane stores a dword)
    CASES[1]   frames 17 x 40 on a 21 x 71 canvas at (5, -4): it is not (byte stores)

    ladder         one constant frame of 100 per target under the exposure (1, target - 100), every frame moved by an integer
                   translation to a band of its own, so every planted value is exact; `last`, and `first` on the reversed order
    wide           test_gpu_mosaic_exposure._scene with frames over 0 .. 255, gains in [0.6, 1.5] and biases in [-40, 40]
    float_state    the x257 and the signed float32 frames of range_feature_scenes.mosaic_scene, accumulated plain and resolved
                   to bytes, on that scene's canvas (42 wide) and on one two columns wider (44: the dword store)
    extremes       uint8 frames of 0, of 255, a 0 / 255 checkerboard and 254 / 255 stripes for the calls that keep the bare
                   conversion (unsigned char)rintf(v): the warps, interpolate_frames and the plain mosaic
    highlight_pan  align_photo_model.pan_scene with the source left at 0 .. 255 and the planted exposures handed over, the
                   anchor the last frame: every earlier frame has eg > 1 and highlights go above 255
"""
from __future__ import annotations

import numpy as np

import mosaic_exposure_model as MEM
import mosaic_model as MM

# frame, canvas, origin, frames of `wide`, the first column of the ladder's bands
CASES = [((9, 13), (19, 68), (-7, 3), 6, 0), ((17, 40), (21, 71), (5, -4), 7, 4)]

INF, NAN = float("inf"), float("nan")
TARGETS = [-1e30, -300.0, -256.5, -1.0, -0.5, -0.25, 0.0, 0.5, 1.5, 254.5, 255.0,
           255.25, 255.5, 256.0, 300.0, 511.5, 512.0, 65535.0, 1e30, INF, -INF, NAN]
# what the rule gives for each target
RULE = [0, 0, 0, 0, 0, 0, 0, 0, 2, 254, 255,
        255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 0]
# the targets are laid out in two strips of eleven bands; a band is as wide as the step to the next frame of its strip.  The
# upper strip's bands are four columns each and start at a multiple of 4: a lane's four pixels hold one target.  The lower
# strip starts with a band of six, so that the bands of 255.5 and 300 (and 256) lie across two lanes each, two pixels in each
STRIP = 11
WIDTHS = [[4] * 10, [6, 4, 4, 4, 2, 4, 4, 4, 4, 4]]


def ladder(case, blend):
    """-> (frames (22, H, W) uint8, maps (22, 9), exposure (22, 2), blend code, band (Hc, Wc) int: the index of the target that
    a canvas pixel shows, -1 where no frame reaches).  blend: "last", or "first" with the frames in reverse order"""
    (H, W), (Hc, Wc), (x0, y0), _, start = CASES[case]
    split = (Hc + 1) // 2 if Hc < 2 * H else H   # the first row of the lower strip
    n = len(TARGETS)
    maps, place = [], []
    for k in range(n):
        s, j = divmod(k, STRIP)
        cx = start + sum(WIDTHS[s][:j])
        cy = split - H if s == 0 else split      # the upper strip's frames end on row split - 1, the lower one's begin below
        place.append((cx, cy))
        maps.append(MM.translation(-(x0 + cx), -(y0 + cy)))
    band = np.full((Hc, Wc), -1, np.int64)
    for k, (cx, cy) in enumerate(place):         # in frame order: the last frame wins
        band[max(cy, 0):max(min(cy + H, Hc), 0), max(cx, 0):max(min(cx + W, Wc), 0)] = k
    frames = np.full((n, H, W), 100, np.uint8)
    exposure = np.array([[1.0, t - 100.0] for t in TARGETS], np.float64)
    maps = np.stack(maps)
    if blend == "first":
        return frames, maps[::-1].copy(), exposure[::-1].copy(), MM.FIRST, band
    assert blend == "last"
    return frames, maps, exposure, MM.LAST, band


def wide(case, dtype=np.uint8, seed=None):
    """-> (frames, maps, skip, exposure): a perspective frame, a culled frame and a skipped frame among sub-pixel translations.

    The frames are not that scene's white noise: a mean of independent uniform samples concentrates, and no seed of 300 took
    more than 1.4 % of the covered pixels below -0.5.  They show one picture instead, as the frames of a mosaic do: dark
    (0 .. 31) over the left quarter of the panned width, bright (224 .. 255) over the right quarter and a ramp between, each
    frame cut at its own translation (the perspective frame at the first frame's), under noise of 12 % of the range"""
    (H, W), (Hc, Wc), (x0, y0), F, _ = CASES[case]
    rng = np.random.default_rng(WIDE_SEEDS[case] if seed is None else seed)
    off = 3.37 * np.arange(F)
    off[F // 2] = 0.0
    X = (np.arange(W)[None, :] + off[:, None]) / (W - 1 + 3.37 * (F - 2))
    f = 255.0 * (0.88 * np.clip(2.0 * X - 0.5, 0.0, 1.0)[:, None, :] + 0.12 * rng.random((F, H, W)))
    frames = np.rint(f).astype(np.uint8) if dtype == np.uint8 else f.astype(np.float32)
    maps = np.stack([MM.translation(-(x0 - 2.25 + 3.37 * k), -(y0 - 1.5 + 1.21 * k)) for k in range(F)])
    maps[F // 2] = [0.9, 0.05, -0.9 * x0 + 1, -0.04, 1.1, -1.1 * y0 + 2, 1e-3, -1e-3, 1.0]   # a perspective frame
    maps[F - 1] = MM.translation(1e6, -3e5)                                                  # a frame that is culled
    skip = np.zeros(F, np.uint8)
    skip[1] = 1
    exposure = np.stack([rng.uniform(0.6, 1.5, F), rng.uniform(-40, 40, F)], 1)
    return frames, maps, skip, exposure


WIDE_SEEDS = (7, 13)   # test_byte_range_cpu holds them to what the scene claims: 5 % of the covered pixels beyond either end

FLOAT_STATES = [(name, projective, extra) for name in ("u16", "signed") for projective, extra in ((False, 0), (True, 2))]


def float_state(name, projective, extra):
    """-> (frames (3, 20, 28) float32, maps, (x0, y0), (Hc, Wc)) of range_feature_scenes.mosaic_scene, the canvas `extra` columns
    wider"""
    import range_feature_scenes as RF

    frames, maps, origin, (Hc, Wc) = RF.mosaic_scene(name, projective)
    return frames, maps, origin, (Hc, Wc + extra)


def state_of(frames, maps, skip, exposure, x0, y0, Hc, Wc, blend):
    """the statement's canvas state after these frames (exposure None: the plain accumulate)"""
    st = MM.empty_state(Hc, Wc)
    if exposure is None:
        return MM.accumulate(st, frames, maps, skip, x0, y0, blend)
    return MEM.accumulate(st, frames, maps, skip, exposure, x0, y0, blend)


def value(state):
    """f32(sum / wsum) where count > 0, else 0: what resolve forms before a uint8 conversion"""
    return MM.resolve(state, False)[0]


# ---- extremes --------------------------------------------------------------------------------------------------------
EXTREMES = ("zeros", "full", "checker", "stripes")


def extreme(name, shape):
    """a uint8 array of any shape (planar, packed or NV12 frames): all 0, all 255, 0 / 255 alternating along every axis, or
    254, 254, 255, 255 along every axis"""
    shape = tuple(shape)
    idx = np.indices(shape).sum(0)   # the sum of all indices: a checkerboard in every pair of axes
    if name == "zeros":
        return np.zeros(shape, np.uint8)
    if name == "full":
        return np.full(shape, 255, np.uint8)
    if name == "checker":
        return np.ascontiguousarray(np.where(idx % 2 == 0, 0, 255).astype(np.uint8))
    assert name == "stripes"
    return np.ascontiguousarray(np.where(idx % 4 < 2, 254, 255).astype(np.uint8))


def warp_cells(name):
    """[(what, layout, arg, frames, maps)]: every warp under the maps of its own GPU test.  layout "planar" (arg None), "packed"
    (arg: the channels) or "nv12" (arg: the siting); maps (F, 6) for the affine warp, (F, 9) for the perspective one"""
    import colour_model as CM
    import nv12_model as NM
    from test_gpu_homography import _maps as perspective_maps
    from test_gpu_stabilize import _maps as affine_maps

    cells = []
    for H, W in ((5, 7), (12, 264)):
        for maps in (affine_maps(H, W), perspective_maps(H, W)):
            cells.append((f"planar {H}x{W}", "planar", None, extreme(name, (len(maps), H, W)), maps))
    for (H, W), C in (((7, 13), 3), ((8, 16), 4)):
        for named in (CM.affine_maps(H, W), CM.perspective_maps(H, W)):
            maps = np.stack(list(named.values()))
            cells.append((f"packed {C} {H}x{W}", "packed", C, extreme(name, (len(maps), H, W, C)), maps))
    for (H, W), siting in (((6, 10), "left"), ((8, 16), "center")):
        for named in (NM.affine_maps(H, W), NM.perspective_maps(H, W)):
            maps = np.concatenate(list(named.values()))
            cells.append((f"nv12 {siting} {H}x{W}", "nv12", siting, extreme(name, (len(maps), 3 * H // 2, W)), maps))
    return [(f"{name} {w} {'affine' if m.shape[1] == 6 else 'perspective'}", lay, arg, fr, m) for w, lay, arg, fr, m in cells]


def _planar(maps):
    import homography_model as HM
    import stabilize_model as SM

    return SM.warp if np.shape(maps)[1] == 6 else HM.warp


def warp_statement(layout, arg, frames, maps):
    """the statement's uint8 frames"""
    import colour_model as CM
    import nv12_model as NM

    affine = np.shape(maps)[1] == 6
    if layout == "planar":
        return _planar(maps)(frames, maps)[0]
    if layout == "packed":
        return (CM.warp_affine if affine else CM.warp_perspective)(frames, maps)[0]
    return (NM.warp_affine if affine else NM.warp_perspective)(frames, maps, arg)[0]


def warp_values(layout, arg, frames, maps):
    """the float32 values that the statement forms before its uint8 conversion, one array per plane: the planar statement on
    the float32 copy of every plane (a byte widens exactly); NV12 chroma where its own warp is outside: 128"""
    import nv12_model as NM

    planar = _planar(maps)
    if layout == "planar":
        return [planar(frames.astype(np.float32), maps)[0]]
    if layout == "packed":
        return [planar(np.ascontiguousarray(frames[..., c], np.float32), maps)[0] for c in range(arg)]
    y, uv = NM.planes(frames)
    out = [planar(np.ascontiguousarray(y, np.float32), maps)[0]]
    mc = NM.chroma_maps(maps, arg)
    for c in range(2):
        v, ins = planar(np.ascontiguousarray(uv[..., c], np.float32), mc)
        out.append(np.where(ins != 0, v, np.float32(NM.FILL)))
    return out


def interp_cells(name):
    """[(what, layout, arg, frames (2, ...), flows, taus)]: interpolate_frames in grey, packed and NV12 on the flows and the
    taus of tests/test_gpu_interp.py"""
    from test_gpu_interp import TAUS, _planted_flows, _wild_flows

    cells = []
    for (H, W), layout, arg in (((37, 53), "planar", None), ((5, 64), "planar", None), ((37, 53), "packed", 3), ((5, 64), "packed", 4),
                                ((38, 54), "nv12", "left"), ((6, 128), "nv12", "center")):
        shape = {"planar": (2, H, W), "packed": (2, H, W, arg), "nv12": (2, 3 * H // 2, W)}[layout]
        for kind, make in (("planted", _planted_flows), ("wild", _wild_flows)):
            cells.append((f"{name} {layout} {arg} {H}x{W} {kind}", layout, arg, extreme(name, shape), make(1, H, W, seed=H * 7 + W), TAUS))
    return cells


def interp_statement(layout, arg, frames, flows, taus):
    import interp_colour_model as CM
    import interp_model as M

    if layout == "planar":
        return M.interpolate(frames, *flows, taus)[0]
    if layout == "packed":
        return CM.interpolate_packed(frames, *flows, taus)[0]
    return CM.interpolate_nv12(frames, *flows, taus, arg)[0]


def interp_values(layout, arg, frames, flows, taus):
    """as warp_values: the float32 frames before the conversion, one array per plane"""
    import interp_colour_model as CM
    import interp_model as M
    import nv12_model as NM

    if layout == "planar":
        return [M.interpolate(frames.astype(np.float32), *flows, taus)[0]]
    if layout == "packed":
        return [M.interpolate(np.ascontiguousarray(frames[..., c], np.float32), *flows, taus)[0] for c in range(arg)]
    y, uv = NM.planes(frames)
    chroma = [CM.chroma_value(uv[0], uv[1], flows[0][0], flows[1][0], flows[2][0], flows[3][0], tau, arg) for tau in taus]
    return [M.interpolate(np.ascontiguousarray(y, np.float32), *flows, taus)[0], np.stack(chroma)]


def mosaic_cells(name):
    """[(what, frames (13, H, W), maps, skip, x0, y0, Hc, Wc)]: the plain mosaic on CASES under one map of every kind of
    tests/test_gpu_mosaic.py"""
    from test_gpu_mosaic import _maps

    cells = []
    for case, ((H, W), (Hc, Wc), (x0, y0), _, _) in enumerate(CASES):
        maps, skip = _maps(13, H, W, x0, y0, Hc, Wc, seed=case)
        cells.append((f"{name} case {case}", extreme(name, (13, H, W)), maps, skip, x0, y0, Hc, Wc))
    return cells


# ---- the pan whose highlights clip -----------------------------------------------------------------------------------
def highlight_pan():
    """-> dict: frames (8, 96, 128) uint8; maps (8, 9) integer translations from the anchor's coordinates (the anchor is the
    last frame); exposure (8, 2) from the planted gains and biases; origin, shape of the canvas; truth (Hc, Wc) float64, the
    source at the anchor's exposure; clipped (Hc, Wc) bool: a sample that was clipped when its frame was made contributes"""
    import align_photo_model as APM

    frames, src, gains, biases = APM.pan_scene(contrast=(0.0, 1.0))
    T, H, W = frames.shape
    step, a = 5, T - 1
    eg = gains[a] / gains
    exposure = np.stack([eg, biases[a] - eg * biases], 1)
    maps = np.stack([MM.translation(step * (a - k), 0) for k in range(T)])
    x0, y0, Hc, Wc = -step * a, 0, H, W + step * a
    truth = gains[a] * src[4:4 + Hc, 4:4 + Wc] + biases[a]
    clipped = np.zeros((Hc, Wc), bool)
    for k in range(T):
        raw = np.rint(gains[k] * src[4:4 + H, 4 + step * k:4 + step * k + W] + biases[k])
        clipped[:, step * k:step * k + W] |= (raw < 0) | (raw > 255)
    return dict(frames=frames, maps=maps, exposure=exposure, origin=(x0, y0), shape=(Hc, Wc), truth=truth, clipped=clipped,
                anchor=a)
