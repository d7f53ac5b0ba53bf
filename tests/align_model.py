"""The statement of direct image alignment (oflk_align_refine, oflk_align_sequence and their host forms) in NumPy.

Test infrastructure: the product never imports this file.  The kernels (csrc/oflk_align.hpp) are held to it byte for byte, a
NaN equal to a NaN.

Inverse-compositional Lucas-Kanade registration of frame B to the template A, coarse to fine, from a given step model.  The
model M maps A's coordinates to B's (warp_perspective(B, M) lies on A); the residual at pixel x of A is r(x) = B(M x) - A(x).
`kind` is AFFINE (six float32 [a00 a01 tx; a10 a11 ty], NP = 6 parameters) or HOMOGRAPHY (nine float32 row-major with
[2][2] == 1, NP = 8).  Both are carried as nine float64 (an affine model has the third row (0, 0, 1)), every operation float64
unless stated, rounded on its own, in the order written.  L levels, n iterations per level.

0. A step whose input status is 0 or whose model has an entry that is not finite is returned as it went in: the model's bytes,
   status 0, stats four zeros.
1. Pyramids: build_gaussian_pyramid (scale 0.5) of A and of B as float32, uint8 frames converted first; level 0 is the
   coarsest, level L-1 the frame.  Level l has H_l x W_l pixels.
2. `sums(l, M_l)`: for every pixel (x, y) of level l
       w = (m6 x + m7 y) + m8;  xs = ((m0 x + m1 y) + m2) / w;  ys = ((m3 x + m4 y) + m5) / w     (the perspective warp's)
       counted = w > 0 and 0 <= xs <= W_l - 1 and 0 <= ys <= H_l - 1, a NaN anywhere meaning not counted
       r = f64(sample(B_l, xs, ys) - A_l[y][x]), the difference in float32 (sample: track_model.sample)
       Gx, Gy = compute_gradients(A_l, A_l)'s Ix, Iy at the pixel, as float64
       xh = (x - cx) / s, yh = (y - cy) / s with cx = (W_l - 1) / 2, cy = (H_l - 1) / 2, s = max(W_l, H_l) / 2
       sd = [Gx xh, Gx yh, Gx, Gy xh, Gy yh, Gy, -(t xh), -(t yh)] with t = sd[0] + sd[4]; AFFINE: the first six
   and the NS = NP (NP + 1) / 2 + NP + 2 sums over the counted pixels, in this order of k: sd[i] sd[j] for i = 0 .. NP-1,
   j = i .. NP-1;  sd[i] r for i = 0 .. NP-1;  r r;  1.0 (the count).  The order of every sum (`ordered_sum`): the level is
   cut into tiles of TILE_W = 64 columns by TILE_H = 32 rows from the origin.  In a tile, column c's partial starts at +0.0
   and adds its counted pixels top to bottom; the 64 partials are combined by motion_model.lane_sum's tree (for stride 32,
   16, .., 1: partial[c] += partial[c + stride] for c < stride); the total starts at +0.0 and adds the tile sums one after
   another in raster order (left to right, then down).  A column past the level's edge has the partial +0.0.
3. e0, c0: r r and the count of sums(L - 1, M) with the input model; stats[0] = e0 / c0.
4. For l = 0 .. L-1: unless the step is frozen, M_l = D M D^-1 with sx = W_l / W, sy = H_l / H (`to_level`):
       [m0, (m1 sx) / sy, m2 sx;  (m3 sy) / sx, m4, m5 sy;  m6 / sx, m7 / sy, m8]
   then n times, unless the step is frozen:
   (a) S = sums(l, M_l).  The step freezes when the count < f64(f32(min_share)) * f64(W_l H_l).
   (b) The normal equations [G | b], G the symmetric matrix of the sd[i] sd[j] sums, b the sd[i] r sums, eliminated without
       pivoting by homography_model.solve8's procedure on NP rows.  The step freezes when a pivot is zero or not finite.
   (c) p = -(q / s) for the solution q: the reference's Sobel operator is a true convolution, so Gx, Gy are minus the
       derivatives of A and q is minus the Gauss-Newton step.  P = [p0 p1 p2; p3 p4 p5; p6 p7 0] (AFFINE: p6 = p7 = 0).  Its
       conjugate to pixels:
       A[r][0] = P[r][0] / s;  A[r][1] = P[r][1] / s;  A[r][2] = P[r][2] - (A[r][0] cx + A[r][1] cy)
       D[0][c] = s A[0][c] + cx A[2][c];  D[1][c] = s A[1][c] + cy A[2][c];  D[2][c] = A[2][c]
       dM = D with 1.0 added to the three diagonal entries.
   (d) I = adj(dM) / adj(dM)[2][2] (homography_model.adjugate, nine divisions);
       N[r][c] = (M_l[r][0] I[0][c] + M_l[r][1] I[1][c]) + M_l[r][2] I[2][c].
       The step freezes when an entry of N is not finite or (n6 x + n7 y) + n8 > 0 fails at one of the level's corners
       (0, 0), (W_l-1, 0), (W_l-1, H_l-1), (0, H_l-1).  Otherwise M_l = N and the step has one more accepted update.
   A step that freezes keeps its M_l.  After the level's last iteration, or at once when the step freezes, M goes back to the
   frame (`from_level`):  [m0, (m1 sy) / sx, m2 / sx;  (m3 sx) / sy, m4, m5 / sy;  m6 sx, m7 sy, m8].  Nothing touches a frozen
   step's model afterwards.
5. e1, c1 of sums(L - 1, M) with the final model.  stats = [e0 / c0, e1 / c1, c1 / f64(W H), accepted updates].
       no accepted update:     the input model's bytes, status 0
       not e1 / c1 <= e0 / c0: the input model's bytes, status 2 (rejected; a NaN on either side -- no counted pixel -- included)
       else:                   status 1 and the model rounded to float32: AFFINE m0 .. m5, HOMOGRAPHY m_k / m8 for k = 0 .. 8
"""
import numpy as np

import homography_model as HM
import oflk_oracle as O
from track_model import sample as bilinear

AFFINE, HOMOGRAPHY = 0, 1
KINDS = {"affine": AFFINE, "homography": HOMOGRAPHY}
TILE_W, TILE_H = 64, 32


def n_params(kind):
    return 8 if kind == HOMOGRAPHY else 6


def n_sums(kind):
    NP = n_params(kind)
    return NP * (NP + 1) // 2 + NP + 2


def ordered_sum(terms, counted):
    """terms (NS, H, W) float64, counted (H, W) bool -> (NS,) float64 in the stated order"""
    NS, H, W = terms.shape
    TH, TW = -(-H // TILE_H), -(-W // TILE_W)
    t = np.zeros((NS, TH * TILE_H, TW * TILE_W))
    t[:, :H, :W] = np.where(counted[None], terms, 0.0)   # adding +0.0 to a partial that began at +0.0 changes nothing
    t = t.reshape(NS, TH, TILE_H, TW, TILE_W)
    acc = np.zeros((NS, TH, TW, TILE_W))
    for r in range(TILE_H):
        acc = acc + t[:, :, r]
    st = TILE_W // 2
    while st >= 1:
        acc[..., :st] = acc[..., :st] + acc[..., st:2 * st]
        st //= 2
    tiles = acc[..., 0].reshape(NS, TH * TW)
    total = np.zeros(NS)
    for k in range(TH * TW):
        total = total + tiles[:, k]
    return total


class Level:
    """the template's quantities at one level: gradients, normalised coordinates"""

    def __init__(self, A, B):
        self.A, self.B = A, B
        self.H, self.W = A.shape
        gx, gy, _ = O.compute_gradients(A, A)
        self.gx, self.gy = gx.astype(np.float64), gy.astype(np.float64)
        self.cx, self.cy = np.float64(self.W - 1) / 2.0, np.float64(self.H - 1) / 2.0
        self.s = np.float64(max(self.W, self.H)) / 2.0
        self.xh = ((np.arange(self.W, dtype=np.float64) - self.cx) / self.s)[None, :]
        self.yh = ((np.arange(self.H, dtype=np.float64) - self.cy) / self.s)[:, None]


def sums(lv, m, kind):
    """step 2: (NS,) float64"""
    NP = n_params(kind)
    H, W = lv.H, lv.W
    xs, ys, w = HM.coordinates(m, H, W)
    with np.errstate(all="ignore"):
        ok = (w > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        v = np.zeros((H, W), np.float32)
        v[ok] = bilinear(lv.B, xs[ok], ys[ok])
        r = (v - lv.A).astype(np.float64)
        sd = [lv.gx * lv.xh, lv.gx * lv.yh, lv.gx, lv.gy * lv.xh, lv.gy * lv.yh, lv.gy]
        if NP == 8:
            t = sd[0] + sd[4]
            sd += [-(t * lv.xh), -(t * lv.yh)]
        terms = [sd[i] * sd[j] for i in range(NP) for j in range(i, NP)] + [sd[i] * r for i in range(NP)]
        terms += [r * r, np.ones((H, W))]
        return ordered_sum(np.stack(terms), ok)


def to_level(m, sx, sy):
    return [m[0], (m[1] * sx) / sy, m[2] * sx, (m[3] * sy) / sx, m[4], m[5] * sy, m[6] / sx, m[7] / sy, m[8]]


def from_level(m, sx, sy):
    return [m[0], (m[1] * sy) / sx, m[2] / sx, (m[3] * sx) / sy, m[4], m[5] / sy, m[6] * sx, m[7] * sy, m[8]]


def solve(G, NP):
    """homography_model.solve8's elimination on the NP x (NP + 1) array [G | b]: ((NP,) float64, ok)"""
    if NP == 8:
        return HM.solve8(G)
    G = np.array(G, np.float64)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(NP):
            piv = G[k, k]
            ok = ok and bool(piv != 0.0 and np.isfinite(piv))
            for i in range(k + 1, NP):
                f = G[i, k] / piv
                for j in range(k + 1, NP + 1):
                    G[i, j] = G[i, j] - f * G[k, j]
        h = np.zeros(NP)
        for i in range(NP - 1, -1, -1):
            s = G[i, NP]
            for j in range(i + 1, NP):
                s = s - G[i, j] * h[j]
            h[i] = s / G[i, i]
    return h, ok


def normal_equations(S, NP):
    G = np.zeros((NP, NP + 1))
    k = 0
    for i in range(NP):
        for j in range(i, NP):
            G[i, j] = G[j, i] = S[k]
            k += 1
    G[:, NP] = S[k:k + NP]
    return G


def update(m, q, lv, NP):
    """steps (c), (d): (N (9 floats), ok)"""
    s, cx, cy = lv.s, lv.cx, lv.cy
    with np.errstate(all="ignore"):
        p = [-(np.float64(q[k]) / s) for k in range(NP)] + [np.float64(0.0)] * (8 - NP)
        P = p + [np.float64(0.0)]
        A = []
        for r in range(3):
            a0, a1 = P[3 * r] / s, P[3 * r + 1] / s
            A += [a0, a1, P[3 * r + 2] - (a0 * cx + a1 * cy)]
        D = [s * A[c] + cx * A[6 + c] for c in range(3)] + [s * A[3 + c] + cy * A[6 + c] for c in range(3)] + A[6:]
        D[0], D[4], D[8] = D[0] + 1.0, D[4] + 1.0, D[8] + 1.0
        adj = HM.adjugate(D)
        inv = [a / adj[8] for a in adj]
        N = [(m[3 * r] * inv[c] + m[3 * r + 1] * inv[3 + c]) + m[3 * r + 2] * inv[6 + c] for r in range(3) for c in range(3)]
        ok = bool(np.isfinite(N).all())
        for x, y in ((0, 0), (lv.W - 1, 0), (lv.W - 1, lv.H - 1), (0, lv.H - 1)):
            ok = ok and bool((N[6] * np.float64(x) + N[7] * np.float64(y)) + N[8] > 0)
    return N, ok


def pyramids(frame, levels):
    return O.build_gaussian_pyramid(np.asarray(frame).astype(np.float32), levels, 0.5)


def refine_pyramids(pa, pb, model, status=1, kind=HOMOGRAPHY, iterations=5, min_share=0.25):
    """one step on the two pyramids: (model like the input, status int, stats (4,) float64)"""
    NP, L = n_params(kind), len(pa)
    model = np.asarray(model, np.float32).reshape(-1)
    assert model.size == (9 if kind == HOMOGRAPHY else 6) and iterations >= 1
    if status == 0 or not np.isfinite(model).all():
        return model.copy(), 0, np.zeros(4)
    m = [np.float64(c) for c in model] + ([np.float64(0.0), np.float64(0.0), np.float64(1.0)] if kind == AFFINE else [])
    lvs = [Level(a, b) for a, b in zip(pa, pb)]
    H, W = lvs[-1].H, lvs[-1].W
    share = np.float64(np.float32(min_share))
    with np.errstate(all="ignore"):
        S = sums(lvs[-1], m, kind)
        before = S[-2] / S[-1]
        frozen, accepted = False, 0
        for lv in lvs:
            if frozen:
                break
            sx, sy = np.float64(lv.W) / np.float64(W), np.float64(lv.H) / np.float64(H)
            m = to_level(m, sx, sy)
            for _ in range(iterations):
                S = sums(lv, m, kind)
                if S[-1] < share * np.float64(lv.W * lv.H):
                    frozen = True
                    break
                q, ok = solve(normal_equations(S, NP), NP)
                if not ok:
                    frozen = True
                    break
                N, ok = update(m, q, lv, NP)
                if not ok:
                    frozen = True
                    break
                m, accepted = N, accepted + 1
            m = from_level(m, sx, sy)
        S = sums(lvs[-1], m, kind)
        after = S[-2] / S[-1]
        stats = np.array([before, after, S[-1] / np.float64(W * H), accepted], np.float64)
        if accepted == 0:
            return model.copy(), 0, stats
        if not after <= before:
            return model.copy(), 2, stats
        out = np.array([c / m[8] for c in m] if kind == HOMOGRAPHY else m[:6], np.float64).astype(np.float32)
    return out, 1, stats


def refine(a, b, model, status=None, kind=HOMOGRAPHY, levels=3, iterations=5, min_share=0.25):
    """a, b (S, H, W) float32 or uint8, model (S, 6 | 9), status (S,) or None -> (model (S, nc) float32, status (S,) int32,
    stats (S, 4) float64)"""
    a, b = np.asarray(a), np.asarray(b)
    model = np.asarray(model, np.float32).reshape(len(a), -1)
    r = [refine_pyramids(pyramids(a[s], levels), pyramids(b[s], levels), model[s], 1 if status is None else int(status[s]), kind,
                         iterations, min_share) for s in range(len(a))]
    return np.stack([x[0] for x in r]), np.array([x[1] for x in r], np.int32), np.stack([x[2] for x in r])


def sequence(frames, model, status=None, kind=HOMOGRAPHY, levels=3, iterations=5, min_share=0.25):
    """frames (T, H, W): the T-1 steps t -> t + 1, every frame's pyramid built once"""
    frames = np.asarray(frames)
    model = np.asarray(model, np.float32).reshape(len(frames) - 1, -1)
    pyr = [pyramids(f, levels) for f in frames]
    r = [refine_pyramids(pyr[t], pyr[t + 1], model[t], 1 if status is None else int(status[t]), kind, iterations, min_share)
         for t in range(len(frames) - 1)]
    return np.stack([x[0] for x in r]), np.array([x[1] for x in r], np.int32), np.stack([x[2] for x in r])


def same(got, want, what=""):
    """model, status, stats byte for byte; a NaN equals a NaN"""
    for g, w, name in zip(got, want, ("model", "status", "stats")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} {g.shape} {g.dtype} != {w.shape} {w.dtype}"
        if g.dtype.kind == "f":
            u = np.uint32 if g.dtype == np.float32 else np.uint64
            eq = (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))
        else:
            eq = g == w
        assert eq.all(), f"{what}: {name} differs at {np.argwhere(~eq)[:5].tolist()}: got {g[~eq][:5]}, want {w[~eq][:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
IDENTITY = {AFFINE: np.array([1, 0, 0, 0, 1, 0], np.float32), HOMOGRAPHY: np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)}


def texture(H, W, seed, sigma=3.0, margin=24):
    """band-limited noise in [0, 255] on a canvas `margin` pixels larger than the frame on every side: (H + 2m, W + 2m) float64"""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    t = gaussian_filter(rng.standard_normal((H + 2 * margin, W + 2 * margin)), sigma)
    t = (t - t.min()) / (t.max() - t.min())
    return 255.0 * t


def view(canvas, H, W, m, margin=24):
    """the (H, W) float32 frame that sees canvas point (margin, margin) + m(x, y) at pixel (x, y): cubic resampling"""
    from scipy.ndimage import map_coordinates

    p = HM.apply(np.asarray(m, np.float64).reshape(9), np.stack(np.meshgrid(np.arange(W, dtype=np.float64),
                                                                           np.arange(H, dtype=np.float64)), -1))
    return map_coordinates(canvas, [p[..., 1] + margin, p[..., 0] + margin], order=3, mode="nearest").astype(np.float32)


def corner_map(H, W, shifts):
    """the homography that moves the frame's corners (0,0), (W-1,0), (W-1,H-1), (0,H-1) by shifts (4, 2): (9,) float64"""
    x = np.array([0.0, W - 1.0, W - 1.0, 0.0])
    y = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    sh = np.asarray(shifts, np.float64)
    S, _ = HM.square_to_quad(list(x), list(y))
    D, _ = HM.square_to_quad(list(x + sh[:, 0]), list(y + sh[:, 1]))
    Hm = np.array(D).reshape(3, 3) @ np.linalg.inv(np.array(S).reshape(3, 3))
    return (Hm / Hm[2, 2]).reshape(9)


def corner_error(m, planted, H, W):
    """the largest distance between the frame's corners under m and under the planted map"""
    c = np.array([[0.0, 0.0], [W - 1.0, 0.0], [W - 1.0, H - 1.0], [0.0, H - 1.0]])
    m = np.asarray(m, np.float64).reshape(-1)
    if m.size == 6:
        m = np.concatenate([m, [0.0, 0.0, 1.0]])
    return float(np.abs(HM.apply(m, c) - HM.apply(planted, c)).max())


def planted_pair(H, W, seed, kind=HOMOGRAPHY, move=3.0):
    """A, B (H, W) float32 and the planted map (9,) float64 with B(M x) = A(x): B is resampled (cubic) from A's canvas under the
    inverse of a map that moves the frame's corners by up to `move` px (AFFINE: three corners, the fourth follows)"""
    canvas = texture(H, W, seed)
    sh = np.random.default_rng(1000 + seed).uniform(-move, move, (4, 2))
    if kind == AFFINE:
        sh[2] = sh[1] + sh[3] - sh[0]
    m = corner_map(H, W, sh)
    if kind == AFFINE:
        m[6:] = (0.0, 0.0, 1.0)
    inv = np.linalg.inv(m.reshape(3, 3))
    return view(canvas, H, W, IDENTITY[HOMOGRAPHY]), view(canvas, H, W, (inv / inv[2, 2]).reshape(9)), m


def pushed(planted, H, W, kind, by=1.0):
    """the planted map with the frame's corners pushed by `by` px in alternating directions (AFFINE: a parallelogram of pushes), as the float32 model of `kind`"""
    push = np.array([[1, -1], [-1, 1], [1, 1], [-1, -1.0]] if kind == HOMOGRAPHY else [[1, -1], [-1, -1], [-1, 1], [1, 1.0]]) * by
    m = corner_map(H, W, push).reshape(3, 3) @ np.asarray(planted).reshape(3, 3)
    m = (m / m[2, 2]).reshape(9)
    return m.astype(np.float32) if kind == HOMOGRAPHY else m[:6].astype(np.float32)


def checker_pair(H, W):
    """a step that the refinement makes worse: a one-pixel checkerboard, which the Sobel operator does not see, on a ramp, and
    the same plus one grey level.  The ramp's gradient asks for a one-pixel shift, which turns the checkerboard over."""
    yy, xx = np.mgrid[:H, :W]
    A = (100.0 * ((xx + yy) % 2) + xx + 0.5 * yy).astype(np.float32)
    return A, A + np.float32(1.0)
