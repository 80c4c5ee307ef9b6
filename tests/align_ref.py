"""The specification of DeviceImage.align / align_sums / warp and lib.utils.align / warp (csrc/ics_img_align.hip, include/ics_hip.h) in
numpy, with the dtype as a parameter: float64 is the oracle of the tests, float32 the restatement of the device's arithmetic and of its
summation order.  Registration of two RGB frames by coarse-to-fine Gauss-Newton on the luma (forward-additive Lucas-Kanade, Levenberg's
damping), and the projective warp of a frame by Keys' cubic convolution.

M, 3 x 3 with M[2][2] = 1, takes a pixel (x, y, 1) of `fixed` to the position (u, v) = (M0 . p, M1 . p) / (M2 . p) in `moving`.

  luma     Y = ((R + G) + B) * (1 / 3), smoothed by the binomial 1 2 1 each way -- a row is (l + r) + 2 c, the three rows are combined
           the same way, times 1 / 16, the window repeating its edge --, every operation rounded once; of the window (y0, y1, x0, x1)
           of `fixed`, of all of `moving`.  The loop runs on the window plane, M T(x0, y0) in place of M.  (The smoothing makes the
           bilinear sample and its central differences describe one and the same surface on pictures with hard edges; without it the
           affine model misses 0.2 px on the dead-leaves pair under a 9 px box.)
  pyramid  level l + 1 = ((a + b) + (c + d)) * 0.25 of the 2 x 2 block a b / c d of level l, an odd last row or column dropped; pixel
           centres map as X = 2 (x + 0.5) - 0.5, so M' = C^-1 M C with C = [[2, 0, 0.5], [0, 2, 0.5], [0, 0, 1]].  levels=None: halve
           while the smaller side of the next level of either plane stays >= 64, at most 8 levels; no level below 16 px a side.
  frame    coordinates are taken from the centre of a plane and divided by half its longer side: N = [[s, 0, (W - 1) / 2], [0, s,
           (H - 1) / 2], [0, 0, 1]], s = max(H, W) / 2.  A = Nm^-1 M Nf with A[2][2] = 1 is what a step works on: its entries are the
           parameters, "translation" A02 A12, "affine" A00 .. A12, "homography" A00 .. A21, in this order, then gain a and bias b.
  sample   at a pixel (x, y) of the fixed plane: xn = (x - cx) (1 / s), yn likewise; D = (A20 xn + A21 yn) + 1, iD = 1 / D,
           un = ((A00 xn + A01 yn) + A02) iD, vn likewise; u = un sm + cmx, v = vn sm + cmy.  The pixel counts where 1 <= u < Wm - 2 and
           1 <= v < Hm - 2.  x0 = floor(u), fx = u - x0 (y likewise); bil(p00, p01, p10, p11) = t + fy (s - t) with t = p00 + fx (p01 -
           p00), s = p10 + fx (p11 - p10).  I = bil of the four pixels around; gx = bil of 0.5 (I[y][x + 1] - I[y][x - 1]) at the same
           four pixels, gy of 0.5 (I[y + 1][x] - I[y - 1][x]).
  row      r = (a I + b) - T;  hu = ((a sm) gx) iD, hv = ((a sm) gy) iD;  J = [hu, hv] | [hu xn, hu yn, hu, hv xn, hv yn, hv]
           | [.., q xn, q yn] with q = -(hu un + hv vn); photometric: and [I, 1].
  sums     S = sum J^T J (upper triangle, row-major), g = sum J^T r, sum r^2, count.  float32: a 32 x 32 tile belongs to 64 lanes,
           lane = 32 (y % 2) + x, each adds its 16 pixels top to bottom, the lanes are added in lane order, all in float32; the tiles
           are added in float64 (the device in interleaved runs, here row-major: at these gates the order of a float64 sum does not show).
  step     (S + lambda diag S) d = -g by Cholesky in float64 (a pivot that is not > 0: "no texture to align on"); A + d is evaluated;
           accepted where sum r^2 / count did not rise (lambda / 10), else rejected (lambda * 10); lambda starts at 1e-6 at every
           level.  A level ends when the largest motion of its four corners under a step is below `tolerance` px (whether the step was
           accepted or not) or after `iterations` steps.  A sum that is not finite: "not finite: despeckle first"; count below a
           quarter of the plane: "frames do not overlap enough".
  warp     out[y][x][c] = src at (u, v) = (((M00 x + M01 y) + M02) / D, ...), D = (M20 x + M21 y) + M22, in float64 for every dtype; u
           clamped to [-2, W + 1] (a NaN to -2); x0 = floor(u), t = u - x0 rounded to the dtype, taps x0 - 1 .. x0 + 2 clamped to the frame, weights w0 = ((-0.5 t + 1) t - 0.5) t,
           w1 = ((1.5 t - 2.5) t) t + 1, w2 = ((-1.5 t + 2) t + 0.5) t, w3 = ((0.5 t - 0.5) t) t; a row is ((w0 p0 + w1 p1) + w2 p2) +
           w3 p3, the four rows are combined the same way."""
import collections
import functools

import numpy as np

from wiener_ref import dead_leaves

MODELS = {"translation": 2, "affine": 6, "homography": 8}
PARAMS = {"translation": (2, 5), "affine": (0, 1, 2, 3, 4, 5), "homography": (0, 1, 2, 3, 4, 5, 6, 7)}   # entries of A (row-major) a step moves
TILE, LANES = 32, 64            # csrc/ics_img_align.hip ALT, ALLANES
SUMS_BAND = 8 * TILE           # rows of a plane whose products `sums` holds at a time (the float64 sum over the tiles goes band by band)
MIN_SIDE, AUTO_SIDE, MAX_LEVELS = 16, 64, 8
MIN_COVERAGE = 0.25
LAMBDA0 = 1e-6
UP = np.array([[2.0, 0.0, 0.5], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]])

Alignment = collections.namedtuple("Alignment", "matrix gain bias rms coverage steps levels")


def luma(pic, dtype=np.float64):
    """the luma of a window, smoothed by the binomial 1 2 1 each way, the window repeating its edge"""
    c = np.asarray(pic).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        Y = np.pad(((c[..., 0] + c[..., 1]) + c[..., 2]) * dtype(1.0 / 3.0), 1, mode="edge")
        R = (Y[:, :-2] + Y[:, 2:]) + dtype(2) * Y[:, 1:-1]
        out = ((R[:-2] + R[2:]) + dtype(2) * R[1:-1]) * dtype(0.0625)
    assert out.dtype == dtype
    return out


def half(P):
    h, w = P.shape[0] // 2, P.shape[1] // 2
    a, b, c, d = P[0:2 * h:2, 0:2 * w:2], P[0:2 * h:2, 1:2 * w:2], P[1:2 * h:2, 0:2 * w:2], P[1:2 * h:2, 1:2 * w:2]
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a + b) + (c + d)) * P.dtype.type(0.25)


def auto_levels(*shapes):
    """levels=None for planes of these (H, W)"""
    side, n = min(min(s[0], s[1]) for s in shapes), 1
    while n < MAX_LEVELS and (side >> n) >= AUTO_SIDE:
        n += 1
    return n


def frame_of(H, W):
    s = max(H, W) / 2.0
    return np.array([[s, 0.0, (W - 1) / 2.0], [0.0, s, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def to_frame(M, shape_f, shape_m):
    A = np.linalg.inv(frame_of(*shape_m)) @ M @ frame_of(*shape_f)
    return A / A[2, 2]


def from_frame(A, shape_f, shape_m):
    M = frame_of(*shape_m) @ A @ np.linalg.inv(frame_of(*shape_f))
    return M / M[2, 2]


def rows(T, I, A, model, photometric, gain=1.0, bias=0.0, dtype=np.float64):
    """per pixel of the fixed plane T: (J, r, valid) -- J of shape H x W x n, zero where the pixel does not count"""
    T, I = np.asarray(T, dtype=dtype), np.asarray(I, dtype=dtype)
    H, W = T.shape
    Hm, Wm = I.shape
    A = np.asarray(A, dtype=np.float64).astype(dtype)
    Nf, Nm = frame_of(H, W), frame_of(Hm, Wm)
    isf, sm = dtype(1.0 / Nf[0, 0]), dtype(Nm[0, 0])
    cfx, cfy, cmx, cmy = dtype(Nf[0, 2]), dtype(Nf[1, 2]), dtype(Nm[0, 2]), dtype(Nm[1, 2])
    a, b = dtype(gain), dtype(bias)
    yy, xx = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        xn, yn = (xx.astype(dtype) - cfx) * isf, (yy.astype(dtype) - cfy) * isf
        D = (A[2, 0] * xn + A[2, 1] * yn) + dtype(1)
        iD = dtype(1) / D
        un = ((A[0, 0] * xn + A[0, 1] * yn) + A[0, 2]) * iD
        vn = ((A[1, 0] * xn + A[1, 1] * yn) + A[1, 2]) * iD
        u, v = un * sm + cmx, vn * sm + cmy
        valid = (u >= 1) & (u < Wm - 2) & (v >= 1) & (v < Hm - 2)
        us, vs = np.where(valid, u, dtype(1)), np.where(valid, v, dtype(1))
        fu, fv = np.floor(us), np.floor(vs)
        fx, fy = us - fu, vs - fv
        x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
        if min(Hm, Wm) < 4:
            valid = np.zeros_like(valid)
            x0, y0 = np.zeros_like(x0), np.zeros_like(y0)
            P = lambda dy, dx: np.zeros((H, W), dtype)
        else:
            P = lambda dy, dx: I[y0 + dy, x0 + dx]
        half_ = dtype(0.5)

        def bil(p00, p01, p10, p11):
            t = p00 + fx * (p01 - p00)
            s = p10 + fx * (p11 - p10)
            return t + fy * (s - t)

        val = bil(P(0, 0), P(0, 1), P(1, 0), P(1, 1))
        gx = bil(half_ * (P(0, 1) - P(0, -1)), half_ * (P(0, 2) - P(0, 0)), half_ * (P(1, 1) - P(1, -1)), half_ * (P(1, 2) - P(1, 0)))
        gy = bil(half_ * (P(1, 0) - P(-1, 0)), half_ * (P(1, 1) - P(-1, 1)), half_ * (P(2, 0) - P(0, 0)), half_ * (P(2, 1) - P(0, 1)))
        r = (a * val + b) - T
        k = a * sm
        hu, hv = (k * gx) * iD, (k * gy) * iD
        if model == "translation":
            cols = [hu, hv]
        else:
            cols = [hu * xn, hu * yn, hu, hv * xn, hv * yn, hv]
            if model == "homography":
                q = -(hu * un + hv * vn)
                cols += [q * xn, q * yn]
        if photometric:
            cols += [val, np.ones_like(val)]
        zero = dtype(0)
        J = np.stack([np.where(valid, c, zero) for c in cols], axis=-1)
        r = np.where(valid, r, zero)
    assert J.dtype == dtype and r.dtype == dtype
    return J, r, valid


def _tile_sum(p):
    """H x W x k products of one dtype -> k sums: float32 in the device's order inside a tile, float64 across the tiles"""
    H, W, k = p.shape
    if p.dtype == np.float64:
        return p.sum(axis=(0, 1))
    ty, tx = -(-H // TILE), -(-W // TILE)
    q = np.zeros((ty * TILE, tx * TILE, k), p.dtype)
    q[:H, :W] = p
    q = q.reshape(ty, TILE // 2, 2, tx, TILE, k)                     # tile row, step, y % 2, tile column, x
    lane = q[:, 0]
    for s in range(1, TILE // 2):
        lane = lane + q[:, s]                                        # ty, 2, tx, 32, k: a lane's pixels top to bottom
    lane = lane.transpose(0, 2, 1, 3, 4).reshape(ty, tx, LANES, k)
    tile = lane[:, :, 0]
    for l in range(1, LANES):
        tile = tile + lane[:, :, l]
    assert tile.dtype == p.dtype
    return tile.astype(np.float64).reshape(ty * tx, k).sum(axis=0)


def sums(T, I, A, model, photometric, gain=1.0, bias=0.0, dtype=np.float64):
    """(S n x n symmetric, g, sum r^2, count) as float64"""
    J, r, valid = rows(T, I, A, model, photometric, gain, bias, dtype)
    n = J.shape[-1]
    iu = np.triu_indices(n)
    tot = None
    with np.errstate(all="ignore"):
        for y in range(0, J.shape[0], SUMS_BAND):                    # whole tile rows at a time: a large frame's products need not all exist at once
            Jb, rb = J[y:y + SUMS_BAND], r[y:y + SUMS_BAND]
            prod = np.concatenate([Jb[..., iu[0]] * Jb[..., iu[1]], Jb * rb[..., None], (rb * rb)[..., None]], axis=-1)
            band = _tile_sum(prod)
            tot = band if tot is None else tot + band
    S = np.zeros((n, n))
    S[iu] = tot[:len(iu[0])]
    S = S + np.triu(S, 1).T
    return S, tot[len(iu[0]):len(iu[0]) + n].copy(), float(tot[-1]), int(valid.sum())


def solve(S, g, lam):
    """the damped step; ValueError("no texture to align on") where the damped matrix is not positive definite"""
    n = len(g)
    B = S + lam * np.diag(np.diag(S))
    L = np.zeros((n, n))
    for i in range(n):                                               # (the C code's Cholesky: a pivot must be > 0 and finite)
        for j in range(i + 1):
            s = B[i, j] - (L[i, :j] * L[j, :j]).sum()
            if i == j:
                if not (s > 0 and np.isfinite(s)):
                    raise ValueError("no texture to align on")
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.linalg.solve(L, -g)
    return np.linalg.solve(L.T, y)


def corner_motion(A0, A1, shape_f, shape_m):
    H, W = shape_f
    Nf, Nm = frame_of(H, W), frame_of(*shape_m)
    c = np.linalg.inv(Nf) @ np.array([[0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1], [1, 1, 1, 1]], dtype=np.float64)
    p0, p1 = A0 @ c, A1 @ c
    d = (p0[:2] / p0[2] - p1[:2] / p1[2]) * Nm[0, 0]
    return float(np.sqrt((d * d).sum(axis=0)).max())


def _evaluate(T, I, A, model, photometric, gain, bias, dtype):
    S, g, rr, count = sums(T, I, A, model, photometric, gain, bias, dtype)
    if not (np.isfinite(S).all() and np.isfinite(g).all() and np.isfinite(rr)):
        raise ValueError("the frames are not finite: despeckle first")
    if count < MIN_COVERAGE * T.size:
        raise ValueError("frames do not overlap enough (coverage %.3f)" % (count / T.size,))
    return S, g, rr, count


def level_loop(T, I, A, model, photometric, gain, bias, iterations, tolerance, dtype=np.float64):
    """one level: (A, gain, bias, sum r^2, count, steps)"""
    idx = PARAMS[model]
    S, g, rr, count = _evaluate(T, I, A, model, photometric, gain, bias, dtype)
    lam, steps = LAMBDA0, 0
    while steps < iterations:
        d = solve(S, g, lam)
        flat = A.reshape(9).copy()
        flat[list(idx)] += d[:len(idx)]
        A1 = flat.reshape(3, 3)
        g1, b1 = (gain + d[-2], bias + d[-1]) if photometric else (gain, bias)
        S1, gr1, rr1, count1 = _evaluate(T, I, A1, model, photometric, g1, b1, dtype)
        steps += 1
        motion = corner_motion(A, A1, T.shape, I.shape)
        if rr1 / count1 <= rr / count:
            A, gain, bias, S, g, rr, count = A1, g1, b1, S1, gr1, rr1, count1
            lam = lam / 10
        else:
            lam = lam * 10
        if motion < tolerance:
            break
    return A, gain, bias, rr, count, steps


def pyramids(moving, fixed, window=None, levels=None, dtype=np.float64):
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    y0, y1, x0, x1 = (0, fixed.shape[0], 0, fixed.shape[1]) if window is None else window
    Tp, Ip = [luma(fixed[y0:y1, x0:x1], dtype)], [luma(moving, dtype)]
    n = auto_levels(Tp[0].shape, Ip[0].shape) if levels is None else int(levels)
    if not 1 <= n <= MAX_LEVELS or min(min(Tp[0].shape), min(Ip[0].shape)) >> (n - 1) < MIN_SIDE:
        raise ValueError("levels: no level may be smaller than %d px a side" % MIN_SIDE)
    for _ in range(n - 1):
        Tp.append(half(Tp[-1])); Ip.append(half(Ip[-1]))
    return Tp, Ip


def align(moving, fixed, model="affine", photometric=True, levels=None, iterations=30, tolerance=1e-3, init=None, window=None, gain=1.0, bias=0.0,
          dtype=np.float64, per_level=None):
    """Alignment(matrix, gain, bias, rms, coverage, steps, levels); per_level: a list that receives the steps of every level, coarsest first"""
    Tp, Ip = pyramids(moving, fixed, window, levels, dtype)
    x0, y0 = (0, 0) if window is None else (window[2], window[0])
    M = np.eye(3) if init is None else np.asarray(init, dtype=np.float64)
    shift = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])
    M = M @ shift
    n = len(Tp)
    for _ in range(n - 1):
        M = np.linalg.inv(UP) @ M @ UP
    total = 0
    for l in range(n - 1, -1, -1):
        A = to_frame(M, Tp[l].shape, Ip[l].shape)
        A, gain, bias, rr, count, steps = level_loop(Tp[l], Ip[l], A, model, photometric, gain, bias, iterations, tolerance, dtype)
        M = from_frame(A, Tp[l].shape, Ip[l].shape)
        total += steps
        if per_level is not None:
            per_level.append(steps)
        if l:
            M = UP @ M @ np.linalg.inv(UP)
    M = M @ np.linalg.inv(shift)
    return Alignment(M / M[2, 2], float(gain), float(bias), float(np.sqrt(rr / count)), count / Tp[0].size, total, n)


def keys(t):
    dt = t.dtype.type
    w0 = ((dt(-0.5) * t + dt(1)) * t - dt(0.5)) * t
    w1 = ((dt(1.5) * t - dt(2.5)) * t) * t + dt(1)
    w2 = ((dt(-1.5) * t + dt(2)) * t + dt(0.5)) * t
    w3 = ((dt(0.5) * t - dt(0.5)) * t) * t
    return w0, w1, w2, w3


def warp(src, M, shape=None, dtype=np.float64):
    src = np.asarray(src).astype(dtype)
    H, W, _ = src.shape
    oh, ow = (H, W) if shape is None else shape
    M = np.asarray(M, dtype=np.float64)
    m = M / M[2, 2]
    yy, xx = np.mgrid[:oh, :ow]
    x, y = xx.astype(np.float64), yy.astype(np.float64)                # the position is float64 for every dtype: a float32 one is 1e-4 px off at x = 2000
    with np.errstate(all="ignore"):
        D = (m[2, 0] * x + m[2, 1] * y) + m[2, 2]
        u = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2]) / D
        v = ((m[1, 0] * x + m[1, 1] * y) + m[1, 2]) / D
        u = np.minimum(np.where(u >= -2, u, -2.0), W + 1.0)
        v = np.minimum(np.where(v >= -2, v, -2.0), H + 1.0)
        fu, fv = np.floor(u), np.floor(v)
        wx, wy = keys((u - fu).astype(dtype)), keys((v - fv).astype(dtype))
        x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
        xs = [np.clip(x0 + d, 0, W - 1) for d in (-1, 0, 1, 2)]
        ys = [np.clip(y0 + d, 0, H - 1) for d in (-1, 0, 1, 2)]
        line = []
        for j in range(4):
            p = [src[ys[j], xs[i]] for i in range(4)]
            line.append(((wx[0][..., None] * p[0] + wx[1][..., None] * p[1]) + wx[2][..., None] * p[2]) + wx[3][..., None] * p[3])
        out = ((wy[0][..., None] * line[0] + wy[1][..., None] * line[1]) + wy[2][..., None] * line[2]) + wy[3][..., None] * line[3]
    assert out.dtype == dtype
    return out


# ---- the pictures and cases of the tests --------------------------------------------------------------------------------------------
MARGIN = 40
PAIR_SHAPE = (160, 192)
GATE = 1e-4                     # align_sums and warp against float64 (tests/test_gpu_align.py)
ALIGN_GATE = 0.05               # px: the device's final matrix against the specification's, at the corners


def translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def about_centre(shape, angle_deg=0.0, scale=1.0, tx=0.0, ty=0.0, h=(0.0, 0.0)):
    """a rotation and scale about the centre of a frame of this shape, a projective row h (per pixel from the centre), then a shift"""
    cy, cx = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    a = np.deg2rad(angle_deg)
    R = np.array([[scale * np.cos(a), -scale * np.sin(a), 0.0], [scale * np.sin(a), scale * np.cos(a), 0.0], [h[0], h[1], 1.0]])
    M = translation(cx + tx, cy + ty) @ R @ translation(-cx, -cy)
    return M / M[2, 2]


# model -> the true M of the recovery pairs: motions of at most a tenth of the side at the corners
TRUE = {"translation": translation(11.3, -7.6),
        "affine": about_centre(PAIR_SHAPE, 4.0, 1.03, 2.3, -1.6),
        "homography": about_centre(PAIR_SHAPE, 2.0, 1.02, 1.7, 1.2, h=(6e-5, -4e-5))}


def corner_error(M, ref, shape):
    H, W = shape[:2]
    c = np.array([[0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1], [1, 1, 1, 1]], dtype=np.float64)
    p, q = np.asarray(M) @ c, np.asarray(ref) @ c
    d = p[:2] / p[2] - q[:2] / q[2]
    return float(np.sqrt((d * d).sum(axis=0)).max())


def box_blur(pic, k):
    from scipy.ndimage import uniform_filter
    return uniform_filter(pic, size=(k, k, 1), mode="nearest")


@functools.lru_cache(maxsize=None)
def canvas(seed, smooth=False):
    """dead leaves, PAIR_SHAPE and MARGIN px all round; smooth: under the binomial 1 4 6 4 1 twice, so that sampling it invents nothing"""
    from scipy.ndimage import convolve1d
    big = dead_leaves(np.random.default_rng(seed), PAIR_SHAPE[0] + 2 * MARGIN, PAIR_SHAPE[1] + 2 * MARGIN)
    w = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(2 if smooth else 0):                                               # (sigma about 1.4 px: the cubic taps then resample it to a few 1e-4)
        big = convolve1d(convolve1d(big, w, axis=0, mode="nearest"), w, axis=1, mode="nearest")
    big.setflags(write=False)
    return big


@functools.lru_cache(maxsize=None)
def pair(model, blur=0, gain=1.0, bias=0.0, sigma=0.002, smooth=False):
    """(moving, fixed, M true) float32: fixed is the middle of the canvas; moving = (fixed - bias) / gain as seen through TRUE[model],
    sampled from the canvas itself (blurred by a box of `blur` px first), so that no border is invented; noise of `sigma` on both.
    smooth: from the smoothed canvas (the photometric test: the cubic taps soften the hard edges of plain dead leaves in `moving`
    alone, which is a difference of contrast between the frames that the gain then rightly absorbs -- (gain, bias) would not be
    the truth of such a pair).  Shared by the tests: do not write to it."""
    M = TRUE[model]
    big = canvas(11, smooth)
    rng = np.random.default_rng(500 + len(model) + 10 * blur)
    H, W = PAIR_SHAPE
    fixed = big[MARGIN:MARGIN + H, MARGIN:MARGIN + W] + rng.normal(0, sigma, (H, W, 3))
    src = box_blur(big, blur) if blur else big
    moving = (warp(src, translation(MARGIN, MARGIN) @ np.linalg.inv(M), (H, W)) - bias) / gain + rng.normal(0, sigma, (H, W, 3))
    moving, fixed = np.ascontiguousarray(moving, dtype=np.float32), np.ascontiguousarray(fixed, dtype=np.float32)
    moving.setflags(write=False); fixed.setflags(write=False)
    return moving, fixed, M


@functools.lru_cache(maxsize=None)
def psf_pair(K=9):
    """(sharp, blurred, off, M) float64 for estimate_psf(register=): dead leaves under the binomial 1 2 1 (about the aperture of a pixel),
    blurred by a K px box plus noise of sigma 0.002, and the sharp frame as seen through M, 1 degree and (2.3, -1.6) px off"""
    from scipy.ndimage import convolve1d
    rng = np.random.default_rng(77)
    H, W = PAIR_SHAPE
    big = dead_leaves(rng, H + 2 * MARGIN, W + 2 * MARGIN)
    w = np.array([1.0, 2.0, 1.0]) / 4.0
    big = convolve1d(convolve1d(big, w, axis=0, mode="nearest"), w, axis=1, mode="nearest")
    blurred = box_blur(big, K)[MARGIN:MARGIN + H, MARGIN:MARGIN + W] + rng.normal(0, 0.002, (H, W, 3))
    sharp = big[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    M = about_centre((H, W), 1.0, 1.0, 2.3, -1.6)
    off = warp(big, translation(MARGIN, MARGIN) @ np.linalg.inv(M), (H, W))
    for a in (sharp, blurred, off):
        a.setflags(write=False)
    return sharp, blurred, off, M


RECOVERY = [(model, blur) for model in MODELS for blur in (0, 9)]
RECOVERY_BOUND = {("translation", 0): 0.1, ("translation", 9): 0.2, ("affine", 0): 0.1, ("affine", 9): 0.2, ("homography", 0): 0.1, ("homography", 9): 0.5}


@functools.lru_cache(maxsize=None)
def recovered(model, blur, dtype=np.float64):
    """(Alignment, steps per level) of the specification on a recovery pair, at the defaults"""
    moving, fixed, _ = pair(model, blur)
    per = []
    res = align(moving, fixed, model, dtype=dtype, per_level=per)
    return res, tuple(per)


# align_sums on the device: (fixed shape, moving shape, window)
SUMS_CASES = [((31, 33), (31, 33), None), ((64, 96), (64, 96), None), ((97, 121), (97, 121), None), ((97, 121), (97, 121), (5, 90, 9, 108)),
              ((64, 96), (80, 100), None)]
SUMS_GAIN, SUMS_BIAS = 1.1, -0.03
# ... and where the reduction over the tiles (k_img_al_reduce: 1024 lanes, parts = 1024 // ns per slot entry, eight tiles a trip while
# t + 7 parts < tiles, then one at a time) runs both loop forms: (frame, model, photometric), one per variant with 8 parts < tiles < 9 parts --
# every lane makes one eight-wide trip, the lanes below tiles - 8 parts a tail step as well -- and one where the lanes make ten trips, or nine and a tail of seven.
# ns = 7, 16, 29, 46, 46, 67; tests/test_trip_counts.py holds the shapes to this.
SUMS_TRIP_CASES = [((1100, 1070), "translation", False), ((720, 710), "translation", True), ((530, 520), "affine", False), ((430, 400), "affine", True),
                   ((430, 400), "homography", False), ((340, 330), "homography", True), ((1100, 1070), "homography", True)]


@functools.lru_cache(maxsize=None)
def sums_trip_reference(case, dtype=np.float64):
    """(moving, fixed, M, (S, g, sum r^2, count)) of a trip case, computed once"""
    shape, model, photometric = SUMS_TRIP_CASES[case]
    moving, fixed = sums_pair(shape, shape)
    M = sums_matrix(shape, shape, None)
    ref = sums_on_window(moving, fixed, M, None, model, photometric, SUMS_GAIN, SUMS_BIAS, dtype)
    for a in ref[:2]:
        a.setflags(write=False)
    return moving, fixed, M, ref


def sums_matrix(shape_f, shape_m, window):
    """a non-identity M for a sums case: a small rotation, scale, shift and projective row that keeps most of the box inside moving"""
    M = about_centre(shape_f, 1.5, 1.02, 1.3, -0.8, h=(4e-5, -3e-5))
    grow = translation((shape_m[1] - shape_f[1]) / 2.0, (shape_m[0] - shape_f[0]) / 2.0)
    return grow @ M


@functools.lru_cache(maxsize=None)
def sums_pair(shape_f, shape_m):
    """(moving, fixed) float32 for a sums case: two views of one dead-leaves scene, a few pixels apart"""
    rng = np.random.default_rng(900 + shape_f[0] + 3 * shape_m[1])
    Hc, Wc = max(shape_f[0], shape_m[0]) + 8, max(shape_f[1], shape_m[1]) + 8
    from scipy.ndimage import uniform_filter
    big = uniform_filter(dead_leaves(rng, Hc, Wc, n=150), size=(3, 3, 1), mode="nearest")
    fixed = np.ascontiguousarray(big[4:4 + shape_f[0], 4:4 + shape_f[1]] + rng.normal(0, 0.002, shape_f + (3,)), dtype=np.float32)
    moving = np.ascontiguousarray(big[2:2 + shape_m[0], 5:5 + shape_m[1]] * 0.9 + 0.02 + rng.normal(0, 0.002, shape_m + (3,)), dtype=np.float32)
    fixed.setflags(write=False); moving.setflags(write=False)
    return moving, fixed


def sums_on_window(moving, fixed, M, window, model, photometric, gain=1.0, bias=0.0, dtype=np.float64):
    """what DeviceImage.align_sums returns: the sums at full resolution for a full-frame M, on the window's plane"""
    y0, y1, x0, x1 = (0, fixed.shape[0], 0, fixed.shape[1]) if window is None else window
    T, I = luma(np.asarray(fixed)[y0:y1, x0:x1], dtype), luma(moving, dtype)
    A = to_frame(np.asarray(M, dtype=np.float64) @ translation(x0, y0), T.shape, I.shape)
    return sums(T, I, A, model, photometric, gain, bias, dtype)


# warp on the device: (source shape, output shape)
WARP_CASES = [((5, 7), (5, 7)), ((33, 65), (33, 65)), ((40, 52), (61, 47)), ((16, 2040), (16, 2040)), ((2040, 16), (2040, 16))]


def warp_matrices(shape_s, shape_o):
    sy, sx = (shape_s[0] - 1) / max(shape_o[0] - 1, 1), (shape_s[1] - 1) / max(shape_o[1] - 1, 1)
    fit = np.diag([sx, sy, 1.0])
    affine = fit @ about_centre(shape_o, 3.0, 0.97, 0.6, -0.4)
    homography = fit @ about_centre(shape_o, -2.0, 1.04, -0.3, 0.7, h=(2e-4 / max(1, shape_o[1] / 64), -1e-4 / max(1, shape_o[0] / 64)))
    return {"affine": affine, "homography": homography}


@functools.lru_cache(maxsize=None)
def warp_source(shape):
    rng = np.random.default_rng(70 + shape[0] + 5 * shape[1])
    src = np.ascontiguousarray(dead_leaves(rng, shape[0], shape[1], n=120) + rng.normal(0, 0.01, shape + (3,)), dtype=np.float32)
    src.setflags(write=False)
    return src
