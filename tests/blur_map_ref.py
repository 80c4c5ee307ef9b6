"""Local blur width of a picture in numpy, the specification of ics_img_blur_map / DeviceImage.blur_map (csrc/ics_img_blurmap.hip)
and of the host rules lib._native.blur_map_taps / blur_map_edge / blur_map_fill / blur_map_box_sigma, with the dtype as a parameter:
float64 is the oracle, float32 restates the device's arithmetic (every operation rounded once, no FMA, the sums in the kernel's order)
and is held to the bits.  Zhuo and Sim's gradient-ratio defocus map: the luma smoothed by two Gaussians sa < sb; at an edge pixel of
a step blurred by a Gaussian of s the gradient magnitudes stand in the ratio R = sqrt((s^2 + sb^2) / (s^2 + sa^2)), hence
s^2 = (sb^2 - R^2 sa^2) / (R^2 - 1).

Over the half-open window (y0, y1, x0, x1), every coordinate clamped to the window:
  Y        = ((R + G) + B) * float32(1 / 3)
  taps     : g_s[i] = exp(-i^2 / (2 s^2)), i = -r .. r, r = ceil(float32(3) * float32(s)) (the product in float32, so that 8 / 3 gives 8),
             s = the sigma as float32 carries it, the exponentials (math.exp) summed in ascending i and divided in double; float32:
             rounded to float32 after that
  S_s      = the rows pass, then the columns pass: acc = 0, acc = acc + g[i] * v for i ascending
  gx, gy   = 0.5 * (S[y, x+1] - S[y, x-1]), 0.5 * (S[y+1, x] - S[y-1, x])
  A, B     = sqrt(gx gx + gy gy) of S_sa, of S_sb
  sector   : of (ax, ay), the gradient of S_sa: 0 if |ay| <= T |ax|; 2 if |ax| <= T |ay|; else 1 if ax * ay > 0, else 3, T = 0.41421357f
             (ics_img_edge_mask's rule); neighbour offsets (dy, dx) = (0, 1), (1, 1), (1, 0), (1, -1)
  kept     : A > A[y+dy, x+dx] and A >= A[y-dy, x-dx]; A >= edge; B > 0; R = A / B > 1;
             s2 = (sb^2 - (R R) sa^2) / (R R - 1) <= max_sigma^2.  Its value: sigma = sqrt(max(s2, 0))
  cells    : CELL x CELL pixels from the window's origin, ragged at the far edges: weight = sum A, moment = sum A sigma, count over the
             kept pixels, a pixel that is not kept adding exactly 0; a row left to right, the row sums top to bottom.  bad = the
             number of pixels of the window whose luma is not finite
"""
import math

import numpy as np

CELL = 16
MAX_RADIUS = 8
SECTOR_T = np.float32(0.41421357)
OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))


def radius(s):
    return int(math.ceil(float(np.float32(3.0) * np.float32(s))))


def taps(s, dtype=np.float64):
    """the normalised Gaussian taps of sigma s, 2 r + 1 of them"""
    s = float(np.float32(s))
    r = radius(s)
    g = [math.exp(-(i * i) / (2.0 * s * s)) for i in range(-r, r + 1)]
    tot = 0.0
    for v in g:
        tot += v
    return np.array([v / tot for v in g], np.float64).astype(dtype)


def check_sigmas(sigmas):
    sa, sb = (float(np.float32(v)) for v in sigmas)
    if not (0.5 <= sa < sb) or radius(sb) > MAX_RADIUS:
        raise ValueError("sigmas %r" % (sigmas,))
    return sa, sb


def luma(img, dtype):
    a = np.asarray(img, np.float32).astype(dtype)
    return ((a[..., 0] + a[..., 1]) + a[..., 2]) * dtype(np.float32(1.0 / 3.0))


def _smooth(Y, g, dtype):
    h, w = Y.shape
    r = (g.size - 1) // 2
    ys, xs = np.arange(h), np.arange(w)
    acc = np.zeros_like(Y)
    for i in range(-r, r + 1):
        acc = acc + g[i + r] * Y[:, np.clip(xs + i, 0, w - 1)]
    out = np.zeros_like(Y)
    for i in range(-r, r + 1):
        out = out + g[i + r] * acc[np.clip(ys + i, 0, h - 1), :]
    return out


def _grad(S, dtype):
    h, w = S.shape
    ys, xs = np.arange(h), np.arange(w)
    half = dtype(0.5)
    gx = half * (S[:, np.clip(xs + 1, 0, w - 1)] - S[:, np.clip(xs - 1, 0, w - 1)])
    gy = half * (S[np.clip(ys + 1, 0, h - 1), :] - S[np.clip(ys - 1, 0, h - 1), :])
    return gx, gy, np.sqrt(gx * gx + gy * gy)


def pixels(img, sigmas=(1.0, 2.0), edge=0.02, max_sigma=8.0, window=None, dtype=np.float64):
    """(A, sigma, kept, Y) of the window: the gradient magnitude of S_sa, the blur width (-1 where not kept) and the kept set"""
    img = np.asarray(img, np.float32)
    if window is not None:
        y0, y1, x0, x1 = window
        img = img[y0:y1, x0:x1]
    sa, sb = check_sigmas(sigmas)
    with np.errstate(all="ignore"):
        Y = luma(img, dtype)
        h, w = Y.shape
        ax, ay, A = _grad(_smooth(Y, taps(sa, dtype), dtype), dtype)
        _, _, B = _grad(_smooth(Y, taps(sb, dtype), dtype), dtype)
        T = dtype(SECTOR_T)
        fx, fy = np.abs(ax), np.abs(ay)
        sec = np.where(fy <= T * fx, 0, np.where(fx <= T * fy, 2, np.where(ax * ay > 0, 1, 3)))
        ys, xs = np.mgrid[0:h, 0:w]
        dy = np.array([o[0] for o in OFFSETS])[sec]
        dx = np.array([o[1] for o in OFFSETS])[sec]
        fwd = A[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
        back = A[np.clip(ys - dy, 0, h - 1), np.clip(xs - dx, 0, w - 1)]
        e, ms = dtype(np.float32(edge)), dtype(np.float32(max_sigma))
        sa2, sb2 = dtype(sa) * dtype(sa), dtype(sb) * dtype(sb)
        R = A / B
        R2 = R * R
        s2 = (sb2 - R2 * sa2) / (R2 - dtype(1))
        kept = (A > fwd) & (A >= back) & (A >= e) & (B > 0) & (R > 1) & (s2 <= ms * ms)
        sigma = np.where(kept, np.sqrt(np.maximum(s2, dtype(0))), dtype(-1)).astype(dtype)
    return A, sigma, kept, Y


def cells(A, sigma, kept, Y, dtype=np.float64):
    """(weight, moment, count, bad): the cell sums in the kernel's order, bad the window's total"""
    h, w = A.shape
    rows, cols = -(-h // CELL), -(-w // CELL)
    with np.errstate(all="ignore"):
        wv = np.zeros((rows * CELL, cols * CELL), dtype)
        mv = np.zeros_like(wv)
        wv[:h, :w] = np.where(kept, A, dtype(0))
        mv[:h, :w] = np.where(kept, A * sigma, dtype(0))

        def total(v):
            v = v.reshape(rows, CELL, cols, CELL)
            rs = np.zeros((rows, CELL, cols), dtype)
            for k in range(CELL):
                rs = rs + v[:, :, :, k]
            out = np.zeros((rows, cols), dtype)
            for k in range(CELL):
                out = out + rs[:, k, :]
            return out
        weight, moment = total(wv), total(mv)
    kc = np.zeros((rows * CELL, cols * CELL), np.int32)
    kc[:h, :w] = kept
    count = kc.reshape(rows, CELL, cols, CELL).sum(axis=(1, 3)).astype(np.int32)
    return weight, moment, count, int((~np.isfinite(Y)).sum())


def blur_map(img, sigmas=(1.0, 2.0), edge=0.02, max_sigma=8.0, window=None, dtype=np.float64):
    """dict(weight, moment, count, bad, pixels, kept): what the kernel stores, and the sparse plane"""
    A, sigma, kept, Y = pixels(img, sigmas, edge, max_sigma, window, dtype)
    weight, moment, count, bad = cells(A, sigma, kept, Y, dtype)
    return dict(weight=weight, moment=moment, count=count, bad=bad, pixels=sigma, kept=kept)


# ---- the host rules (lib._native restates them) ---------------------------------------------------------------------------------------
def cell_sigma(weight, moment, count):
    """moment / weight in double, NaN where count == 0"""
    weight, moment = np.asarray(weight, np.float64), np.asarray(moment, np.float64)
    out = np.full(weight.shape, np.nan)
    ok = np.asarray(count) > 0
    out[ok] = moment[ok] / weight[ok]
    return out


def filled(sigma, weight):
    """normalised convolution on the cell grid: an empty cell (sigma NaN) takes the weight-weighted mean of the nearest ring (Chebyshev
    distance) of cells that holds any; a grid without any stays NaN"""
    sigma, weight = np.asarray(sigma, np.float64), np.asarray(weight, np.float64)
    out = sigma.copy()
    have = ~np.isnan(sigma)
    if not have.any():
        return out
    rows, cols = sigma.shape
    for i, j in zip(*np.nonzero(~have)):
        for d in range(1, max(rows, cols)):
            num = den = 0.0
            for y in range(max(i - d, 0), min(i + d, rows - 1) + 1):
                for x in range(max(j - d, 0), min(j + d, cols - 1) + 1):
                    if max(abs(y - i), abs(x - j)) == d and have[y, x]:
                        num += weight[y, x] * sigma[y, x]
                        den += weight[y, x]
            if den > 0:
                out[i, j] = num / den
                break
    return out


def box_sigma(sigma, weight, count, side, extent):
    """the weight-weighted mean over the n x n cells, n = side // CELL, of every candidate box of window_scores: box (i, j) has its
    origin CELL i, CELL j pixels from the region's origin and takes the cells [i, i + n) x [j, j + n) of the map of that region,
    (extent - side) // CELL + 1 boxes a side; NaN where a box holds no kept pixel.  extent: (height, width) of the region"""
    have = np.asarray(count) > 0
    wgt = np.where(have, np.asarray(weight, np.float64), 0.0)
    mom = np.where(have, wgt * np.where(have, np.asarray(sigma, np.float64), 0.0), 0.0)
    n = side // CELL
    nci, ncj = (extent[0] - side) // CELL + 1, (extent[1] - side) // CELL + 1
    out = np.full((nci, ncj), np.nan)
    for i in range(nci):
        for j in range(ncj):
            if have[i:i + n, j:j + n].any():
                out[i, j] = mom[i:i + n, j:j + n].sum() / wgt[i:i + n, j:j + n].sum()
    return out


def edge_from_noise(sigma_noise, sa, strength=5.0):
    """strength times the standard deviation of one gradient component of S_sa under white noise of sigma_noise per channel"""
    g = taps(sa, np.float64)
    gp = np.concatenate(([0.0, 0.0], g, [0.0, 0.0]))
    d = 0.5 * (gp[:-2] - gp[2:])                                           # 0.5 (g[i-1] - g[i+1]), i = -r - 1 .. r + 1
    return float(strength) * (float(sigma_noise) / math.sqrt(3.0)) * math.sqrt(float((g * g).sum()) * float((d * d).sum()))
