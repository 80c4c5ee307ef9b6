"""The choice of the PSF-estimation window in numpy, the specification of ics_img_window_scores / DeviceImage.window_scores
(csrc/ics_img_mask.hip) and of lib.utils.best_mask, with the dtype as a parameter: float64 is the oracle of the tests, float32 the
restatement of the device's arithmetic.

    usable   : |v| < clip for all three channels (NaN and inf are never usable; clip = inf keeps every finite pixel)
    Y        = (R + G + B) * (1 / 3), rounded once per operation
    dx[y,x]  = Y[y,x+1] - Y[y,x] where x + 1 < x1 and both pixels are usable, else 0; dy[y,x] = Y[y+1,x] - Y[y,x] likewise with y + 1 < y1
               (region (y0, y1, x0, x1), half-open; nothing outside it is looked at)
    cells    : CELL x CELL pixels, n = size // CELL, off = (size - CELL n) // 2, the grid anchored at (y0 + off, x0 + off); per cell
               Sxx = sum dx dx, Syy = sum dy dy, Sxy = sum dx dy and the number of unusable pixels
    box (i,j): origin (y0 + CELL i, x0 + CELL j), i = 0 .. (y1 - y0 - size) // CELL, j likewise, scored over the cells
               [i, i + n) x [j, j + n): trace = (Sxx + Syy) / (CELL n)^2,
               score = max(0, (Sxx + Syy - sqrt((Sxx - Syy)^2 + 4 Sxy^2)) / 2 / (CELL n)^2), clipped = the count
    choice   : the largest score, ties to the lowest i, then the lowest j

float32: luma, differences, products and the sums inside a cell are float32; the cells of a box are added in float64 in row-major order,
and the score is float64 arithmetic."""
import numpy as np

CELL = 16                    # csrc/ics_img_mask.hip MKCELL == include/ics_hip.h ICS_IMG_MASK_CELL
TILE = 64                    # the cell kernel's tile side in pixels (csrc/ics_img_mask.hip MKT: asserted equal in tests/test_mask_isa.py)


def grid(region, size):
    """(n, off, candidates along y, candidates along x) of a region (y0, y1, x0, x1) and a box side; ValueError where there is no candidate"""
    y0, y1, x0, x1 = (int(v) for v in region)
    size = int(size)
    if size < CELL:
        raise ValueError("size = %d (at least %d)" % (size, CELL))
    if y1 - y0 < size or x1 - x0 < size:
        raise ValueError("region %r is smaller than the box (size = %d)" % (region, size))
    n = size // CELL
    return n, (size - CELL * n) // 2, (y1 - y0 - size) // CELL + 1, (x1 - x0 - size) // CELL + 1


def cells(pic, region, size, clip, dtype=np.float64):
    """(Sxx, Syy, Sxy, count) per cell: three arrays of `dtype` and one of int64, cells along y x cells along x"""
    pic = np.asarray(pic)
    if pic.ndim != 3 or pic.shape[2] != 3:
        raise ValueError("H x W x 3 expected, got %s" % (pic.shape,))
    y0, y1, x0, x1 = (int(v) for v in region)
    H, W = pic.shape[:2]
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError("region %r (half-open, not empty, inside the %d x %d frame)" % (region, H, W))
    if not clip > 0:
        raise ValueError("clip = %r (above 0)" % (clip,))
    n, off, nci, ncj = grid(region, size)
    c = np.asarray(pic[y0:y1, x0:x1], dtype=dtype)
    with np.errstate(invalid="ignore"):
        usable = (np.abs(pic[y0:y1, x0:x1]) < np.float32(clip)).all(axis=2)      # (the device takes clip as a float32)
    with np.errstate(invalid="ignore", over="ignore"):
        Y = ((c[..., 0] + c[..., 1]) + c[..., 2]) * dtype(1.0 / 3.0)
        assert Y.dtype == dtype
        dx, dy = np.zeros_like(Y), np.zeros_like(Y)
        dx[:, :-1] = np.where(usable[:, 1:] & usable[:, :-1], Y[:, 1:] - Y[:, :-1], dtype(0))
        dy[:-1, :] = np.where(usable[1:, :] & usable[:-1, :], Y[1:, :] - Y[:-1, :], dtype(0))
    ncy, ncx = nci - 1 + n, ncj - 1 + n

    def per_cell(a, kind):
        a = a[off:off + CELL * ncy, off:off + CELL * ncx].reshape(ncy, CELL, ncx, CELL).transpose(0, 2, 1, 3).reshape(ncy, ncx, CELL * CELL)
        return np.sum(a, axis=2, dtype=kind)

    out = tuple(per_cell(p, dtype) for p in (dx * dx, dy * dy, dx * dy))
    assert all(a.dtype == dtype for a in out)
    return out + (per_cell(~usable, np.int64),)


def scores(pic, region, size, clip, dtype=np.float64):
    """(score, trace, clipped) of every candidate: two float64 maps and an int64 one, candidates along y x candidates along x"""
    n, _, nci, ncj = grid(region, size)
    sxx, syy, sxy, bad = cells(pic, region, size, clip, dtype)
    S = [np.zeros((nci, ncj), np.float64) for _ in range(3)]
    B = np.zeros((nci, ncj), np.int64)
    for a in range(n):                                # row-major cell order, every addition in float64
        for b in range(n):
            for acc, src in zip(S, (sxx, syy, sxy)):
                acc += src[a:a + nci, b:b + ncj].astype(np.float64)
            B += bad[a:a + nci, b:b + ncj]
    area = float(CELL * n) ** 2
    tr, df = S[0] + S[1], S[0] - S[1]
    score = 0.5 * (tr - np.sqrt(df * df + 4.0 * (S[2] * S[2]))) / area
    return np.where(score > 0, score, 0.0), tr / area, B


def choice(pic, region, size, clip, dtype=np.float64):
    """(i, j, score, trace, clipped) of the chosen candidate"""
    score, trace, bad = scores(pic, region, size, clip, dtype)
    i, j = np.unravel_index(int(np.argmax(score)), score.shape)      # (the first of equal maxima in row-major order: lowest i, then lowest j)
    return int(i), int(j), float(score[i, j]), float(trace[i, j]), int(bad[i, j])


def center(pic, mask_size, clip, region=None):
    """what lib.utils.best_mask returns for a frame: (center_y, center_x, score, trace, clipped fraction)"""
    half = int(mask_size) // 2
    H, W = np.asarray(pic).shape[:2]
    region = (0, H, 0, W) if region is None else region
    i, j, score, trace, bad = choice(pic, region, 2 * half + 1, clip)
    n = (2 * half + 1) // CELL
    return region[0] + CELL * i + half, region[2] + CELL * j + half, score, trace, bad / float(CELL * n) ** 2
