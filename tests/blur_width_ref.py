"""Blur width from the autocorrelation of the picture's derivatives in numpy, the specification of ics_img_blur_profile /
DeviceImage.blur_profile (csrc/ics_img_blurwidth.hip) and of the rule lib._native.blur_extent / blur_width_from, with the dtype as a
parameter: float64 is the oracle of the tests, float32 the restatement of the device's arithmetic.

    Y       = (R + G + B) * (1 / 3), rounded once per operation
    dx[y,x] = Y[y,x+1] - Y[y,x], dy[y,x] = Y[y+1,x] - Y[y,x], both pixels inside the window (y0, y1, x0, x1), half-open
    Sx(l)   = sum over the window of dx[y,x] dx[y,x+l] for every pair inside it, nx(l) the number of such pairs, Ax(l) = Sx(l) / nx(l)
              (0 where nx(l) = 0), l = 0 .. L; Ay(l) likewise with dy along y

float32: luma, differences and products are float32; the products of the pairs whose first element lies in one ACTH x ACTW tile of the
window (tiles counted from the window's origin) are summed in float32, the tiles in float64 in row-major order; the division is float64.

The derivative of a sharp picture is close to white along its axis, so the profile of a blurred one is the autocorrelation of the PSF's
projection on that axis: a triangle for a box, a disc or a motion line.  extent(A) reads its base:

    P       = A[2] + 2 (A[2] - A[3]): the peak extrapolated from lags 2 and 3 (white noise in the picture adds to A[0] and, through the
              shared pixel of neighbouring differences, to A[1], and to no other lag)
    h       = the largest lag with A[l] >= P / 2 for every 2 <= l <= h (1 if there is none)
    h >= 3  : the least-squares line through (l, A[l]), l = 2 .. h, and the lag at which it crosses zero; SATURATED if the slope is not
              negative or the crossing lies above L = len(A) - 1
    h < 3   : the first l >= 2 with A[l] <= 0.05 P (SATURATED if there is none)
    1 where P is not above 0 or the profile has fewer than 4 lags

blur_width(Ax, Ay) = max(3, the smallest odd integer >= max(extent_x, extent_y) - 1e-9)."""
import math

import numpy as np

ACTH, ACTW = 32, 64          # the kernel's tile (csrc/ics_img_blurwidth.hip ACTH, ACTW: asserted equal in tests/test_blur_width_isa.py)
MAX_LAG = 128
SATURATED = math.inf


def luma(pic, dtype=np.float64):
    c = np.asarray(pic, dtype=dtype)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("H x W x 3 expected, got %s" % (c.shape,))
    y = ((c[..., 0] + c[..., 1]) + c[..., 2]) * dtype(1.0 / 3.0)
    assert y.dtype == dtype
    return y


def _axis_profile(d, axis, L, dtype):
    """(A, n) of lags 0 .. L of the differences d along `axis` (1: x, 0: y)"""
    A, n = np.zeros(L + 1, np.float64), np.zeros(L + 1, np.int64)
    for l in range(L + 1):
        m = d.shape[axis] - l
        if m <= 0 or d.size == 0:
            continue
        prod = d[:, :m] * d[:, l:] if axis == 1 else d[:m, :] * d[l:, :]
        assert prod.dtype == dtype
        n[l] = prod.size
        if dtype == np.float64:
            A[l] = prod.sum() / n[l]
            continue
        s = np.float64(0.0)                       # a pair belongs to the tile of its first element; tiles in row-major order
        for ty in range(0, prod.shape[0], ACTH):
            for tx in range(0, prod.shape[1], ACTW):
                s += np.float64(np.sum(prod[ty:ty + ACTH, tx:tx + ACTW], dtype=np.float32))
        A[l] = s / np.float64(n[l])
    return A, n


def profiles(pic, window, L, dtype=np.float64):
    """(Ax, Ay, nx, ny) of lags 0 .. L over the window (y0, y1, x0, x1); the profiles are float64 arrays, the counts int64"""
    y0, y1, x0, x1 = (int(v) for v in window)
    H, W = np.asarray(pic).shape[:2]
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError("window %r (half-open, not empty, inside the %d x %d frame)" % (window, H, W))
    L = int(L)
    if not 0 <= L <= MAX_LAG:
        raise ValueError("L = %d (0 .. %d)" % (L, MAX_LAG))
    Y = luma(pic, dtype)[y0:y1, x0:x1]
    Ax, nx = _axis_profile(Y[:, 1:] - Y[:, :-1], 1, L, dtype)
    Ay, ny = _axis_profile(Y[1:, :] - Y[:-1, :], 0, L, dtype)
    return Ax, Ay, nx, ny


def extent(A):
    """the base of the triangle one profile describes, in pixels; SATURATED where it does not end inside the profile"""
    A = np.asarray(A, dtype=np.float64)
    L = A.size - 1
    if A.size < 4:
        return 1.0
    P = A[2] + 2.0 * (A[2] - A[3])
    if not P > 0:
        return 1.0
    h = 1
    while h + 1 <= L and A[h + 1] >= 0.5 * P:
        h += 1
    if h >= 3:
        l = np.arange(2, h + 1, dtype=np.float64)
        a = A[2:h + 1]
        lm, am = l.mean(), a.mean()
        slope = float(((l - lm) * (a - am)).sum() / ((l - lm) ** 2).sum())
        if not slope < 0:
            return SATURATED
        cross = float(lm - am / slope)
        return SATURATED if cross > L else cross
    for l in range(2, L + 1):
        if A[l] <= 0.05 * P:
            return float(l)
    return SATURATED


def blur_width(Ax, Ay):
    """the odd PSF size deblur_module takes; ValueError where a profile is saturated"""
    e = max(extent(Ax), extent(Ay))
    if e == SATURATED:
        raise ValueError("saturated profile: the blur is wider than the lags reach")
    n = int(math.ceil(e - 1e-9))
    return max(3, n if n % 2 else n + 1)
