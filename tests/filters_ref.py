"""Exact references for the stand-alone filters (csrc/ics_filters.hip, csrc/ics_img_filters.hip), numpy only, and the case lists of
tests/test_filters_edges.py (CPU: the references are right) and tests/test_gpu_filters_edges.py (GPU: the kernels are right).

On small integers every correct convolution gives the same bits, whatever its summation order or use of FMA: each product and
each partial sum is an integer below 2^52 (float64) or 2^23 (float32), and a scale by a power of two only moves the exponent.  So
the device is compared with `np.array_equal`, and an error of one tap at one pixel is as visible as a wrong frame.

LDS formulas, restated from the comments and launchers of the two .hip files (bytes of dynamic LDS per workgroup):
    float64 convolution   (32 + KH - 1) * (32 + KW - 1) * 8                       32 x 32 tile + halo
    float64 bilateral     (32 + 2 r)^2 * 8
    float32 rows / 2-D    (16 + KH - 1) * (256 + 12 * ceil(KW / 4) + 4) * 4       16 rows of 256 flat floats + halo
    float32 columns       (32 + KH - 1) * 256 * 4                                 32 rows of 256 flat floats + halo
    float32 bilateral     (16 + 2 r) * (4 nq + (4 nq >> 5) + 1) * 4, nq = (256 + 6 r + 3) // 4     one pad float per 32
A launch above LDS_OPT_IN needs hipFuncSetAttribute first; one above LDS_LIMIT is refused by the host (ICS_ENOSUP).
"""
import math

import numpy as np

LDS_OPT_IN = 64 * 1024
LDS_LIMIT = 160 * 1024

# exactness budgets: bits of the picture, bits of the taps, bits of the mantissa that an integer sum may fill
F64_BITS = (8, 8, 52)
F32_BITS = (4, 3, 23)


# ---- LDS sizes ---------------------------------------------------------------------------------------------------------------------
def lds_f64_conv(KH, KW):
    return (32 + KH - 1) * (32 + KW - 1) * 8


def lds_f64_bilateral(r):
    return (32 + 2 * r) ** 2 * 8


def lds_f32_rows(KH, KW):
    return (16 + KH - 1) * (256 + 12 * ((KW + 3) // 4) + 4) * 4


def lds_f32_cols(KH):
    return (32 + KH - 1) * 256 * 4


def lds_f32_bilateral(r):
    nq = (256 + 6 * r + 3) // 4
    return (16 + 2 * r) * (4 * nq + (4 * nq >> 5) + 1) * 4


# ---- budget ------------------------------------------------------------------------------------------------------------------------
def budget_bits(pic_bits, kern_bits, KH, KW):
    """bits of the largest sum of KH * KW products of a pic_bits-bit pixel and a kern_bits-bit tap"""
    return pic_bits + kern_bits + math.ceil(math.log2(KH * KW)) if KH * KW > 1 else pic_bits + kern_bits


def assert_budget(bits, KH, KW):
    pic_bits, kern_bits, mantissa = bits
    used = budget_bits(pic_bits, kern_bits, KH, KW)
    assert used <= mantissa, "a %d x %d kernel needs %d bits, the format holds %d: a mistake in the case list" % (KH, KW, used, mantissa)


# ---- case generators ---------------------------------------------------------------------------------------------------------------
def int_picture(H, W, bits, seed, channels=None):
    """integers in [0, 2^bits): H x W, or H x W x channels"""
    shape = (H, W) if channels is None else (H, W, channels)
    return np.random.default_rng([seed, H, W]).integers(0, 2 ** bits, shape, dtype=np.int64)


def int_kernel(KH, KW, bits, seed):
    """integers in [0, 2^bits), not an outer product whenever an outer product is possible (both sides above 1)"""
    rng = np.random.default_rng([seed, KH, KW])
    k = rng.integers(0, 2 ** bits, (KH, KW), dtype=np.int64)
    k[0, 0] = 2 ** bits - 1                      # never all zero
    if min(KH, KW) > 1:
        k[:2, :2] = [[2 ** bits - 1, 1], [1, 2]]   # a 2 x 2 minor that does not vanish
        assert np.linalg.matrix_rank(k.astype(np.float64)) > 1
    return k


def pow2_vector(n, top, rng):
    """integers in [1, top] whose largest entry is `top`, a power of two"""
    assert top >= 1 and top & (top - 1) == 0
    v = rng.integers(1, top + 1, n, dtype=np.int64)
    v[rng.integers(0, n)] = top
    return v


def int_outer_kernel(KH, KW, seed, bits=8):
    """np.outer(a, b), a and b integer vectors whose largest entries are powers of two, max(a) * max(b) = 2^(bits - 1): the host's
    rank-1 test (rank1_factors, csrc/ics_ops.hip) pivots on the largest element and divides a column by it; with a power-of-two
    pivot its factors, and the two 1-D passes, stay exact."""
    rng = np.random.default_rng([seed, KH, KW, 1])
    ta = 2 ** ((bits - 1) // 2)
    tb = 2 ** (bits - 1) // ta
    k = np.outer(pow2_vector(KH, ta, rng), pow2_vector(KW, tb, rng))
    assert k.max() == 2 ** (bits - 1) and k.min() >= 1
    return k


def shift_of(kern_int):
    """the power of two at or above the sum of the taps: kern / 2^shift is a window that sums to about 1"""
    return max(0, int(kern_int.sum()) - 1).bit_length()


# ---- references --------------------------------------------------------------------------------------------------------------------
def conv_symm_exact(src_int, kern_int):
    """scipy.signal.convolve2d(src, kern, mode="same", boundary="symm") on integers, in int64: symmetric pad of the two leading axes
    by (KH-1-cy, cy) and (KW-1-cx, cx), cy = (KH-1)//2, cx = (KW-1)//2, then out[i, j] = sum_pq k[p, q] ext[i + KH-1 - p, j + KW-1 - q].
    src: H x W or H x W x C (every channel on its own)."""
    src, k = np.asarray(src_int), np.asarray(kern_int)
    assert src.dtype.kind in "iu" and k.dtype.kind in "iu" and k.ndim == 2 and src.ndim in (2, 3)
    src, k = src.astype(np.int64), k.astype(np.int64)
    KH, KW = k.shape
    H, W = src.shape[:2]
    cy, cx = (KH - 1) // 2, (KW - 1) // 2
    ext = np.pad(src, ((KH - 1 - cy, cy), (KW - 1 - cx, cx)) + ((0, 0),) * (src.ndim - 2), mode="symmetric")
    out = np.zeros_like(src)
    for p in range(KH):
        for q in range(KW):
            if k[p, q]:
                out += k[p, q] * ext[KH - 1 - p: KH - 1 - p + H, KW - 1 - q: KW - 1 - q + W]
    return out


def representable(x, dtype):
    return bool(np.all(np.asarray(x, np.float64).astype(dtype).astype(np.float64) == x))


def usm_exact(src_int, kern_int, shift, amount, dtype=np.float64, conv=None):
    """src + (src - conv / 2^shift) * amount in float64, exact for a dyadic `amount`; asserts that the blur, the difference and the
    result are numbers of `dtype`, so that a device working in `dtype` has nothing to round.  conv: conv_symm_exact(src_int, kern_int)
    where the caller has it already."""
    assert float(amount) * 4 == int(amount * 4), "amount must be a multiple of 1/4"
    src = np.asarray(src_int).astype(np.float64)
    blur = (conv_symm_exact(src_int, kern_int) if conv is None else conv).astype(np.float64) / 2.0 ** shift
    diff = src - blur
    out = src + diff * amount
    limit = 2.0 ** 52
    for v in (blur, diff, out):       # all three are integers / 2^(shift + 2) well below 2^52: float64 held them exactly
        assert np.all(np.abs(v) * 2.0 ** (shift + 2) < limit) and np.all(v * 2.0 ** (shift + 2) == np.rint(v * 2.0 ** (shift + 2)))
        assert representable(v, dtype), "not exact in %s: a mistake in the case list" % np.dtype(dtype).name
    return out


def box_mean(src, radius, dtype):
    """symmetric pad by `radius`, integer window sum, ONE division by (2 r + 1)^2 in `dtype`: what the bilateral filter is when both of
    its weights are exactly 1.  src: H x W or H x W x C integers."""
    src = np.asarray(src)
    assert src.dtype.kind in "iu"
    D = 2 * radius + 1
    s = conv_symm_exact(src, np.ones((D, D), np.int64))
    assert s.max() < 2 ** (np.finfo(dtype).nmant + 1)
    return s.astype(dtype) / dtype(D * D)


# ---- case lists (shared by the CPU and the GPU file) -------------------------------------------------------------------------------
# 3a: float64 convolution and USM
F64_FRAMES = [(1, 1), (1, 65), (65, 1), (3, 5), (31, 33), (32, 32), (33, 64), (64, 65)]
F64_KERNELS = [(1, 1), (1, 7), (7, 1), (3, 3), (4, 6), (6, 4), (2, 31), (9, 7), (15, 15)]
USM_AMOUNTS = [0.5, -0.25, 1.5]
NAN_FRAME_F64, NAN_FRAME_F32, NAN_KERNEL = (33, 64), (17, 171), (9, 7)

# 3b: float64 above 64 KB of LDS and at the limit; (KH, KW, route, LDS bytes of the 2-D launch or None, accepted)
F64_LDS_FRAMES = [(33, 40), (70, 66)]
F64_LDS_CASES = [(59, 59, "2d", 64800, True), (61, 61, "2d", 67712, True), (112, 112, "2d", 163592, True), (113, 113, "2d", None, False),
                 (111, 111, "rank1", None, True)]
F64_LDS_BILATERAL = [(29, 64800, True), (30, 67712, True), (55, 161312, True), (56, None, False)]

# 3c: bilateral as a box mean
F64_BOX_RADII = [0, 1, 3, 10]
F64_BOX_WRAP = [(5, (3, 5)), (20, (3, 5)), (5, (1, 65)), (20, (1, 65))]     # the radius exceeds the frame: reflection more than once
F32_BOX_FRAMES = [(1, 1), (17, 85), (16, 86), (33, 171), (5, 7)]
F32_BOX_RADII = [(0, None), (1, None), (5, None), (14, 61776), (15, 66056), (34, 159600)]
F32_BOX_REFUSED = 35

# 3d: float64 bilateral with real weights at the new radii
F64_BILATERAL_REAL = [29, 30, 55]

# 3e: float32 convolution and USM on resident frames
F32_FRAMES = [(1, 1), (1, 2), (15, 85), (16, 86), (17, 171), (31, 172), (32, 87), (33, 5)]
F32_BIG_FRAMES = [(33, 5), (17, 171)]
F32_KERNELS_2D = [(3, 3), (4, 6), (2, 31), (13, 15)]          # on every frame
F32_ABOVE_OPT_IN = 32                                          # smallest square with (15 + K) * (260 + 12 * ceil(K / 4)) * 4 > 65 536
F32_KERNELS_2D_BIG = [(F32_ABOVE_OPT_IN, F32_ABOVE_OPT_IN, 66928), (71, 71, 163744)]   # on F32_BIG_FRAMES
F32_KERNEL_REFUSED = (73, 73)
F32_COLS_ONLY = [(33, 65536), (35, 67584), (129, 163840)]      # K x 1, on F32_COLS_FRAMES
F32_COLS_FRAMES = [(1, 2), (33, 5), (17, 171)]
F32_KERNELS_RANK1 = [(3, 3), (4, 6), (2, 31), (13, 15)]       # on every frame
F32_KERNELS_RANK1_BIG = [(35, 35), (129, 9)]                  # on F32_BIG_FRAMES; column pass at 67 584 and 163 840 bytes

# 3f: TV
TV_STRIDED = (595, 597)
TV_SMALL = [(3, 3), (3, 597)]
TV_DEGENERATE = [(1, 1), (2, 9), (9, 2)]
TV_GRID_CAP, TV_BLOCK = 4096, 256


def f64_kernels(KH, KW):
    """[(route, integer kernel)] of one kernel shape on the float64 path"""
    ks = [("2d", int_kernel(KH, KW, F64_BITS[1], seed=11))]
    if min(KH, KW) > 1:
        ks.append(("rank1", int_outer_kernel(KH, KW, seed=12, bits=F64_BITS[1])))
    return ks


def f64_pairs():
    """every (frame, route, kernel) of 3a and 3b that is accepted"""
    for H, W in F64_FRAMES:
        for KH, KW in F64_KERNELS:
            for route, k in f64_kernels(KH, KW):
                yield (H, W), route, k
    for H, W in F64_LDS_FRAMES:
        for KH, KW, route, _, ok in F64_LDS_CASES:
            if ok:
                yield (H, W), route, (int_kernel(KH, KW, F64_BITS[1], seed=13) if route == "2d" else int_outer_kernel(KH, KW, seed=14, bits=F64_BITS[1]))


def f32_pairs():
    """every (frame, route, kernel) of 3e that is accepted"""
    kb = F32_BITS[1]
    for H, W in F32_FRAMES:
        for KH, KW in F32_KERNELS_2D:
            yield (H, W), "2d", int_kernel(KH, KW, kb, seed=21)
        for KH, KW in F32_KERNELS_RANK1:
            yield (H, W), "rank1", int_outer_kernel(KH, KW, seed=22, bits=kb)
    for H, W in F32_BIG_FRAMES:
        for KH, KW, _ in F32_KERNELS_2D_BIG:
            yield (H, W), "2d", int_kernel(KH, KW, kb, seed=23)
        for KH, KW in F32_KERNELS_RANK1_BIG:
            yield (H, W), "rank1", int_outer_kernel(KH, KW, seed=24, bits=kb)
    for H, W in F32_COLS_FRAMES:
        for K, _ in F32_COLS_ONLY:
            yield (H, W), "cols", int_kernel(K, 1, kb, seed=25)


def f64_box_cases():
    """(radius, frame) of the float64 box means of 3c: the radii on the frames of 3a that hold them, then the ones that do not"""
    return [(r, f) for r in F64_BOX_RADII for f in F64_FRAMES if r == 0 or min(f) > r] + list(F64_BOX_WRAP)


def f64_picture(H, W):
    return int_picture(H, W, F64_BITS[0], seed=31)


def f32_picture(H, W):
    return int_picture(H, W, F32_BITS[0], seed=32, channels=3)


def nan_case(H, W, channels=None):
    """(picture as float64 with one NaN and one +inf, 9 x 7 integer kernel with zeros): the NaN rectangle of the result shows which
    pixels every output read"""
    bits = F64_BITS if channels is None else F32_BITS
    pic = int_picture(H, W, bits[0], seed=41, channels=channels).astype(np.float64)
    k = int_kernel(*NAN_KERNEL, bits[1], seed=42)
    k[0, :] = 0; k[:, -1] = 0; k[4, 3] = 0                             # zero first row, zero last column, a zero inside
    k[1:3, :2] = [[2 ** bits[1] - 1, 1], [1, 2]]
    assert np.linalg.matrix_rank(k.astype(np.float64)) > 1
    nan_at, inf_at = (H // 3, W // 4), ((2 * H) // 3, W - 2)           # the inf next to the right edge: its reflection is read too
    if channels is not None:                                           # one channel each: the others must stay finite
        nan_at, inf_at = nan_at + (1,), inf_at + (channels - 1,)
    pic[nan_at] = np.nan
    pic[inf_at] = np.inf
    return pic, k
