"""CPU: the exact references of tests/filters_ref.py are right, and the case lists of tests/test_gpu_filters_edges.py are what they
claim to be -- every case within the exactness budget, every quoted LDS size recomputed from the formulas of the .hip files and on
the stated side of the 64 KB opt-in and the 160 KB limit."""
import numpy as np
import pytest

import filters_ref as fr
import utils_oracle as uo


def scipy_conv(src, k):
    src = np.asarray(src, np.float64)
    if src.ndim == 3:
        return np.dstack([uo.conv2d_symm(src[..., c], k.astype(np.float64)) for c in range(src.shape[2])])
    return uo.conv2d_symm(src, k.astype(np.float64))


def conv_float_loop(src, k):
    """conv_symm_exact's loop in float64 with no tap skipped: 0 * NaN and 0 * inf are NaN, as in any plain multiply-add"""
    KH, KW = k.shape
    H, W = src.shape[:2]
    cy, cx = (KH - 1) // 2, (KW - 1) // 2
    ext = np.pad(src, ((KH - 1 - cy, cy), (KW - 1 - cx, cx)) + ((0, 0),) * (src.ndim - 2), mode="symmetric")
    out = np.zeros_like(src)
    with np.errstate(invalid="ignore"):
        for p in range(KH):
            for q in range(KW):
                out += float(k[p, q]) * ext[KH - 1 - p: KH - 1 - p + H, KW - 1 - q: KW - 1 - q + W]
    return out


@pytest.mark.parametrize("which", ["float64", "float32"])
def test_conv_symm_exact_equals_scipy_on_every_pair_of_the_gpu_file(which):
    pairs, picture = (fr.f64_pairs, fr.f64_picture) if which == "float64" else (fr.f32_pairs, fr.f32_picture)
    n = 0
    for (H, W), route, k in pairs():
        pic = picture(H, W)
        exact = fr.conv_symm_exact(pic, k)
        assert exact.dtype == np.int64 and exact.shape == pic.shape
        assert np.array_equal(scipy_conv(pic, k), exact.astype(np.float64)), ((H, W), route, k.shape)
        n += 1
    assert n >= 80


@pytest.mark.parametrize("frame,kernel", [((5, 7), (13, 15)), ((2, 3), (31, 2)), ((4, 4), (111, 111)), ((1, 1), (9, 7)), ((1, 1), (1, 1))])
def test_kernels_larger_than_the_frame_reflect_more_than_once(frame, kernel):
    pic = fr.f64_picture(*frame)
    k = fr.int_kernel(*kernel, fr.F64_BITS[1], seed=5)
    fr.assert_budget(fr.F64_BITS, *kernel)
    assert np.array_equal(scipy_conv(pic, k), fr.conv_symm_exact(pic, k).astype(np.float64))


def test_box_mean_is_the_bilateral_oracle_with_unit_weights():
    for r, (H, W) in fr.f64_box_cases() + [(r, f) for r, _, ok in fr.F64_LDS_BILATERAL if ok for f in fr.F64_LDS_FRAMES]:
        pic = fr.f64_picture(H, W)
        assert np.array_equal(fr.box_mean(pic, r, np.float64), uo.bilateral_filter(pic.astype(np.float64), r, 1e18, 1e18)), (r, H, W)
    # float32: the same integer sum, the one division rounded to float32 (correct rounding of the exact quotient)
    pic = fr.f32_picture(16, 86)
    for r in (0, 5, 34):
        D2 = (2 * r + 1) ** 2
        s = fr.conv_symm_exact(pic, np.ones((2 * r + 1, 2 * r + 1), np.int64))
        b = fr.box_mean(pic, r, np.float32)
        q = s.astype(np.float64) / D2
        assert b.dtype == np.float32 and s.max() < 2 ** 24 and np.all(np.abs(b - q) <= 2.0 ** -24 * q)   # within half an ulp of the quotient
    # the unit weights: both exponentials are exactly 1 in float32 and float64
    ki32 = np.float32(-1.0 / (2.0 * 1e18 * 1e18))
    assert np.isfinite(ki32) and abs(ki32) >= np.finfo(np.float32).tiny                         # a normal number
    assert np.exp(np.float32(15 * 15) * ki32, dtype=np.float32) == 1 and np.float32(np.exp(-(34 * 34 * 2) / 2e36)) == 1
    assert np.exp(-(255.0 ** 2) / 2e36) == 1.0 and np.exp(-(55 * 55 * 2) / 2e36) == 1.0


def test_every_case_is_within_the_exactness_budget():
    for bits, pairs in ((fr.F64_BITS, fr.f64_pairs), (fr.F32_BITS, fr.f32_pairs)):
        for (H, W), route, k in pairs():
            fr.assert_budget(bits, *k.shape)
            assert k.min() >= 0 and k.max() < 2 ** bits[1]
            rank = np.linalg.matrix_rank(k.astype(np.float64))
            if route == "rank1":
                top = int(k.max())
                assert rank == 1 and min(k.shape) > 1 and top & (top - 1) == 0
            elif min(k.shape) > 1:
                assert rank > 1
            else:
                assert route in ("2d", "cols")
    assert fr.budget_bits(4, 3, 71, 71) == 20          # 5041 taps are 13 bits
    with pytest.raises(AssertionError):
        fr.assert_budget(fr.F32_BITS, 300, 300)
    for bits, picture in ((fr.F64_BITS, fr.f64_picture), (fr.F32_BITS, fr.f32_picture)):
        pic = picture(33, 5)
        assert pic.min() >= 0 and pic.max() < 2 ** bits[0] and pic.max() >= 2 ** (bits[0] - 1)
    # box means: the window sum of (2 r + 1)^2 pixels
    assert 8 + np.log2(111 ** 2) <= 52 and 4 + np.log2(69 ** 2) <= 23


def test_usm_reference_is_exact_in_the_precision_of_the_device():
    """usm_exact asserts that the blur, the difference and the result are numbers of the device's format for every case of the GPU file"""
    for dtype, pairs, picture in ((np.float64, fr.f64_pairs, fr.f64_picture), (np.float32, fr.f32_pairs, fr.f32_picture)):
        for (H, W), route, k in pairs():
            pic = picture(H, W)
            for amount in fr.USM_AMOUNTS:
                out = fr.usm_exact(pic, k, fr.shift_of(k), amount, dtype)
                assert out.shape == pic.shape
    pic, k = fr.f64_picture(3, 5), fr.int_kernel(3, 3, 8, seed=1)
    blur = fr.conv_symm_exact(pic, k) / 2.0 ** fr.shift_of(k)
    assert np.array_equal(fr.usm_exact(pic, k, fr.shift_of(k), 1.5), pic + (pic - blur) * 1.5)
    with pytest.raises(AssertionError):
        fr.usm_exact(pic, k, fr.shift_of(k), 0.3)


def test_nan_case_scipy_spreads_nan_like_a_plain_loop():
    for (H, W), ch in ((fr.NAN_FRAME_F64, None), (fr.NAN_FRAME_F32, 3)):
        pic, k = fr.nan_case(H, W, ch)
        assert np.isnan(pic).sum() == 1 and np.isinf(pic).sum() == 1 and (k == 0).sum() >= 16
        ref, loop = scipy_conv(pic, k), conv_float_loop(pic, k)
        assert np.array_equal(np.isnan(ref), np.isnan(loop)) and np.array_equal(np.isposinf(ref), np.isposinf(loop))
        fin = np.isfinite(ref)
        assert np.array_equal(ref[fin], loop[fin])
        n = int(np.isnan(ref).sum())
        assert 9 * 7 <= n < 3 * 9 * 7 and fin.sum() > ref.size // 2      # the NaN's whole window, and the zero taps over the inf
        if ch:
            assert np.isfinite(ref[..., 0]).all()                         # channels do not mix


def test_quoted_lds_sizes_and_the_limits():
    lo, hi = fr.LDS_OPT_IN, fr.LDS_LIMIT
    assert (lo, hi) == (65536, 163840)
    # float64 convolution
    for KH, KW, route, quoted, ok in fr.F64_LDS_CASES:
        if route == "2d":
            assert (fr.lds_f64_conv(KH, KW) <= hi) == ok
            if ok:
                assert fr.lds_f64_conv(KH, KW) == quoted
        else:   # two 1-D passes; the host still gates on the 2-D size
            assert fr.lds_f64_conv(KH, KW) <= hi and max(fr.lds_f64_conv(1, KW), fr.lds_f64_conv(KH, 1)) <= lo
    assert fr.lds_f64_conv(59, 59) <= lo < fr.lds_f64_conv(60, 60) <= fr.lds_f64_conv(61, 61)
    assert fr.lds_f64_conv(112, 112) <= hi < fr.lds_f64_conv(113, 113) and fr.lds_f64_conv(112, 113) > hi
    assert max(fr.lds_f64_conv(*k) for k in fr.F64_KERNELS) <= lo
    # float64 bilateral
    for r, quoted, ok in fr.F64_LDS_BILATERAL:
        assert (fr.lds_f64_bilateral(r) <= hi) == ok
        if ok:
            assert fr.lds_f64_bilateral(r) == quoted
    assert fr.lds_f64_bilateral(29) <= lo < fr.lds_f64_bilateral(30) and fr.lds_f64_bilateral(55) <= hi < fr.lds_f64_bilateral(56)
    # float32 bilateral
    for r, quoted in fr.F32_BOX_RADII:
        assert fr.lds_f32_bilateral(r) <= hi and (quoted is None or fr.lds_f32_bilateral(r) == quoted)
    assert fr.lds_f32_bilateral(14) <= lo < fr.lds_f32_bilateral(15) and fr.lds_f32_bilateral(34) <= hi < fr.lds_f32_bilateral(fr.F32_BOX_REFUSED)
    assert fr.F32_BOX_REFUSED == 35
    # float32 2-D
    K = fr.F32_ABOVE_OPT_IN
    assert fr.lds_f32_rows(K - 1, K - 1) <= lo < fr.lds_f32_rows(K, K) and K == 32
    for KH, KW, quoted in fr.F32_KERNELS_2D_BIG:
        assert lo < fr.lds_f32_rows(KH, KW) == quoted <= hi
    assert fr.lds_f32_rows(71, 71) <= hi < fr.lds_f32_rows(72, 72) <= fr.lds_f32_rows(*fr.F32_KERNEL_REFUSED)
    assert max(fr.lds_f32_rows(*k) for k in fr.F32_KERNELS_2D) <= lo
    # float32 columns only and rank 1
    for KH, quoted in fr.F32_COLS_ONLY:
        assert fr.lds_f32_cols(KH) == quoted <= hi
    assert fr.lds_f32_cols(33) <= lo < fr.lds_f32_cols(35) and fr.lds_f32_cols(129) <= hi < fr.lds_f32_cols(130)
    for KH, KW in fr.F32_KERNELS_RANK1_BIG:
        assert lo < fr.lds_f32_cols(KH) <= hi and fr.lds_f32_rows(1, KW) <= lo
    assert fr.lds_f32_rows(1, 764) <= hi < fr.lds_f32_rows(1, 765)      # "rank 1: up to 129 x 764" of the refusal text
    # TV: the strided frame has more elements than the capped grid has lanes, by less than 1 %; the small ones fit one pass
    M, N = fr.TV_STRIDED
    cap = fr.TV_GRID_CAP * fr.TV_BLOCK
    assert 1.01 * cap > (M - 2) * (N - 2) * 3 == 1058505 > cap
    assert all((m - 2) * (n - 2) * 3 <= cap for m, n in fr.TV_SMALL) and all(min(m, n) < 3 for m, n in fr.TV_DEGENERATE)


def test_frames_sit_on_the_tile_edges():
    """float64: 32 x 32 tiles; float32: 256 flat floats (3 W) by 16 rows (row / 2-D pass, bilateral) or 32 rows (column pass)"""
    sides = {s for f in fr.F64_FRAMES for s in f}
    assert {1, 31, 32, 33, 64, 65} <= sides
    widths = sorted({W for _, W in fr.F32_FRAMES})
    assert {(3 * W) % 4 for W in (85, 86, 171, 172)} == {0, 1, 2, 3} and {85, 86, 171, 172} <= set(widths)
    assert 3 * 85 < 256 < 3 * 86 and 3 * 171 == 513 and 3 * 172 > 512 and (256 % 3, 512 % 3) == (1, 2)   # the tile edge falls inside a pixel
    assert {15, 16, 17, 31, 32, 33} <= {H for H, _ in fr.F32_FRAMES}
