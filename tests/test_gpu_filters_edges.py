"""GPU: the stand-alone filters at tile, halo and LDS edges, bit for bit.

The float64 per-channel filters behind lib.utils on arrays (csrc/ics_filters.hip, hosts in csrc/ics_ops.hip), the float32 filters on
resident frames (csrc/ics_img_filters.hip, hosts in csrc/ics_images.hip) and the TV stencil k_tv.  Pictures and taps are small
integers (tests/filters_ref.py), a window is the integer kernel scaled by a power of two, a USM amount a multiple of 1/4: every
product and every partial sum is then a number of the device's format, so any correct kernel gives the bits of the int64 reference,
whatever its summation order or use of FMA, and every convolution, USM and box-mean case is compared with `np.array_equal`.  The
references are checked against scipy and the float64 bilateral oracle in tests/test_filters_edges.py (CPU).  The bilateral filter
runs with std_i = std_s = 1e18, where both of its weights are exactly 1 and it is the window's integer sum divided once by
(2 r + 1)^2.  The only tolerances are imported from tests/test_utils.py: BILATERAL_RTOL (bilateral with real weights) and
TV_NORM2_RTOL (norm 2 of the TV stencil, as in test_gpu_tv_stencil_matches_oracle).

Dynamic LDS of the large cases, bytes per workgroup (64 KB = 65 536 is the default limit of a launch, above it the launcher raises
the kernel's limit first; 160 KB = 163 840 is what the host accepts):
    float64 2-D convolution   59 x 59  64 800 (last below the opt-in)   61 x 61  67 712 (first above)   112 x 112  163 592 (largest)
                              113 x 113 refused;  rank 1 111 x 111: two 1-D passes of 36 352 bytes
    float64 bilateral         radius 29  64 800   radius 30  67 712   radius 55  161 312 (largest)   radius 56 refused
    float32 bilateral         radius 14  61 776   radius 15  66 056 (first above)   radius 34  159 600 (largest)   radius 35 refused
    float32 2-D convolution   32 x 32  66 928 (smallest square above the opt-in)   71 x 71  163 744 (largest square)   73 x 73 refused
    float32 columns only      33 x 1  65 536 (no opt-in)   35 x 1  67 584 (first above)   129 x 1  163 840 (largest)
    float32 rank 1            35 x 35: column pass 67 584   129 x 9: column pass 163 840

Measured on an MI355X, float64 bilateral with real weights (std_i 0.2, std_s r / 2, 40 x 40) against the oracle, worst relative
error / BILATERAL_RTOL: radius 29 7.4e-5 (7.370e-16), radius 30 7.4e-5 (7.379e-16), radius 55 8.4e-5 (8.436e-16).
"""
import numpy as np
import pytest

import filters_ref as fr
import utils_oracle as uo
from test_utils import BILATERAL_RTOL, TV_NORM2_RTOL

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def same(out, ref, what):
    """np.array_equal, with the place and the size of the first difference in the message"""
    ref = np.asarray(ref)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if not np.array_equal(out, ref):
        bad = np.argwhere(out != ref)
        at = tuple(int(v) for v in bad[0])
        pytest.fail("%s: %d of %d values differ, first at %s: device %r, exact %r" % (what, len(bad), ref.size, at, out[at], ref[at]))


def window(k, dtype=F64):
    """(the integer kernel scaled by a power of two to a sum of about 1, the shift)"""
    sh = fr.shift_of(k)
    w = (k.astype(F64) / 2.0 ** sh).astype(dtype)
    assert np.array_equal(w.astype(F64) * 2.0 ** sh, k)
    return w, sh


def refused(call, text="LDS"):
    from lib import _native
    with pytest.raises(_native.NativeError) as ei:
        call()
    assert ei.value.code == _native.ICS_ENOSUP and text in str(ei.value), str(ei.value)


# ---- a. float64 convolution and USM ------------------------------------------------------------------------------------------------
def check_f64(ctx, pic, route, k, amounts, what):
    w, sh = window(k)
    src = pic.astype(F64)
    exact = fr.conv_symm_exact(pic, k)
    same(ctx.conv2d_symm(src, w), exact.astype(F64) / 2.0 ** sh, "%s conv %s" % (what, route))
    for amount in amounts:
        same(ctx.usm(src, w, amount), fr.usm_exact(pic, k, sh, amount, F64, conv=exact), "%s usm %g %s" % (what, amount, route))


@pytest.mark.parametrize("H,W", fr.F64_FRAMES)
def test_f64_convolution_and_usm_are_exact(ctx, H, W):
    pic = fr.f64_picture(H, W)
    for KH, KW in fr.F64_KERNELS:
        for route, k in fr.f64_kernels(KH, KW):
            check_f64(ctx, pic, route, k, fr.USM_AMOUNTS, "%d x %d, kernel %d x %d" % (H, W, KH, KW))


def test_f64_lib_utils_wrappers_with_a_dyadic_window():
    """lib.utils.gaussian_blur / USM on an array: at std 1e30 the Gaussian window of 4 taps is exactly 1, the kernel 1/16 everywhere"""
    from lib import utils
    assert np.array_equal(utils.gaussian_kernel(4, 1e30), np.full((4, 4), 1.0 / 16))
    pic = fr.f64_picture(33, 64)
    ones = np.ones((4, 4), np.int64)
    same(utils.gaussian_blur(pic.astype(F64), 4, 1e30), fr.conv_symm_exact(pic, ones) / 16.0, "utils.gaussian_blur")
    same(utils.USM(pic.astype(F64), 4, 1e30, 0.5, method="gauss"), fr.usm_exact(pic, ones, 4, 0.5), "utils.USM")


def check_nan_locality(out, ref):
    """NaN exactly where scipy has it, +inf likewise, the bits of scipy wherever it is finite"""
    assert np.array_equal(np.isnan(out), np.isnan(ref)), "the NaN rectangle moved: %d device, %d scipy" % (np.isnan(out).sum(), np.isnan(ref).sum())
    assert np.array_equal(np.isposinf(out), np.isposinf(ref)) and not np.isneginf(out).any()
    fin = np.isfinite(ref)
    same(out[fin], ref[fin], "finite values")


def test_f64_nan_and_inf_stay_in_their_window(ctx):
    pic, k = fr.nan_case(*fr.NAN_FRAME_F64)
    w, _ = window(k)
    check_nan_locality(ctx.conv2d_symm(pic, w), uo.conv2d_symm(pic, w))


# ---- b. float64 above 64 KB of LDS and at the limit --------------------------------------------------------------------------------
def test_f64_above_64k_lds_and_at_the_limit(ctx):
    for H, W in fr.F64_LDS_FRAMES:
        pic = fr.f64_picture(H, W)
        src = pic.astype(F64)
        for KH, KW, route, _, ok in fr.F64_LDS_CASES:
            k = fr.int_kernel(KH, KW, fr.F64_BITS[1], seed=13) if route == "2d" else fr.int_outer_kernel(KH, KW, seed=14, bits=fr.F64_BITS[1])
            if ok:
                check_f64(ctx, pic, route, k, [1.5], "%d x %d, kernel %d x %d" % (H, W, KH, KW))
            else:
                w, _ = window(k)
                refused(lambda: ctx.conv2d_symm(src, w), "LDS tile (up to 112 x 112")      # the text states what the formula allows
                refused(lambda: ctx.usm(src, w, 0.5))
        for r, _, ok in fr.F64_LDS_BILATERAL:
            if ok:
                same(ctx.bilateral(src, r, 1e18, 1e18), fr.box_mean(pic, r, F64), "%d x %d, box mean radius %d" % (H, W, r))
            else:
                refused(lambda: ctx.bilateral(src, r, 1e18, 1e18), "LDS tile (up to 55)")


# ---- c. bilateral indexing: the box mean -------------------------------------------------------------------------------------------
def test_f64_bilateral_with_unit_weights_is_the_box_mean(ctx):
    for r, (H, W) in fr.f64_box_cases():
        pic = fr.f64_picture(H, W)
        same(ctx.bilateral(pic.astype(F64), r, 1e18, 1e18), fr.box_mean(pic, r, F64), "%d x %d, box mean radius %d" % (H, W, r))


def check_f32_box(ctx, radii):
    from lib._native import DeviceImage
    for H, W in fr.F32_BOX_FRAMES:
        pic = fr.f32_picture(H, W)
        img = DeviceImage.from_host(pic.astype(F32), ctx)
        for r in radii:
            same(img.bilateral(r, 1e18, 1e18).to_host(), fr.box_mean(pic, r, F32), "%d x %d x 3, box mean radius %d" % (H, W, r))
    return img


def test_f32_bilateral_with_unit_weights_is_the_box_mean(ctx):
    check_f32_box(ctx, [r for r, _ in fr.F32_BOX_RADII if fr.lds_f32_bilateral(r) <= fr.LDS_OPT_IN])


def test_f32_bilateral_above_64k_lds_and_at_the_limit(ctx):
    img = check_f32_box(ctx, [r for r, _ in fr.F32_BOX_RADII if fr.lds_f32_bilateral(r) > fr.LDS_OPT_IN])
    refused(lambda: img.bilateral(fr.F32_BOX_REFUSED, 1e18, 1e18), "LDS tile (up to 34)")


# ---- d. float64 bilateral with real weights at the new radii -----------------------------------------------------------------------
@pytest.mark.parametrize("radius", fr.F64_BILATERAL_REAL)
def test_f64_bilateral_with_real_weights_above_the_tested_radii(ctx, radius):
    src = np.random.default_rng(radius).random((40, 40))
    out = ctx.bilateral(src, radius, 0.2, radius / 2.0)
    ref = uo.bilateral_filter(src, radius, 0.2, radius / 2.0)
    err = float(np.max(np.abs(out - ref) / np.abs(ref)))
    print("bilateral radius %d, 40 x 40: worst relative error %.3e, error / gate %.1e" % (radius, err, err / BILATERAL_RTOL))
    np.testing.assert_allclose(out, ref, rtol=BILATERAL_RTOL)


# ---- e. float32 resident-frame convolution and USM ---------------------------------------------------------------------------------
def f32_usm(img, w, amount):
    """ics_img_usm with a kernel of the caller's (DeviceImage.usm builds a Kaiser or Gaussian window of its own)"""
    from lib import _native
    w = np.ascontiguousarray(w, dtype=F32)
    return img._new(_native.load().ics_img_usm, _native._ptr(w), w.shape[0], w.shape[1], float(amount))


def check_f32(img, pic, route, k, amounts, what):
    w, sh = window(k, F32)
    exact = fr.conv_symm_exact(pic, k)
    same(img.convolve(w).to_host(), (exact.astype(F64) / 2.0 ** sh).astype(F32), "%s conv %s" % (what, route))
    for amount in amounts:
        same(f32_usm(img, w, amount).to_host(), fr.usm_exact(pic, k, sh, amount, F32, conv=exact).astype(F32), "%s usm %g %s" % (what, amount, route))


@pytest.mark.parametrize("H,W", fr.F32_FRAMES)
def test_f32_convolution_and_usm_are_exact(ctx, H, W):
    from lib._native import DeviceImage
    pic = fr.f32_picture(H, W)
    img = DeviceImage.from_host(pic.astype(F32), ctx)
    kb = fr.F32_BITS[1]
    for KH, KW in fr.F32_KERNELS_2D:
        check_f32(img, pic, "2d", fr.int_kernel(KH, KW, kb, seed=21), fr.USM_AMOUNTS, "%d x %d x 3, kernel %d x %d" % (H, W, KH, KW))
    for KH, KW in fr.F32_KERNELS_RANK1:
        check_f32(img, pic, "rank1", fr.int_outer_kernel(KH, KW, seed=22, bits=kb), fr.USM_AMOUNTS, "%d x %d x 3, kernel %d x %d" % (H, W, KH, KW))
    same(img.to_host(), pic.astype(F32), "the source after the filters")


def test_f32_convolution_above_64k_lds_and_at_the_limit(ctx):
    from lib._native import DeviceImage
    kb = fr.F32_BITS[1]
    for H, W in fr.F32_BIG_FRAMES:
        pic = fr.f32_picture(H, W)
        img = DeviceImage.from_host(pic.astype(F32), ctx)
        for KH, KW, _ in fr.F32_KERNELS_2D_BIG:
            check_f32(img, pic, "2d", fr.int_kernel(KH, KW, kb, seed=23), [1.5], "%d x %d x 3, kernel %d x %d" % (H, W, KH, KW))
        for KH, KW in fr.F32_KERNELS_RANK1_BIG:
            check_f32(img, pic, "rank1", fr.int_outer_kernel(KH, KW, seed=24, bits=kb), [-0.25], "%d x %d x 3, kernel %d x %d" % (H, W, KH, KW))
        w, _ = window(fr.int_kernel(*fr.F32_KERNEL_REFUSED, kb, seed=23), F32)
        refused(lambda: img.convolve(w))
        refused(lambda: f32_usm(img, w, 0.5))
    for H, W in fr.F32_COLS_FRAMES:
        pic = fr.f32_picture(H, W)
        img = DeviceImage.from_host(pic.astype(F32), ctx)
        for K, _ in fr.F32_COLS_ONLY:
            check_f32(img, pic, "cols", fr.int_kernel(K, 1, kb, seed=25), [0.5], "%d x %d x 3, kernel %d x 1" % (H, W, K))


def test_f32_nan_and_inf_stay_in_their_window_and_channel(ctx):
    from lib._native import DeviceImage
    pic, k = fr.nan_case(*fr.NAN_FRAME_F32, channels=3)
    w, _ = window(k, F32)
    out = DeviceImage.from_host(pic.astype(F32), ctx).convolve(w).to_host()
    ref = np.dstack([uo.conv2d_symm(pic[..., c], w.astype(F64)) for c in range(3)])
    check_nan_locality(out.astype(F64), ref)


@pytest.mark.parametrize("H,W", [(1, 1), (15, 85), (33, 5)])
def test_f32_rows_that_end_inside_a_quad_on_poisoned_red_zoned_blocks(ctx, debug_switch, H, W):
    """3 W = 3 (mod 4): the last 16-byte access of a row holds one float of the next row, and behind the last row one float that
    belongs to nobody.  A load of it reads the poison of the pool's check mode (tests/test_gpu_pool_check.py), a store of it lands in
    the red zone: either is seen whatever the order of the workgroups."""
    import test_gpu_pool_check as pc
    from lib._native import DeviceImage
    ok, seen = pc.selftest()
    assert ok, seen
    assert (3 * W) % 4 == 3
    kb = fr.F32_BITS[1]
    pic = fr.f32_picture(H, W)
    kernels = {"2d": fr.int_kernel(3, 3, kb, seed=21), "rank1": fr.int_outer_kernel(4, 6, seed=22, bits=kb), "cols": fr.int_kernel(33, 1, kb, seed=25)}

    def run():
        img = DeviceImage.from_host(pic.astype(F32), ctx)
        out = {"box": pc._host(img.bilateral(1, 1e18, 1e18))}
        for route, k in kernels.items():
            w, _ = window(k, F32)
            out[route] = pc._host(img.convolve(w))
            out[route + " usm"] = pc._host(f32_usm(img, w, 0.5))
        img.close()
        return out

    got, _, _ = pc.on_poison(debug_switch, run)       # poisoned and unpoisoned runs agree bit for bit, no store behind a block
    out = got[pc.FILLS[0]]
    same(out["box"], fr.box_mean(pic, 1, F32), "box mean")
    for route, k in kernels.items():
        sh = fr.shift_of(k)
        exact = fr.conv_symm_exact(pic, k)
        same(out[route], (exact.astype(F64) / 2.0 ** sh).astype(F32), "conv " + route)
        same(out[route + " usm"], fr.usm_exact(pic, k, sh, 0.5, F32, conv=exact).astype(F32), "usm " + route)


# ---- seeded top-up -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["f64_conv", "f64_usm", "f32_conv", "f32_usm"])
def test_random_frames_and_kernels_are_exact(ctx, entry):
    """Seeded hypothesis top-up: 8 cases per entry point, frame sides 1 .. 70, kernel sides 1 .. 40, 2-D or rank 1, all within the
    exactness budget (40 x 40 taps are 11 bits) and the LDS limit"""
    from hypothesis import HealthCheck, given, settings, strategies as st
    from lib._native import DeviceImage
    bits = fr.F64_BITS if entry.startswith("f64") else fr.F32_BITS

    @settings(max_examples=8, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(st.integers(1, 70), st.integers(1, 70), st.integers(1, 40), st.integers(1, 40), st.booleans(), st.sampled_from(fr.USM_AMOUNTS), st.integers(0, 10 ** 6))
    def check(H, W, KH, KW, outer, amount, seed):
        fr.assert_budget(bits, KH, KW)
        route = "rank1" if outer and min(KH, KW) > 1 else "2d"
        k = fr.int_outer_kernel(KH, KW, seed, bits=bits[1]) if route == "rank1" else fr.int_kernel(KH, KW, bits[1], seed)
        what = "%d x %d, kernel %d x %d, seed %d" % (H, W, KH, KW, seed)
        amounts = [amount] if entry.endswith("usm") else []
        if entry.startswith("f64"):
            check_f64(ctx, fr.int_picture(H, W, bits[0], seed), route, k, amounts, what)
        else:
            pic = fr.int_picture(H, W, bits[0], seed, channels=3)
            check_f32(DeviceImage.from_host(pic.astype(F32), ctx), pic, route, k, amounts, what)

    check()


# ---- f. TV stencil -----------------------------------------------------------------------------------------------------------------
def check_tv(ctx, M, N, order, norm):
    import rl_mm_oracle as orc
    u = np.random.default_rng([M, N, order, norm]).random((M, N, 3), dtype=F32)
    for eps in (1e-2, 1e-6):
        out, div = ctx.tv(u, eps, order, norm)
        ro, rd = orc.TV(u, M, N, eps, order, norm)       # pinned bit for bit to the compiled reference (tests/golden/tv.npz)
        same(div, rd, "TV div %d x %d order %d norm %d eps %g" % (M, N, order, norm, eps))
        if norm == 1:
            same(out, ro, "TV out %d x %d order %d norm %d eps %g" % (M, N, order, norm, eps))
        else:
            np.testing.assert_allclose(out, ro, rtol=TV_NORM2_RTOL, atol=0)
        assert np.all(out[0] == 0) and np.all(out[-1] == 0) and np.all(div[:, 0] == 0) and np.all(div[:, -1] == 0)
        assert np.all(out[1:-1, 1:-1] > 0)               # every interior value was written: a norm plus epsilon is positive


@pytest.mark.parametrize("order,norm", [(2, 1), (2, 2), (1, 1), (1, 2)])
def test_tv_stencil_where_the_capped_grid_strides(ctx, order, norm):
    check_tv(ctx, *fr.TV_STRIDED, order, norm)


def test_tv_stencil_on_one_interior_pixel_and_one_interior_row(ctx):
    for M, N in fr.TV_SMALL:
        for order, norm in ((2, 1), (2, 2), (1, 1), (1, 2)):
            check_tv(ctx, M, N, order, norm)


def test_tv_stencil_without_an_interior_is_zero(ctx):
    for M, N in fr.TV_DEGENERATE:
        u = np.random.default_rng(M * 10 + N).random((M, N, 3), dtype=F32)
        for order, norm in ((2, 1), (1, 2)):
            out, div = ctx.tv(u, 1e-3, order, norm)
            assert out.shape == u.shape and not out.any() and not div.any()
