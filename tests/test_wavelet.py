"""CPU: the oracle of the wavelet equaliser (tests/wavelet_ref.py: undecimated B3-spline scales, soft-thresholded, weighted, summed)
checked against what the algorithm guarantees, and the surface of ics_img_wavelet_equalize / DeviceImage.wavelet_equalize /
lib.utils.wavelet_equalizer / deblur_module(local_contrast=...) as far as it can be checked without a GPU.

Rounding bounds.  Pictures lie in [0, 1]; every c_j is a convex combination of pixels and lies there too, |w_j| <= 1, and u is the
unit roundoff of the dtype (2^-24 / 2^-53).  With gains 1, thresholds 0 and residual 1 the shrinkage and the products are exact
(m / m = 1), so the output is c_J + ((w_0 + w_1) + ...) and differs from f = c_J + sum w_j only by the J subtractions w_j =
c_j - c_{j+1}, the J - 1 additions of the accumulator (the first, to zero, is exact) and the final addition, each rounding a value
of magnitude <= 1 (the final one <= 2): at most (2 J + 1) u."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wavelet_ref as wr
from test_gpu_img_filters import picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ics_hip.h")
TINY = [(1, 9), (9, 1), (5, 7)]
SHAPES = TINY + [(33, 100), (64, 96)]
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def wv_picture(H, W):
    return picture(H, W, seed=3000 + 3 * H + W)


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
def test_identity_setting_returns_the_picture(coupling, dtype):
    for H, W in SHAPES:
        pic = wv_picture(H, W)
        for J in (1, 5, 8):
            out = wr.wavelet_equalize(pic, [1.0] * J, None, 1.0, coupling, dtype=dtype)
            assert out.dtype == dtype and out.shape == pic.shape
            assert worst(out, pic) <= (2 * J + 1) * U[dtype] + 1e-18, (H, W, J, worst(out, pic))     # (1e-18: a w whose square underflows)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_hot_details_and_the_residual_sum_to_the_picture(dtype):
    """gains one-hot, residual 0: the detail w_j itself (0 + 1 * w_j, the other scales add 0 * s = 0); gains 0: c_J.  Summed in
    float64 they give f up to the J roundings of the subtractions."""
    J = 5
    for H, W in SHAPES:
        pic = wv_picture(H, W)
        details, cJ = wr.decompose(pic, J, dtype)
        total = np.zeros(pic.shape, np.float64)
        for j in range(J):
            w = wr.wavelet_equalize(pic, np.eye(J)[j], None, 0.0, "channel", dtype=dtype)
            assert np.array_equal(w, details[j])
            assert np.array_equal(wr.wavelet_equalize(pic, np.eye(J)[j], None, 0.0, "vector", dtype=dtype), details[j])
            total += w
        total += wr.wavelet_equalize(pic, [0.0] * J, None, 1.0, "vector", dtype=dtype)
        assert worst(total, pic) <= (J + 1) * U[dtype], (H, W, worst(total, pic))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
def test_a_constant_picture_is_a_fixed_point(coupling, dtype):
    """With at most 8 significant bits in the constant every product and sum of the axis pass is exact (5 v / 8 + 3 v / 8 = v), so c_j =
    v, w_j = 0 and the output is v exactly, whatever the gains.  Any other constant comes back within the roundings of the passes:
    three per pass, so |c_{j+1} - c_j| <= 6 u v (1 + 6 u)^j and |out - v| <= 8 u v (J + sum |g_j|)."""
    gains, thr = [2.5, -1.0, 0.0, 4.0, 1.0], [0.0, 0.01, 0.0, 0.0, 0.02]
    exact = np.full((11, 13, 3), 0.375, np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    assert np.array_equal(wr.wavelet_equalize(exact, gains, thr, 1.0, coupling, dtype=dtype), exact.astype(dtype))
    other = np.full((11, 13, 3), np.float32(0.37), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    out = wr.wavelet_equalize(other, gains, None, 1.0, coupling, dtype=dtype)
    assert worst(out, other) <= 8 * U[dtype] * 0.74 * (5 + sum(abs(g) for g in gains))


def test_zero_gains_give_the_residual_and_the_transform_keeps_the_mean():
    """The folded operator is a symmetric matrix with unit row sums (the symmetric extension of a symmetric filter), so its column
    sums are 1 too and every c_j has the mean of f on any frame.  The frame where no fold takes part at all: 96 x 80, zero outside
    rows 30 .. 65 and columns 30 .. 49, J = 3 (reach 2 (2^3 - 1) = 14 px): what the folded taps read near the border is zero and the
    bump never gets there."""
    pic = wv_picture(96, 80)
    J = 5
    cJ = wr.decompose(pic, J)[1]
    for coupling in wr.COUPLINGS:
        assert np.array_equal(wr.wavelet_equalize(pic, [0.0] * J, [0.1] * J, 0.5, coupling), 0.5 * cJ)
    assert np.max(np.abs(cJ.mean(axis=(0, 1)) - pic.astype(np.float64).mean(axis=(0, 1)))) <= 1e-14
    bump = np.zeros_like(pic)
    bump[30:66, 30:50] = pic[30:66, 30:50]
    c3 = wr.decompose(bump, 3)[1]
    assert not c3[:16].any() and not c3[-16:].any() and not c3[:, :16].any() and not c3[:, -16:].any()
    assert c3[20].any()                                                  # it did spread
    assert np.max(np.abs(c3.sum(axis=(0, 1)) - bump.astype(np.float64).sum(axis=(0, 1)))) <= 1e-11


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
def test_a_channel_permutation_permutes_the_output_exactly(coupling, dtype):
    pic = wv_picture(33, 40)
    gains, thr = [2.5, 2.0, 1.5, 1.2], [0.05, 0.02, 0.01, 0.0]
    out = wr.wavelet_equalize(pic, gains, thr, 0.9, coupling, dtype=dtype)
    for order in ([2, 0, 1], [1, 0, 2]):
        assert np.array_equal(wr.wavelet_equalize(np.ascontiguousarray(pic[..., order]), gains, thr, 0.9, coupling, dtype=dtype), out[..., order])


def test_channel_coupling_keeps_the_channels_apart_and_vector_coupling_does_not():
    pic = wv_picture(33, 40)
    other = pic.copy()
    other[..., 1] = wv_picture(40, 33)[:33, :33].mean()
    gains, thr = [1.0, 1.0, 1.0], [0.05, 0.02, 0.01]
    a, b = wr.wavelet_equalize(pic, gains, thr, 1.0, "channel"), wr.wavelet_equalize(other, gains, thr, 1.0, "channel")
    assert np.array_equal(a[..., 0], b[..., 0]) and np.array_equal(a[..., 2], b[..., 2]) and not np.array_equal(a[..., 1], b[..., 1])
    a, b = wr.wavelet_equalize(pic, gains, thr, 1.0, "vector"), wr.wavelet_equalize(other, gains, thr, 1.0, "vector")
    assert not np.array_equal(a[..., 0], b[..., 0]) and not np.array_equal(a[..., 2], b[..., 2])
    # without a threshold there is nothing to couple: both forms return w
    assert worst(wr.wavelet_equalize(pic, [2.0, 1.5], None, 1.0, "vector"), wr.wavelet_equalize(pic, [2.0, 1.5], None, 1.0, "channel")) <= 4 * U[np.float64] * 4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
def test_a_threshold_above_the_largest_detail_removes_the_scale_exactly(coupling, dtype):
    pic = wv_picture(33, 40)
    J = 4
    gains = [2.5, 2.0, 1.5, 1.2]
    details, _ = wr.decompose(pic, J, dtype)
    for j in range(J):
        thr = [0.0] * J
        thr[j] = 2.0 * float(np.max(np.abs(details[j])))                # > sqrt(3) max |w|: above the vector magnitude too
        without = [g if i != j else 0.0 for i, g in enumerate(gains)]
        assert np.array_equal(wr.wavelet_equalize(pic, gains, thr, 1.0, coupling, dtype=dtype), wr.wavelet_equalize(pic, without, None, 1.0, coupling, dtype=dtype))


def test_the_folding_is_numpy_pad_symmetric():
    for n in (1, 2, 5, 9):
        ref = np.pad(np.arange(n), 3 * 256, mode="symmetric")
        assert np.array_equal(wr.fold(np.arange(-3 * 256, n + 3 * 256), n), ref)
    for H, W in TINY:
        c = wv_picture(H, W).astype(np.float64)
        for j in range(8):
            d = 2 ** j
            p = np.pad(c, ((2 * d, 2 * d), (2 * d, 2 * d), (0, 0)), mode="symmetric")
            tap = lambda a, k, axis: np.take(a, np.arange(a.shape[axis] - 4 * d) + (2 + k) * d, axis=axis)     # noqa: E731
            h = ((tap(p, -2, 1) + tap(p, 2, 1)) * (1 / 16) + (tap(p, -1, 1) + tap(p, 1, 1)) * (4 / 16)) + tap(p, 0, 1) * (6 / 16)
            v = ((tap(h, -2, 0) + tap(h, 2, 0)) * (1 / 16) + (tap(h, -1, 0) + tap(h, 1, 0)) * (4 / 16)) + tap(h, 0, 0) * (6 / 16)
            assert v.shape == c.shape and np.array_equal(wr.smooth(c, j), v), (H, W, j)
            c = v


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_function_and_the_constants():
    from lib import _native
    raw = open(HEADER).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    assert ("int ics_img_wavelet_equalize(const ics_img *src, int scales, const float *gains, const float *thresholds , float residual, "
            "int coupling, int route, ics_img **out);") in text
    assert "#define ICS_ABI_VERSION 4 " in text
    kh = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")).read()
    for src in (raw, kh):
        assert int(re.search(r"#define ICS_IMG_WAVELET_MAX_SCALES (\d+)", src).group(1)) == _native.IMG_WAVELET_MAX_SCALES == wr.MAX_SCALES == 8
        assert int(re.search(r"#define ICS_IMG_WAVELET_FUSED (\d+)", src).group(1)) == _native.IMG_WAVELET_FUSED
    assert 1 <= _native.IMG_WAVELET_FUSED <= _native.IMG_WAVELET_MAX_SCALES


def test_native_binds_it_and_refuses_bad_arguments_before_any_device_work():
    from lib import _native
    lib = _native.load()
    vp, ci, cf, pvp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)
    assert lib.ics_img_wavelet_equalize.argtypes == [vp, ci, vp, vp, cf, ci, ci, pvp] and lib.ics_img_wavelet_equalize.restype is ci
    out = C.c_void_p()
    fake = C.c_void_p(8)    # never dereferenced: the arguments are checked first
    ok = np.ones(8, np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    assert lib.ics_img_wavelet_equalize(None, 5, ptr(ok), None, 1.0, 1, 0, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_wavelet_equalize(fake, 5, ptr(ok), None, 1.0, 1, 0, None) == _native.ICS_EINVAL
    nan, inf, neg = ok.copy(), ok.copy(), ok.copy()
    nan[2], inf[0], neg[1] = np.nan, np.inf, -0.01
    for scales, gains, thr, residual, coupling, route, word in (
            (0, ok, None, 1.0, 1, 0, b"scales"), (9, ok, None, 1.0, 1, 0, b"scales"), (-1, ok, None, 1.0, 1, 0, b"scales"),
            (5, None, None, 1.0, 1, 0, b"gains"), (5, nan, None, 1.0, 1, 0, b"gains[2]"), (5, inf, ok, 1.0, 1, 0, b"gains[0]"),
            (5, ok, nan, 1.0, 1, 0, b"thresholds[2]"), (5, ok, inf, 1.0, 0, 0, b"thresholds[0]"), (5, ok, neg, 1.0, 0, 0, b"thresholds[1]"),
            (5, ok, ok, float("nan"), 1, 0, b"residual"), (5, ok, ok, float("inf"), 1, 0, b"residual"),
            (5, ok, None, 1.0, 2, 0, b"coupling"), (5, ok, None, 1.0, -1, 0, b"coupling"), (5, ok, None, 1.0, 1, 3, b"route"), (5, ok, None, 1.0, 1, -1, b"route")):
        assert lib.ics_img_wavelet_equalize(fake, scales, ptr(gains), ptr(thr), residual, coupling, route, C.byref(out)) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error(), (word, lib.ics_last_error())
    assert out.value is None
    # (2, nan at index 2): only the first `scales` values are looked at -- refused here for the NULL image alone
    assert lib.ics_img_wavelet_equalize(None, 2, ptr(nan), None, 1.0, 1, 0, C.byref(out)) == _native.ICS_EINVAL and b"NULL" in lib.ics_last_error()


BAD_ARGUMENTS = [
    (dict(gains=[]), "gains"), (dict(gains=[1.0] * 9), "gains"), (dict(gains=[[1.0, 1.0]]), "gains"), (dict(gains=[1.0, float("nan")]), "gains"),
    (dict(gains=[1.0, float("inf")]), "gains"), (dict(gains=[1.0, 1e39]), "gains"),
    (dict(gains=[1.0, 1.0], thresholds=[0.1]), "thresholds"), (dict(gains=[1.0], thresholds=[0.1, 0.1]), "thresholds"),
    (dict(gains=[1.0, 1.0], thresholds=[0.1, -0.1]), "thresholds"), (dict(gains=[1.0, 1.0], thresholds=[0.1, float("nan")]), "thresholds"),
    (dict(gains=[1.0, 1.0], thresholds=[float("inf"), 0.0]), "thresholds"),
    (dict(gains=[1.0], residual=float("nan")), "residual"), (dict(gains=[1.0], residual=float("-inf")), "residual"),
    (dict(gains=[1.0], coupling="colour"), "coupling"), (dict(gains=[1.0], coupling=1), "coupling"),
    (dict(gains=[1.0], route=3), "route"), (dict(gains=[1.0], route=-1), "route")]


def test_device_image_and_utils_raise_value_errors_before_any_native_call(monkeypatch):
    from lib import _native, utils
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("a native call"))
    img = _native.DeviceImage(None, None)                                # no handle: nothing to destroy
    assert callable(_native.DeviceImage.wavelet_equalize)
    for kw, word in BAD_ARGUMENTS:
        with pytest.raises(ValueError, match=word):
            img.wavelet_equalize(**kw)
        if "route" not in kw:
            with pytest.raises(ValueError, match=word):
                utils.wavelet_equalizer(np.zeros((8, 9, 3), np.float32), **kw)
    for bad in (np.zeros((8, 9)), np.zeros((8, 9, 4)), np.zeros((3, 8, 9, 3)), np.zeros(7)):
        with pytest.raises(ValueError, match="H x W x 3"):
            utils.wavelet_equalizer(bad, [1.0, 1.0])
    g, t, r, c, route = _native.wavelet_args([1, 2.5], None)
    assert g.dtype == np.float32 and g.tolist() == [1.0, 2.5] and t is None and (r, c, route) == (1.0, "vector", 0)
    g, t, r, c, route = _native.wavelet_args((1, 2), (0, 0.5), 0.5, "channel", 2)
    assert t.dtype == np.float32 and t.tolist() == [0.0, 0.5] and (r, c, route) == (0.5, "channel", 2)


# ---- deblur_module(local_contrast=...) --------------------------------------------------------------------------------------------
def test_deblur_module_validates_local_contrast_before_it_touches_a_device(monkeypatch):
    import deconvolve as dv
    from lib import _native
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("a native call"))
    pic = np.full((64, 64, 3), 128, np.uint8)
    for bad in ((), 1.5, ([1.0, 1.0], None, "vector", 1), ([1.0, 1.0], None, "colour"), ([],), ([1.0] * 9,), ([1.0, float("nan")],),
                ([1.0, 1.0], [0.1]), ([1.0, 1.0], [0.1, -0.1]), ([1.0, 1.0], [0.1, float("inf")]), ("abc",)):
        for resident in (None, False, True):
            with pytest.raises(ValueError, match="local_contrast"):
                dv.deblur_module(pic, "x", ".", 5, save=False, display=False, device_resident=resident, local_contrast=bad)
    assert dv._local_contrast_args(None) is None
    assert dv._local_contrast_args(([1, 1.5, 2],)) == ((1.0, 1.5, 2.0), None, "vector")
    assert dv._local_contrast_args([[1, 1.5], [0.25, 0]]) == ((1.0, 1.5), (0.25, 0.0), "vector")
    assert dv._local_contrast_args(([1, 1.5], None, "channel")) == ((1.0, 1.5), None, "channel")


def _recording_solver(calls):
    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd, **kw):
        calls.append((image.copy(), u.copy(), psf.copy(), (top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd), kw))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]
    return solver


def test_deblur_module_host_driver_equalises_after_the_denoiser_and_before_the_mask(monkeypatch, capsys):
    """local_contrast=None never calls utils.wavelet_equalizer and changes nothing; with all three arguments the host driver hands the
    deblurred gamma-encoded frame to tv_denoise, its result to wavelet_equalizer (residual 1) and that to USM, then clips (stand-ins
    record the order and answer with the oracles: no GPU here)"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    import tv_denoise_ref as tvr
    import utils_oracle as uo
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)
    seen, frames = [], {}

    def tv(src, weight=0.1, iterations=50, coupling="vector"):
        seen.append(("tv", src.shape, src.dtype, weight, iterations, coupling))
        frames["tv"] = tvr.tv_denoise(src, weight, iterations, coupling, dtype=np.float32)
        return frames["tv"]

    def wavelet(src, gains, thresholds=None, residual=1.0, coupling="vector"):
        seen.append(("wavelet", src.shape, src.dtype, tuple(gains), None if thresholds is None else tuple(thresholds), residual, coupling))
        frames["wavelet_in"] = src.copy()
        frames["wavelet"] = wr.wavelet_equalize(src, gains, thresholds, residual, coupling, dtype=np.float32)
        return frames["wavelet"]

    def usm(src, radius, strength, amount, method="bessel"):
        seen.append(("usm", src.shape))
        frames.setdefault("usm_in", []).append(np.array(src))
        return uo.USM(np.asarray(src, np.float64), radius, strength, amount, method)
    monkeypatch.setattr(dv.utils, "tv_denoise", tv)
    monkeypatch.setattr(dv.utils, "wavelet_equalizer", wavelet)
    monkeypatch.setattr(dv.utils, "USM", usm)
    pic = (np.random.default_rng(0).random((90, 100, 3)) * 255).astype(np.uint8)
    kw = dict(mask=[46, 50], mask_size=41, display=False, pyramid=False, save=False, iterations=7)
    base, none, full = [], [], []
    out0, psf0 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(base), **kw)
    out1, psf1 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(none), local_contrast=None, **kw)
    assert seen == [] and out0.dtype == out1.dtype and np.array_equal(out0, out1) and np.array_equal(psf0, psf1)
    gains, thr = (1.0, 1.6, 1.8, 1.4, 1.0), (0.02, 0.0, 0.0, 0.0, 0.0)
    out2, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(full), denoise=(0.05, 10), sharpen=(9, 4., 0.5),
                               local_contrast=(gains, thr, "channel"), **kw)
    assert seen == [("tv", (93, 103, 3), np.float32, 0.05, 10, "vector"), ("wavelet", (93, 103, 3), np.float32, gains, thr, 1.0, "channel")] + [("usm", (93, 103))] * 3
    assert np.array_equal(frames["wavelet_in"], frames["tv"])            # the denoiser's result goes in ...
    assert all(np.array_equal(frames["usm_in"][c], frames["wavelet"][..., c]) for c in range(3))      # ... and the equalised frame on to the mask
    assert len(base) == len(full) == 2
    for x, y in zip(base, full):                                          # the solver sees nothing of it
        assert x[3] == y[3] and x[4] == y[4] and all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))
    assert out2.shape == out0.shape and out2.min() >= 0 and out2.max() <= 65535 and not np.array_equal(out0, out2)
    # alone: applied to the gamma-encoded frame (the identity setting gives the plain result back, up to its roundings), then the clip
    seen.clear()
    out3, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), local_contrast=([1.0] * 5,), **kw)
    assert seen == [("wavelet", (93, 103, 3), np.float32, (1.0,) * 5, None, 1.0, "vector")]
    assert frames["wavelet_in"].min() >= 0 and frames["wavelet_in"].max() <= 1.0 + 1e-6                # gamma-encoded, not 16-bit
    assert float(np.abs(out3.astype(np.float64) - out0).max()) / 65535 <= (2.2 * 11 + 4) * 2.0 ** -24   # d(x^2.2) <= 2.2 dx on [0, 1]; + the float32 roundings of the two power steps
    seen.clear()
    out4, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), local_contrast=[[1.0, 3.0, 3.0]], **kw)
    assert seen == [("wavelet", (93, 103, 3), np.float32, (1.0, 3.0, 3.0), None, 1.0, "vector")]
    assert out4.min() >= 0 and out4.max() <= 65535 and not np.array_equal(out4, out0)                    # lifted, and clipped afterwards
