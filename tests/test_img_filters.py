"""CPU: the surface of the device-resident RGB filters (ics_img_convolve / ics_img_usm / ics_img_bilateral, DeviceImage.convolve /
gaussian_blur / bessel_blur / usm / bilateral, lib.utils dispatch, deblur_module(sharpen=...)) as far as it can be checked without a
GPU: declarations, bindings, argument handling, that the default call into the solver is unchanged, and that the gfx950 code
of csrc/ics_img_filters.hip uses no scratch memory."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ics_hip.h")


def test_header_declares_the_three_functions_and_keeps_the_abi_version():
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    assert "int ics_img_convolve(const ics_img *src, const float *kern, int KH, int KW, ics_img **out);" in text
    assert "int ics_img_usm(const ics_img *src, const float *kern, int KH, int KW, float amount, ics_img **out);" in text
    assert "int ics_img_bilateral(const ics_img *src, int radius, float std_i, float std_s, ics_img **out);" in text
    assert "#define ICS_ABI_VERSION 4 " in text


def test_native_binds_them_with_the_declared_argument_types():
    from lib import _native
    lib = _native.load()
    vp, ci, cf, pvp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)
    assert lib.ics_img_convolve.argtypes == [vp, vp, ci, ci, pvp] and lib.ics_img_convolve.restype is ci
    assert lib.ics_img_usm.argtypes == [vp, vp, ci, ci, cf, pvp] and lib.ics_img_usm.restype is ci
    assert lib.ics_img_bilateral.argtypes == [vp, ci, cf, cf, pvp] and lib.ics_img_bilateral.restype is ci
    for name in ("convolve", "gaussian_blur", "bessel_blur", "usm", "bilateral"):
        assert callable(getattr(_native.DeviceImage, name)), name


def test_null_and_bad_arguments_are_refused_before_any_device_work():
    """ICS_EINVAL in the style of the neighbouring functions: checked before the image is touched, so no GPU is needed"""
    from lib import _native
    lib = _native.load()
    out = C.c_void_p()
    k = np.ones((3, 3), np.float32)
    kp = k.ctypes.data_as(C.c_void_p)
    assert lib.ics_img_convolve(None, kp, 3, 3, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_usm(None, kp, 3, 3, 0.5, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_bilateral(None, 2, 0.1, 1.0, C.byref(out)) == _native.ICS_EINVAL
    assert b"NULL" in lib.ics_last_error()
    fake = C.c_void_p(8)    # never dereferenced: the arguments are checked first
    assert lib.ics_img_convolve(fake, None, 3, 3, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_convolve(fake, kp, 0, 3, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_usm(fake, kp, 3, -1, 0.5, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_usm(fake, kp, 3, 3, 0.5, None) == _native.ICS_EINVAL
    assert lib.ics_img_bilateral(fake, -1, 0.1, 1.0, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_bilateral(fake, 2, 0.0, 1.0, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_bilateral(fake, 2, 0.1, -1.0, C.byref(out)) == _native.ICS_EINVAL
    assert lib.ics_img_bilateral(fake, 35, 0.1, 1.0, C.byref(out)) == _native.ICS_ENOSUP     # tile + halo beyond 160 KB of LDS
    assert b"radius 35" in lib.ics_last_error()
    assert out.value is None


def _recording_solver(calls):
    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd, **kw):
        calls.append(dict(image=image.copy(), u=u.copy(), psf=psf.copy(), args=(top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd), kw=kw))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]
    return solver


def _same_calls(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["args"] == y["args"] and x["kw"] == y["kw"]
        for key in ("image", "u", "psf"):
            assert x[key].dtype == y[key].dtype and np.array_equal(x[key], y[key]), key


def test_deblur_module_sharpen_none_calls_the_solver_exactly_as_without_it(monkeypatch, capsys):
    import deconvolve as dv
    import rl_mm_oracle as orc
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)   # no GPU in this test: oracle as stand-in
    monkeypatch.setattr(dv.utils, "USM", lambda *a, **k: pytest.fail("USM called although sharpen is None"))
    rng = np.random.default_rng(0)
    pic = (rng.random((90, 100, 3)) * 255).astype(np.uint8)
    kw = dict(mask=[46, 50], mask_size=41, display=False, pyramid=False, save=False, iterations=7, tolerance=2, confidence=10)
    base, with_none = [], []
    out0, psf0 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(base), **kw)
    out1, psf1 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(with_none), sharpen=None, **kw)
    assert len(base) == 2 and base[0]["kw"]["blind"] is True and base[1]["kw"]["blind"] is False     # tests/test_driver.py: blind window, full frame
    assert base[0]["args"][:4] == (3, 38, 3, 38) and base[0]["args"][5:9] == (43, 43, 3, 5) and base[1]["args"][5:9] == (95, 105, 3, 5)
    _same_calls(base, with_none)
    assert out0.dtype == out1.dtype and np.array_equal(out0, out1) and np.array_equal(psf0, psf1)


def test_deblur_module_sharpen_on_the_host_driver_is_usm_per_channel_before_the_clip(monkeypatch, capsys):
    """the host driver calls utils.USM on each channel as a user would; a stand-in records what it is given (no GPU here)"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    import utils_oracle as uo
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)
    seen = []

    def usm(src, radius, strength, amount, method="bessel"):
        seen.append((src.shape, radius, strength, amount, method))
        return uo.USM(np.asarray(src, np.float64), radius, strength, amount, method)
    monkeypatch.setattr(dv.utils, "USM", usm)
    rng = np.random.default_rng(0)
    pic = (rng.random((90, 100, 3)) * 255).astype(np.uint8)
    kw = dict(mask=[46, 50], mask_size=41, display=False, pyramid=False, save=False, iterations=7)
    calls, calls_s = [], []
    out0, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(calls), **kw)
    out1, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(calls_s), sharpen=(9, 4., 0.5), **kw)
    _same_calls(calls, calls_s)                                        # the solver sees nothing of it
    assert seen == [((93, 103), 9, 4., 0.5, "bessel")] * 3
    assert out1.shape == out0.shape == (90, 100, 3) and out1.min() >= 0 and out1.max() <= 65535
    assert not np.array_equal(out0, out1)
    seen.clear()
    dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), sharpen=[5, 1.5, 1.0, "gauss"], **kw)
    assert seen == [((93, 103), 5, 1.5, 1.0, "gauss")] * 3


def test_deblur_module_rejects_a_sharpen_tuple_of_the_wrong_length():
    import deconvolve as dv
    pic = np.full((64, 64, 3), 128, np.uint8)
    for bad in ((9, 4.), (9,), (9, 4., 0.5, "bessel", 1), ()):
        with pytest.raises(ValueError, match="sharpen"):
            dv.deblur_module(pic, "x", ".", 5, save=False, display=False, sharpen=bad)
    with pytest.raises(ValueError, match="sharpen"):
        dv.deblur_module(pic, "x", ".", 5, save=False, display=False, sharpen=(9, 4., 0.5, "median"))


def test_utils_filters_keep_their_float64_path_for_arrays(monkeypatch):
    """dispatch does not leak: a 2-D array still goes to Context.usm / conv2d_symm / bilateral as float64 and comes back as float64,
    a 3-D array still raises.  (The context is a stand-in that answers with the oracle: no GPU here.)"""
    import utils_oracle as uo
    from lib import _native, utils

    class Ctx:
        def usm(self, src, kern, amount):
            assert src.dtype == np.float64 and src.ndim == 2 and kern.dtype == np.float64
            return src + (src - uo.conv2d_symm(src, kern)) * amount

        def conv2d_symm(self, src, kern):
            assert src.dtype == np.float64 and src.ndim == 2
            return uo.conv2d_symm(src, kern)

        def bilateral(self, src, radius, std_i, std_s):
            assert src.dtype == np.float64 and src.ndim == 2
            return uo.bilateral_filter(src, radius, std_i, std_s)
    monkeypatch.setattr(_native.Context, "get", classmethod(lambda cls, device=None: Ctx()))
    rng = np.random.default_rng(3)
    src = rng.random((20, 17)).astype(np.float32)
    out = utils.USM(src, 5, 3.0, 0.7)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and np.array_equal(out, uo.USM(src.astype(np.float64), 5, 3.0, 0.7))
    assert utils.gaussian_blur(src, 7, 1.5).dtype == np.float64 and utils.bessel_blur(src, 9, 4.0).dtype == np.float64
    assert utils.bilateral_filter(src, 2, 0.1, 1.0).dtype == np.float64
    pic = rng.random((8, 9, 3))
    for f, args in ((utils.USM, (5, 3.0, 0.7)), (utils.gaussian_blur, (7, 1.5)), (utils.bessel_blur, (9, 4.0)), (utils.bilateral_filter, (2, 0.1, 1.0))):
        with pytest.raises(ValueError, match="2-D channel"):
            f(pic, *args)


def test_img_filter_kernels_use_no_scratch(tmp_path):
    """every kernel of csrc/ics_img_filters.hip in the gfx950 code object: no private segment, no spilled register (read from the
    AMDGPU metadata of the cross-compiled library like tests/test_isa.py)"""
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_filters.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_bilateral", "k_img_conv_cols", "k_img_conv_rows"]
    tab = kernel_table(tmp_path)
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v["vgpr_count"] <= 64, (k, v)       # 8 waves per SIMD as far as registers go: LDS sets the occupancy
