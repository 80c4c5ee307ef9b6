"""CPU: the oracle of the TV denoiser (tests/tv_denoise_ref.py, Chambolle's dual projection with tau = 1/8) checked against what
the algorithm guarantees, and the surface of ics_img_tv_denoise / DeviceImage.tv_denoise / lib.utils.tv_denoise /
deblur_module(denoise=...) as far as it can be checked without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tv_denoise_ref as tvr
from test_gpu_img_filters import picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ics_hip.h")


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
def test_zero_iterations_is_the_identity_and_a_constant_picture_a_fixed_point(coupling):
    pic = picture(23, 31, seed=1)
    out = tvr.tv_denoise(pic, 0.1, 0, coupling)
    assert out.dtype == np.float64 and np.array_equal(out, pic.astype(np.float64))
    assert out is not pic
    const = np.full((17, 19, 3), 0.37) * np.array([1.0, 0.5, 2.0])
    for dtype in (np.float64, np.float32):
        assert np.array_equal(tvr.tv_denoise(const, 0.1, 30, coupling, dtype=dtype), const.astype(dtype))


@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
def test_the_mean_of_every_channel_is_preserved(coupling):
    """div q sums to zero over the picture (every q value enters once with + and once with -, the last row / column of qy / qx is 0
    because g is 0 there), so sum(u) = sum(f) up to the rounding of H W additions: a few float64 ulps of the values times H W."""
    H, W = 301, 287
    pic = picture(H, W, seed=2).astype(np.float64)
    out = tvr.tv_denoise(pic, 0.1, 50, coupling)
    gate = 8 * 2.0 ** -53 * H * W                       # on the sums; values are in [0, 1]
    for c in range(3):
        assert abs(out[..., c].sum() - pic[..., c].sum()) <= gate, (c, out[..., c].sum() - pic[..., c].sum(), gate)


@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
def test_the_rof_energy_does_not_increase(coupling):
    pic = picture(301, 287, seed=3)
    e = [tvr.rof_energy(tvr.tv_denoise(pic, 0.1, k, coupling), pic, 0.1, coupling) for k in (0, 1, 2, 5, 50)]
    print("ROF energy, %s coupling, k = 0, 1, 2, 5, 50: %s" % (coupling, [round(v, 1) for v in e]))
    assert all(b <= a for a, b in zip(e, e[1:])), e
    assert e[-1] < 0.5 * e[0], e                        # and it is a denoiser: TV of the noisy picture dominates the start


def test_vector_coupling_on_equal_planes_is_channel_coupling_with_a_scaled_weight():
    """three equal planes: s_vector = 3 s_channel, so 1 + (tau / w) sqrt(3 s) is the channel denominator at weight w / sqrt(3)"""
    plane = picture(60, 47, seed=4)[..., :1].astype(np.float64)
    same = np.repeat(plane, 3, axis=2)
    v = tvr.tv_denoise(same, 0.1, 50, "vector")
    ch = tvr.tv_denoise(same, 0.1 / np.sqrt(3.0), 50, "channel")
    assert np.array_equal(v[..., 0], v[..., 1]) and np.array_equal(v[..., 0], v[..., 2])
    assert np.max(np.abs(v - ch)) <= 64 * 2.0 ** -53     # 50 iterations of a contraction, a few ulps each; values in [0, 1]


@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
def test_permuting_the_channels_permutes_the_output(coupling):
    """exact for both couplings: the vector sum takes its three terms in ascending order, whatever channel they come from"""
    pic = picture(40, 33, seed=5)
    out = tvr.tv_denoise(pic, 0.1, 30, coupling)
    for order in ([2, 0, 1], [1, 0, 2]):
        assert np.array_equal(tvr.tv_denoise(np.ascontiguousarray(pic[..., order]), 0.1, 30, coupling), out[..., order])


def test_channel_coupling_does_not_mix_the_channels_and_vector_coupling_does():
    pic = picture(40, 33, seed=6)
    other = pic.copy()
    other[..., 1] = picture(40, 33, seed=7)[..., 1]
    a, b = tvr.tv_denoise(pic, 0.1, 20, "channel"), tvr.tv_denoise(other, 0.1, 20, "channel")
    assert np.array_equal(a[..., 0], b[..., 0]) and np.array_equal(a[..., 2], b[..., 2])
    a, b = tvr.tv_denoise(pic, 0.1, 20, "vector"), tvr.tv_denoise(other, 0.1, 20, "vector")
    assert not np.array_equal(a[..., 0], b[..., 0])


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_function_and_keeps_the_abi_version():
    from lib import _native
    raw = open(HEADER).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    assert "int ics_img_tv_denoise(const ics_img *src, float weight, int iterations, int coupling, int route, ics_img **out);" in text
    assert "#define ICS_ABI_VERSION 4 " in text
    assert int(re.search(r"#define ICS_IMG_TV_BLOCK (\d+)", raw).group(1)) == _native.IMG_TV_BLOCK
    kh = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")).read()
    assert int(re.search(r"#define ICS_IMG_TV_BLOCK (\d+)", kh).group(1)) == _native.IMG_TV_BLOCK


def test_native_binds_it_and_refuses_bad_arguments_before_any_device_work():
    from lib import _native
    lib = _native.load()
    vp, ci, cf, pvp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)
    assert lib.ics_img_tv_denoise.argtypes == [vp, cf, ci, ci, ci, pvp] and lib.ics_img_tv_denoise.restype is ci
    assert callable(_native.DeviceImage.tv_denoise)
    out = C.c_void_p()
    assert lib.ics_img_tv_denoise(None, 0.1, 5, 0, 0, C.byref(out)) == _native.ICS_EINVAL
    fake = C.c_void_p(8)    # never dereferenced: the arguments are checked first
    assert lib.ics_img_tv_denoise(fake, 0.1, 5, 0, 0, None) == _native.ICS_EINVAL
    for weight, iterations, coupling, route, word in ((0.0, 5, 0, 0, b"weight"), (-1.0, 5, 0, 0, b"weight"), (float("nan"), 5, 0, 0, b"weight"),
                                                      (float("inf"), 5, 0, 0, b"weight"), (0.1, -1, 0, 0, b"iterations"), (0.1, 5, 2, 0, b"coupling"),
                                                      (0.1, 5, -1, 0, b"coupling"), (0.1, 5, 1, 3, b"route"), (0.1, 5, 1, -1, b"route")):
        assert lib.ics_img_tv_denoise(fake, weight, iterations, coupling, route, C.byref(out)) == _native.ICS_EINVAL, (weight, iterations, coupling, route)
        assert word in lib.ics_last_error()
    assert out.value is None


def test_utils_tv_denoise_rejects_what_is_no_rgb_picture():
    from lib import utils
    for bad in (np.zeros((8, 9)), np.zeros((8, 9, 4)), np.zeros((3, 8, 9, 3)), np.zeros(7)):
        with pytest.raises(ValueError, match="H x W x 3"):
            utils.tv_denoise(bad)


def test_deblur_module_validates_denoise():
    import deconvolve as dv
    pic = np.full((64, 64, 3), 128, np.uint8)
    for bad in ((0.1,), (), (0.1, 5, "vector", 1), (0.1, 5, "colour"), (0.0, 5), (-0.1, 5), (float("nan"), 5), (float("inf"), 5), (0.1, -1), (0.1, 2.5)):
        with pytest.raises(ValueError, match="denoise"):
            dv.deblur_module(pic, "x", ".", 5, save=False, display=False, denoise=bad)
    assert dv._denoise_args(None) is None
    assert dv._denoise_args((0.1, 20)) == (0.1, 20, "vector") and dv._denoise_args([0.05, 7, "channel"]) == (0.05, 7, "channel")


def _recording_solver(calls):
    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd, **kw):
        calls.append((image.copy(), u.copy(), psf.copy(), (top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd), kw))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]
    return solver


def test_deblur_module_host_driver_denoises_before_it_sharpens(monkeypatch, capsys):
    """denoise=None never calls utils.tv_denoise and changes nothing; with both arguments the host driver hands the deblurred frame
    to tv_denoise first and its result to USM (stand-ins record the order and answer with the oracle: no GPU here)"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    import utils_oracle as uo
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)
    seen = []

    def tv(src, weight=0.1, iterations=50, coupling="vector"):
        seen.append(("tv", src.shape, src.dtype, weight, iterations, coupling))
        return tvr.tv_denoise(src, weight, iterations, coupling, dtype=np.float32)

    def usm(src, radius, strength, amount, method="bessel"):
        seen.append(("usm", src.shape))
        return uo.USM(np.asarray(src, np.float64), radius, strength, amount, method)
    monkeypatch.setattr(dv.utils, "tv_denoise", tv)
    monkeypatch.setattr(dv.utils, "USM", usm)
    pic = (np.random.default_rng(0).random((90, 100, 3)) * 255).astype(np.uint8)
    kw = dict(mask=[46, 50], mask_size=41, display=False, pyramid=False, save=False, iterations=7)
    base, none, both = [], [], []
    out0, psf0 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(base), **kw)
    out1, psf1 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(none), denoise=None, **kw)
    assert seen == [] and out0.dtype == out1.dtype and np.array_equal(out0, out1) and np.array_equal(psf0, psf1)
    out2, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(both), denoise=(0.05, 10), sharpen=(9, 4., 0.5), **kw)
    assert seen == [("tv", (93, 103, 3), np.float32, 0.05, 10, "vector")] + [("usm", (93, 103))] * 3
    assert len(base) == len(both) == 2
    for x, y in zip(base, both):                                      # the solver sees nothing of it
        assert x[3] == y[3] and x[4] == y[4] and all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))
    assert out2.shape == out0.shape and out2.min() >= 0 and out2.max() <= 65535 and not np.array_equal(out0, out2)
    seen.clear()
    dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), denoise=[0.2, 3, "channel"], **kw)
    assert seen == [("tv", (93, 103, 3), np.float32, 0.2, 3, "channel")]
