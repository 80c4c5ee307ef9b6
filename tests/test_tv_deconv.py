"""CPU: the specification of the TV-regularised deconvolution (tests/tv_deconv_ref.py) beats the Wiener filter in the three quality
cases, keeps a constant frame, and its options do what they say; its float32 evaluation stays within a quarter of the GPU gate at every
GPU case; and the host layers above the kernels (lib._native.tv_deconvolve_args / tv_deconvolve_plan, deconvolve._nonblind_args,
lib.utils.tv_deconvolve) accept and refuse what they state.  The GPU side: tests/test_gpu_tv_deconv.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import tv_deconv_ref as tr
import wiener_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_CASES = [(shape, K, coupling) for shape, K in wr.GPU_SHAPES for coupling in tr.COUPLINGS]


def rms(a):
    return float(np.sqrt((a ** 2).mean()))


# ---- the specification ------------------------------------------------------------------------------------------------------------------
def test_the_three_quality_cases_beat_the_wiener_filter():
    for sharp, blurred, psf in wr.quality_cases():
        w = rms(wr.wiener(blurred, psf, 0.01) - sharp)
        for coupling in tr.COUPLINGS:
            t = rms(tr.tv_deconvolve(blurred, psf, coupling=coupling) - sharp)
            print("%s %s: blurred %.4f, wiener %.4f, tv %.4f" % (blurred.shape[:2], coupling, rms(blurred - sharp), w, t))
            assert t < w


def test_a_constant_frame_comes_back_constant():
    f = np.full((33, 47, 3), 0.37)
    for coupling in tr.COUPLINGS:
        assert np.abs(tr.tv_deconvolve(f, wr.three_psfs(7), coupling=coupling) - 0.37).max() <= 1e-12


def test_the_options_change_the_result():
    f, k = wr.frame(40, 52, 7), wr.three_psfs(5)
    ten = tr.tv_deconvolve(f, k)
    assert np.abs(ten - tr.tv_deconvolve(f, k, coupling="channel")).max() > 1e-4
    assert np.abs(ten - tr.tv_deconvolve(f, k, iterations=9)).max() > 1e-5
    assert np.abs(tr.tv_deconvolve(f, k, iterations=1) - f).max() > 1e-3


# ---- float32 against float64 at the GPU cases -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_case(shape, K, coupling, iterations=tr.ITERATIONS):
    """frame, PSF and the float64 reference of one GPU case (shared with tests/test_gpu_tv_deconv.py)"""
    f = wr.frame(shape[0], shape[1], 7).astype(np.float32)
    k = wr.three_psfs(K).astype(np.float32)
    ref = tr.tv_deconvolve(f.astype(np.float64), normalised(k).astype(np.float64), tr.FIDELITY, tr.PENALTY, iterations, coupling)
    for a in (f, k, ref):
        a.setflags(write=False)
    return f, k, ref


def normalised(k):
    """what tv_deconvolve_args hands to the library"""
    k64 = k.astype(np.float64)
    return (k64 / k64.sum(axis=(0, 1))).astype(np.float32)


def gate(ref):
    return wr.GATE * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("shape,K,coupling", GPU_CASES)
def test_float32_evaluation_is_within_a_quarter_of_the_gate(shape, K, coupling):
    f, k, ref = gpu_case(shape, K, coupling)
    got = tr.tv_deconvolve(f, normalised(k), tr.FIDELITY, tr.PENALTY, tr.ITERATIONS, coupling, np.float32)
    assert got.dtype == np.float32
    err, bound = float(np.abs(got - ref).max()), 0.25 * gate(ref)
    print("float32 - float64: %.3g (bound %.3g, max |ref| %.3g)" % (err, bound, np.abs(ref).max()))
    assert err <= bound


# ---- the host layers ------------------------------------------------------------------------------------------------------------------------------
def test_tv_deconvolve_args_accepts_and_refuses_what_it_states():
    from lib import _native
    k, mu, beta, n, coupling = _native.tv_deconvolve_args(2.0 * np.ones((5, 5)), 2000, 10, 10, "vector", (40, 52, 3))
    assert k.shape == (5, 5, 3) and k.dtype == np.float32 and k.flags.c_contiguous
    assert np.array_equal(k, np.full((5, 5, 3), np.float32(1 / 25)))
    assert (mu, beta, n, coupling) == (2000.0, 10.0, 10, "vector") and isinstance(mu, float) and isinstance(beta, float) and isinstance(n, int)
    assert _native.tv_deconvolve_args(np.ones((3, 3)), 1, 1, 500, "channel", (3, 3))[1:] == (1.0, 1.0, 500, "channel")
    assert np.array_equal(k, _native.wiener_args(2.0 * np.ones((5, 5)), 0.01, (40, 52, 3))[0])
    bad_psf = [np.ones((4, 4)), np.ones((1, 1)), np.ones((257, 257)), np.ones((3, 5)), np.ones((3, 3, 2)), np.ones(3), np.ones((7, 7)),
               np.full((3, 3), np.nan), np.full((3, 3), np.inf), np.zeros((3, 3)), -np.ones((3, 3)),
               np.dstack([np.ones((3, 3)), np.ones((3, 3)), np.zeros((3, 3))]), "box"]
    for psf in bad_psf:
        with pytest.raises(ValueError):
            _native.tv_deconvolve_args(psf, 2000, 10, 10, "vector", (6, 300, 3))
    for v in (0, -1, np.nan, np.inf, "x"):
        with pytest.raises(ValueError):
            _native.tv_deconvolve_args(np.ones((3, 3)), v, 10, 10, "vector", (6, 300, 3))
        with pytest.raises(ValueError):
            _native.tv_deconvolve_args(np.ones((3, 3)), 2000, v, 10, "vector", (6, 300, 3))
    for n in (0, -1, 2.5, 501, "x"):
        with pytest.raises(ValueError):
            _native.tv_deconvolve_args(np.ones((3, 3)), 2000, 10, n, "vector", (6, 300, 3))
    for coupling in ("luma", None, 1):
        with pytest.raises(ValueError):
            _native.tv_deconvolve_args(np.ones((3, 3)), 2000, 10, 10, coupling, (6, 300, 3))


def test_tv_deconvolve_plan_returns_the_sizes_of_the_specification():
    from lib import _native
    for H, W, K in [(5, 7, 3), (40, 52, 5), (60, 60, 5), (61, 61, 5), (70, 150, 9), (16, 2040, 9), (8170, 24, 23), (4096, 4096, 15), (4000, 6000, 45),
                    (8190, 8190, 3)]:
        plan = _native.tv_deconvolve_plan(H, W, K)
        wplan = _native.wiener_plan(H, W, K)
        assert (plan.Py, plan.Px) == wr.sizes(H, W, K) == tuple(wplan[:2])
        planes = 3 * 4 * plan.Py * plan.Px                          # three real planes
        # 11 floats per transform point and channel, and the Wiener filter's tables (its own block is two spectrum frames and them)
        assert plan.workspace_bytes - 11 * planes == wplan.workspace_bytes - 4 * planes > 0
        # the tables are 2 K / Py of three planes and a little: below one of them unless the frame is only a few taps high
        if plan.Py > 3 * K:
            assert 10 * planes < plan.workspace_bytes < 12 * planes, (H, W, K, plan.workspace_bytes / planes)
    for H, W, K in [(16, 8192, 3), (8192, 16, 3), (8171, 24, 23)]:
        with pytest.raises(_native.NativeError) as ei:
            _native.tv_deconvolve_plan(H, W, K)
        assert ei.value.code == -6 and "8192" in str(ei.value)        # ICS_ENOSUP, the message names the limit
    for H, W, K in [(40, 52, 4), (40, 52, 1), (40, 52, 257), (4, 52, 5), (40, 4, 5), (0, 5, 3)]:
        with pytest.raises(_native.NativeError) as ei:
            _native.tv_deconvolve_plan(H, W, K)
        assert ei.value.code == -1


def test_nonblind_args_takes_the_tv_forms_and_keeps_the_old_answers():
    import deconvolve as dv
    assert dv._nonblind_args("rl") is None
    assert dv._nonblind_args("wiener") == 0.01
    assert dv._nonblind_args(("wiener", 0.1)) == 0.1
    assert dv._nonblind_args("tv") == ("tv", 2000.0, 10, "vector")
    assert dv._nonblind_args(("tv", 500)) == ("tv", 500.0, 10, "vector")
    assert dv._nonblind_args(["tv", 500, 20]) == ("tv", 500.0, 20, "vector")
    assert dv._nonblind_args(("tv", 1e4, 3, "channel")) == ("tv", 1e4, 3, "channel")
    for bad in (("tv", 0), ("tv", 2000, 0), ("tv", 2000, 10, "x"), ("tv", 2000, 10, "vector", 1), "TV", ("tv",), ("tv", np.nan), ("tv", 2000, 2.5),
                ("tv", 2000, 501)):
        with pytest.raises(ValueError):
            dv._nonblind_args(bad)
    with pytest.raises(ValueError):                                   # refused before the picture is touched
        dv.deblur_module(None, "x", ".", 5, nonblind=("tv", -1))


def test_the_two_entries_exist_with_their_signatures():
    from lib import _native
    lib = _native.load()
    assert len(lib.ics_img_tv_deconvolve.argtypes) == 8 and len(lib.ics_img_tv_deconvolve_plan.argtypes) == 6
    assert lib.ics_img_tv_deconvolve.restype is C.c_int and lib.ics_img_tv_deconvolve_plan.restype is C.c_int
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    assert ("int ics_img_tv_deconvolve(const ics_img *src, const float *psf, int K, float fidelity, float penalty, int iterations, int coupling, "
            "ics_img **out);") in header
    assert "int ics_img_tv_deconvolve_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);" in header
    assert int(re.search(r"#define ICS_IMG_TVD_MAX_ITERATIONS (\d+)", header).group(1)) == _native.IMG_TVD_MAX_ITERATIONS == tr.MAX_ITERATIONS == 500
    assert lib.ics_abi_version() == 4
    # the native entry refuses by itself what the Python layer refuses before it
    out = C.c_void_p()
    fake = C.c_void_p(1)
    psf = (C.c_float * 27)(*([1 / 9] * 27))
    for args in [(0.0, 10.0, 10, 1), (float("nan"), 10.0, 10, 1), (2000.0, -1.0, 10, 1), (2000.0, float("inf"), 10, 1), (2000.0, 10.0, 0, 1),
                 (2000.0, 10.0, 501, 1), (2000.0, 10.0, 10, 2)]:
        assert lib.ics_img_tv_deconvolve(fake, psf, 3, *args, C.byref(out)) == _native.ICS_EINVAL, args
    assert lib.ics_img_tv_deconvolve(None, psf, 3, 2000.0, 10.0, 10, 1, C.byref(out)) == _native.ICS_EINVAL


def test_utils_tv_deconvolve_has_no_cpu_fallback():
    from lib import _native, utils
    with pytest.raises(ValueError):                                   # refused before anything is uploaded
        utils.tv_deconvolve(np.zeros((10, 10, 3)), np.ones((4, 4)))
    with pytest.raises(ValueError):
        utils.tv_deconvolve(np.zeros((10, 10)), np.ones((3, 3)))
    if _native.device_count() == 0:
        with pytest.raises(_native.NativeError) as ei:
            utils.tv_deconvolve(np.zeros((10, 10, 3)), np.ones((3, 3)))
        assert ei.value.code == _native.ICS_ENODEV
