"""CPU: the oracle of the fast local Laplacian filter (tests/llf_ref.py) checked against what the filter must be -- a linear remap
scales the Laplacian pyramid, more samples converge on the exact (unsampled) filter, the identity remap and a constant picture come
back bit for bit in float32 -- and the surface of ics_img_local_laplacian / DeviceImage.local_laplacian / lib.utils.local_laplacian /
deblur_module(clarity=...) as far as it can be checked without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import llf_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ics_hip.h")


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5, 8])
def test_a_linear_remap_scales_every_detail_level_whatever_the_number_of_samples(K):
    """detail == edges == s makes r_g(i) = g + s (i - g), affine in i and in g: every L_k[l] is s L[l] plus the Laplacian of a constant
    (zero), so the interpolation between samples returns s L[l] for any K, and the result is the pyramid with its detail levels
    scaled by s, collapsed.  Float64 roundings only: 1e-12 (measured 1e-15)."""
    pic = np.random.default_rng(41).random((41, 30))
    J = 3
    for s in (0.5, 1.0, 1.75):
        lap = lr.laplacian_pyramid(pic, J)
        expect = lr.collapse([s * lap[l] for l in range(J)] + [lap[J]])
        err = worst(lr.filter_plane(pic, 0.2, s, s, J, K), expect)
        print("linear remap s %g K %d: %.3e" % (s, K, err))
        assert err <= 1e-12, (s, K, err)


def test_sampling_converges_on_the_exact_filter():
    """a sine, a step and mild noise, 24 x 20, J = 2, sigma 0.25, detail 2, edges 0.8: the worst error against the filter that remaps
    about every coefficient's own g falls as K grows; linear interpolation of a smooth function of g with spacing 1 / (K - 1) errs
    as the spacing squared, so a doubling of K - 1 should quarter it: at least a halving is asserted, and 1 / 16 from K = 5 to 33
    (three doublings: 1 / 64 expected)."""
    y, x = np.mgrid[0:24, 0:20]
    pic = 0.45 + 0.2 * np.sin(x / 3.0 + y / 5.0) + 0.25 * (x > 11) + 0.02 * (np.random.default_rng(3).random((24, 20)) - 0.5)
    assert 0 <= pic.min() and pic.max() <= 1
    args = (0.25, 2.0, 0.8)
    ref = lr.exact_plane(pic, *args, 2)
    errs = {K: worst(lr.filter_plane(pic, *args, 2, K), ref) for K in (3, 5, 9, 17, 33)}
    print("sampled against exact:", {K: "%.3e" % e for K, e in errs.items()})
    assert errs[33] <= errs[5] / 16, errs
    for a, b in ((3, 5), (5, 9), (9, 17), (17, 33)):
        assert errs[b] <= errs[a] / 2, (a, b, errs)


@pytest.mark.parametrize("shape", [(37, 45), (1, 9), (9, 1), (5, 7), (64, 64), (65, 65)])
def test_the_identity_remap_returns_the_picture_bit_for_bit_in_float32(shape):
    """values in {0, 1/4, 1/2, 3/4}, K = 5 (the samples are these values and 1), detail = edges = 1: d = i - g, g + d, every tap sum
    (multiples of 2^-10 below 16 at level 1, of 2^-18 at level 2), every expand and every difference is exactly representable in
    float32, a = b so the blend adds f * 0, and P - expand(P') + expand(P') returns P.  Per channel: the luma of such a pixel has a
    full mantissa, so "vector" is exact only in what it adds to a constant (below)."""
    pic = (np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 4, shape + (3,)) / 4.0).astype(np.float32)
    for J in (1, 2):
        out = lr.local_laplacian(pic, 0.2, 1.0, 1.0, levels=J, samples=5, coupling="channel", dtype=np.float32)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), pic.view(np.uint32)), (J, worst(out, pic))
        for c in range(3):
            assert np.array_equal(lr.filter_plane(pic[..., c], 0.2, 1.0, 1.0, J, 5, np.float32), pic[..., c])


@pytest.mark.parametrize("coupling", lr.COUPLINGS)
def test_a_constant_picture_is_returned_bit_for_bit_for_any_arguments(coupling):
    """0.375 x (1, 1/2, 2): with the weight 6 of the taps split into 2 + 4 every partial sum of a constant c is c times a power of
    two, so every level of every pyramid is c exactly whatever the bits of the remapped c, every Laplacian coefficient is +0, and the
    collapse returns G[J] = the constant.  (With ((a0 + a4) + 4 (a1 + a3)) + 6 a2 the sums 10 c and 6 c round, and sigma 0.3, detail
    1.7, edges 0.9, K = 8, J = 6 came back an ulp off.)"""
    const = np.full((37, 45, 3), np.float32(0.375), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    for J in (1, 3, 6):
        for args, K in (((0.2, 2.0, 0.8), 8), ((0.05, 0.5, 1.0), 5), ((0.3, 1.7, 0.9), 8), ((1.0, 3.0, 1.0), 2), ((0.01, 0.0, 0.25), 16), ((0.7, 0.3, 2.5), 3)):
            out = lr.local_laplacian(const, *args, levels=J, samples=K, coupling=coupling, dtype=np.float32)
            assert np.array_equal(out.view(np.uint32), const.view(np.uint32)), (J, args, K, worst(out, const))


def test_default_levels_and_the_fold():
    from lib import _native
    for H, W in ((1, 1), (16, 9), (17, 1), (120, 131), (4096, 4096), (3, 20000), (2 ** 20, 5)):
        assert _native.llf_levels(H, W) == lr.default_levels(H, W)
    assert [lr.default_levels(n, 1) for n in (16, 17, 32, 33, 4096, 2 ** 20)] == [1, 1, 1, 2, 8, 10]
    assert list(lr.symm(np.arange(-7, 10), 3)) == list(np.pad(np.arange(3), 7, mode="symmetric"))       # ... at any distance
    assert list(lr.symm(np.arange(-2, 3), 1)) == [0] * 5


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_function_and_the_constants():
    from lib import _native
    raw = open(HEADER).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    assert ("int ics_img_local_laplacian(const ics_img *src, float sigma, float detail, float edges, int levels, int samples, int coupling, int route, "
            "ics_img **out);") in text
    assert "#define ICS_ABI_VERSION 4 " in text
    kh = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")).read()
    for src in (raw, kh):
        assert int(re.search(r"#define ICS_IMG_LLF_MAX_LEVELS (\d+)", src).group(1)) == _native.IMG_LLF_MAX_LEVELS == lr.MAX_LEVELS == 10
        assert int(re.search(r"#define ICS_IMG_LLF_MAX_SAMPLES (\d+)", src).group(1)) == _native.IMG_LLF_MAX_SAMPLES == lr.MAX_SAMPLES == 16


def test_native_binds_it_and_refuses_bad_arguments_before_any_device_work():
    from lib import _native
    lib = _native.load()
    vp, ci, cf, pvp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)
    assert lib.ics_img_local_laplacian.argtypes == [vp, cf, cf, cf, ci, ci, ci, ci, pvp] and lib.ics_img_local_laplacian.restype is ci
    out = C.c_void_p()
    fake = C.c_void_p(8)    # never dereferenced: the arguments are checked first
    ok = (0.2, 1.8, 1.0, 3, 8, 1, 0)
    assert lib.ics_img_local_laplacian(None, *ok, C.byref(out)) == _native.ICS_EINVAL and b"NULL" in lib.ics_last_error()
    assert lib.ics_img_local_laplacian(fake, *ok, None) == _native.ICS_EINVAL
    nan, inf = float("nan"), float("inf")
    above = float(np.nextafter(np.float32(3 * 0.8), np.float32(4)))
    for change, word in (({0: 0.0}, b"sigma"), ({0: -0.2}, b"sigma"), ({0: nan}, b"sigma"), ({0: inf}, b"sigma"),
                         ({1: -0.5}, b"detail"), ({1: nan}, b"detail"), ({1: inf}, b"detail"),
                         ({2: 0.0}, b"edges"), ({2: -1.0}, b"edges"), ({2: nan}, b"edges"), ({2: inf}, b"edges"),
                         ({1: 3.5}, b"detail"), ({1: above, 2: 0.8}, b"detail"), ({1: 1.0, 2: 0.25}, b"detail"),
                         ({3: 0}, b"levels"), ({3: 11}, b"levels"), ({3: -3}, b"levels"), ({4: 1}, b"samples"), ({4: 17}, b"samples"), ({4: 0}, b"samples"),
                         ({5: 2}, b"coupling"), ({5: -1}, b"coupling"), ({6: 3}, b"route"), ({6: -1}, b"route")):
        a = list(ok)
        for pos, value in change.items():
            a[pos] = value
        out = C.c_void_p(1)
        assert lib.ics_img_local_laplacian(fake, *a, C.byref(out)) == _native.ICS_EINVAL, (word, a)
        assert word in lib.ics_last_error() and out.value is None, (word, lib.ics_last_error(), out.value)


ABOVE = float(np.nextafter(np.float32(3 * 0.8), np.float32(4)))          # just above 3 edges at edges = float32(0.8)
BAD_ARGUMENTS = [
    (dict(sigma=0.0), "sigma"), (dict(sigma=-0.2), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma=float("inf")), "sigma"), (dict(sigma=1e-60), "sigma"),
    (dict(sigma=None), "sigma"), (dict(sigma="wide"), "sigma"),
    (dict(detail=-0.5), "detail"), (dict(detail=float("nan")), "detail"), (dict(detail=float("inf")), "detail"), (dict(detail=1e39), "detail"),
    (dict(detail=None), "detail"),
    (dict(edges=0.0), "edges"), (dict(edges=-1.0), "edges"), (dict(edges=float("nan")), "edges"), (dict(edges=float("inf")), "edges"), (dict(edges=None), "edges"),
    (dict(detail=3.5), "detail"), (dict(detail=ABOVE, edges=0.8), "detail"), (dict(detail=1.0, edges=0.25), "detail"),
    (dict(levels=0), "levels"), (dict(levels=11), "levels"), (dict(levels=2.5), "levels"), (dict(levels="3"), "levels"), (dict(levels=True), "levels"),
    (dict(samples=1), "samples"), (dict(samples=17), "samples"), (dict(samples=4.5), "samples"), (dict(samples=None), "samples"), (dict(samples=True), "samples"),
    (dict(coupling="colour"), "coupling"), (dict(coupling=1), "coupling"),
    (dict(route=3), "route"), (dict(route=-1), "route")]


def test_llf_args_device_image_and_utils_raise_value_errors_before_any_native_call(monkeypatch):
    from lib import _native, utils
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("a native call"))
    img = _native.DeviceImage(None, None)                                # no handle: nothing to destroy
    for kw, word in BAD_ARGUMENTS:
        full = dict(dict(sigma=0.2, detail=1.8), **kw)
        with pytest.raises(ValueError, match=word):
            _native.llf_args(**full)
        with pytest.raises(ValueError, match=word):
            img.local_laplacian(**full)
        if "route" not in kw:
            with pytest.raises(ValueError, match=word):
                utils.local_laplacian(np.zeros((8, 9, 3), np.float32), **full)
    for bad in (np.zeros((8, 9)), np.zeros((8, 9, 4)), np.zeros((3, 8, 9, 3)), np.zeros(7)):
        with pytest.raises(ValueError, match="H x W x 3"):
            utils.local_laplacian(bad, 0.2, 1.8)
    assert _native.llf_args(0.2, 1.8) == (0.2, 1.8, 1.0, None, 8, "vector", 0)
    assert _native.llf_args(np.float32(0.25), 3, np.float64(1), np.int64(10), 16.0, "channel", 2) == (0.25, 3.0, 1.0, 10, 16, "channel", 2)
    assert _native.llf_args(0.05, 0, 0.5, 1, 2, "vector", 1) == (0.05, 0.0, 0.5, 1, 2, "vector", 1)       # detail 0 and detail == 3 edges are legal
    assert _native.llf_args(0.2, float(np.float32(3) * np.float32(0.8)), 0.8)[1] == float(np.float32(3) * np.float32(0.8))


# ---- deblur_module(clarity=...) ---------------------------------------------------------------------------------------------------
def test_deblur_module_validates_clarity_before_it_touches_a_device(monkeypatch):
    import deconvolve as dv
    from lib import _native
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("a native call"))
    pic = np.full((64, 64, 3), 128, np.uint8)
    for bad, word in (((), "clarity"), (0.2, "clarity"), ((0.2,), "clarity"), ((0.2, 1.8, 1.0, "vector", 1), "clarity"), ((0.0, 1.8), "sigma"),
                      ((float("nan"), 1.8), "sigma"), ((0.2, -1.0), "detail"), ((0.2, float("inf")), "detail"), ((0.2, 3.5), "detail"),
                      ((0.2, ABOVE, 0.8), "detail"), ((0.2, 1.0, 0.0), "edges"), ((0.2, 1.0, float("nan")), "edges"), ((0.2, 1.8, 1.0, "colour"), "coupling")):
        for resident in (None, False, True):
            with pytest.raises(ValueError, match="clarity") as info:
                dv.deblur_module(pic, "x", ".", 5, save=False, display=False, device_resident=resident, clarity=bad)
            assert word in str(info.value)
        with pytest.raises(ValueError, match=word):
            dv._clarity_args(bad)
    assert dv._clarity_args(None) is None
    assert dv._clarity_args((0.2, 1.8)) == (0.2, 1.8, 1.0, "vector")
    assert dv._clarity_args([0.2, 1, 0.6]) == (0.2, 1.0, 0.6, "vector")
    assert dv._clarity_args((0.1, 0.5, 1.0, "channel")) == (0.1, 0.5, 1.0, "channel")


def _recording_solver(calls):
    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd, **kw):
        calls.append((image.copy(), u.copy(), psf.copy(), (top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd), kw))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]
    return solver


def test_deblur_module_applies_clarity_after_denoise_and_before_local_contrast_in_both_drivers(monkeypatch, capsys):
    """clarity=None never calls utils.local_laplacian and changes nothing; with all five arguments the host driver hands the
    deblurred gamma-encoded frame to tv_denoise, its result to local_laplacian, that to wavelet_equalizer, guided_filter and USM,
    then clips (stand-ins record the order and answer with the oracles: no GPU here).  The resident driver needs a device to run
    (tests/test_gpu_llf.py records its calls); here its source must name the five steps in the same order."""
    import deconvolve as dv
    import guided_ref as gr
    import rl_mm_oracle as orc
    import tv_denoise_ref as tvr
    import utils_oracle as uo
    import wavelet_ref as wr
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)
    seen, frames = [], {}

    def tv(src, weight=0.1, iterations=50, coupling="vector"):
        seen.append(("tv", src.shape, src.dtype, weight, iterations, coupling))
        frames["tv"] = tvr.tv_denoise(src, weight, iterations, coupling, dtype=np.float32)
        return frames["tv"]

    def llf(src, sigma, detail, edges=1.0, levels=None, samples=8, coupling="vector"):
        seen.append(("llf", src.shape, src.dtype, sigma, detail, edges, levels, samples, coupling))
        frames["llf_in"] = src.copy()
        frames["llf"] = lr.local_laplacian(src, sigma, detail, edges, levels, samples, coupling, dtype=np.float32)
        return frames["llf"]

    def wavelet(src, gains, thresholds=None, residual=1.0, coupling="vector"):
        seen.append(("wavelet", src.shape, src.dtype, tuple(gains), thresholds, residual, coupling))
        frames["wavelet_in"] = src.copy()
        return wr.wavelet_equalize(src, gains, thresholds, residual, coupling, dtype=np.float32)

    def guided(src, radius, eps, detail=0.0, coupling="vector"):
        seen.append(("guided", src.shape, src.dtype, radius, eps, detail, coupling))
        return gr.guided_filter(src, radius, eps, detail, coupling, dtype=np.float32)

    def usm(src, radius, strength, amount, method="bessel"):
        seen.append(("usm", src.shape))
        return uo.USM(np.asarray(src, np.float64), radius, strength, amount, method)
    monkeypatch.setattr(dv.utils, "tv_denoise", tv)
    monkeypatch.setattr(dv.utils, "local_laplacian", llf)
    monkeypatch.setattr(dv.utils, "wavelet_equalizer", wavelet)
    monkeypatch.setattr(dv.utils, "guided_filter", guided)
    monkeypatch.setattr(dv.utils, "USM", usm)
    pic = (np.random.default_rng(0).random((90, 100, 3)) * 255).astype(np.uint8)
    kw = dict(mask=[46, 50], mask_size=41, display=False, pyramid=False, save=False, iterations=7)
    base, none, full = [], [], []
    out0, psf0 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(base), **kw)
    out1, psf1 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(none), clarity=None, **kw)
    assert seen == [] and out0.dtype == out1.dtype and np.array_equal(out0, out1) and np.array_equal(psf0, psf1)
    assert len(base) == len(none) == 2                                    # clarity=None: the solver is called exactly as without the keyword
    for x, y in zip(base, none):
        assert x[3] == y[3] and x[4] == y[4] and all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))
    gains = (1.0, 1.6, 1.8)
    out2, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(full), denoise=(0.05, 10), sharpen=(9, 4., 0.5),
                               local_contrast=(gains,), detail=(8, 1e-3, 1.5, "channel"), clarity=(0.2, 1.8, 0.9, "channel"), **kw)
    assert seen == [("tv", (93, 103, 3), np.float32, 0.05, 10, "vector"), ("llf", (93, 103, 3), np.float32, 0.2, 1.8, 0.9, None, 8, "channel"),
                    ("wavelet", (93, 103, 3), np.float32, gains, None, 1.0, "vector"),
                    ("guided", (93, 103, 3), np.float32, 8, 1e-3, 1.5, "channel")] + [("usm", (93, 103))] * 3
    assert np.array_equal(frames["llf_in"], frames["tv"])                 # the denoised frame goes in ...
    assert np.array_equal(frames["wavelet_in"], frames["llf"])            # ... and its result on to the equaliser
    assert len(full) == 2
    for x, y in zip(base, full):                                          # the solver sees nothing of it
        assert x[3] == y[3] and x[4] == y[4] and all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))
    assert out2.shape == out0.shape and out2.min() >= 0 and out2.max() <= 65535 and not np.array_equal(out0, out2)
    # alone, with the defaults: edges 1, "vector", default levels, 8 samples, on the gamma-encoded frame
    seen.clear()
    out3, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), clarity=(0.2, 1.8), **kw)
    assert seen == [("llf", (93, 103, 3), np.float32, 0.2, 1.8, 1.0, None, 8, "vector")]
    assert frames["llf_in"].min() >= 0 and frames["llf_in"].max() <= 1.0 + 1e-6                       # gamma-encoded, not 16-bit
    assert out3.min() >= 0 and out3.max() <= 65535 and not np.array_equal(out3, out0)
    # the resident driver: the same five steps in the same order
    text = inspect.getsource(dv._deblur_device)
    at = [text.index(call) for call in ("deb.tv_denoise(", "deb.local_laplacian(", "deb.wavelet_equalize(", "deb.guided_filter(", "deb.usm(", "deb.gamma(1.0, 2.2")]
    assert at == sorted(at), at
    got = []
    monkeypatch.setattr(dv, "_deblur_device", lambda *a: got.append(a) or (None, None))                    # ... and the keyword reaches it
    dv.deblur_module(pic, "x", ".", 5, device_resident=True, denoise=(0.05, 10), clarity=[0.2, 1, 0.6], **kw)
    assert len(got) == 1 and got[0][-1] == (0.2, 1.0, 0.6, "vector") and got[0][-4] == (0.05, 10, "vector")
