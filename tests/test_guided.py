"""CPU: the oracle of the guided filter (tests/guided_ref.py: box means, a closed-form solve per window, the averaged fits applied to
the picture) checked against an independent statement of the same filter, and the surface of ics_img_guided /
DeviceImage.guided_filter / lib.utils.guided_filter / deblur_module(detail=...) as far as it can be checked without a GPU.

The independent statement: for every pixel k the filter fits q = a . I + b over k's clipped window w by ridge least squares,
min sum_w (a . I_p + b - I_p,c)^2 + eps |w| |a|^2 for each output channel c, and a pixel's output is the average of the fits of all
windows that contain it, applied to the pixel.  numpy.linalg.lstsq solves each fit on the uncentred picture; the oracle's moments,
cofactor inverse and centring must agree with it to 1e-12 in float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guided_ref as gr
from test_gpu_img_filters import picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ics_hip.h")


def gf_picture(H, W):
    return picture(H, W, seed=5000 + 3 * H + W)


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def fitted(I, r, eps, coupling):
    """the filter by per-window ridge least squares (see the module docstring), float64"""
    I = np.asarray(I, np.float64)
    H, W, _ = I.shape
    a = np.zeros((H, W, 3, 3))
    b = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            w = I[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].reshape(-1, 3)
            n = len(w)
            for c in range(3):
                cols = [c] if coupling == "channel" else [0, 1, 2]
                X = np.zeros((n + len(cols), len(cols) + 1))
                X[:n, :-1], X[:n, -1] = w[:, cols], 1.0
                X[n:, :-1] = np.sqrt(eps * n) * np.eye(len(cols))
                sol = np.linalg.lstsq(X, np.concatenate([w[:, c], np.zeros(len(cols))]), rcond=None)[0]
                a[y, x, c, cols], b[y, x, c] = sol[:-1], sol[-1]
    q = np.zeros_like(I)
    for y in range(H):
        for x in range(W):
            ys, xs = slice(max(y - r, 0), y + r + 1), slice(max(x - r, 0), x + r + 1)
            q[y, x] = a[ys, xs].mean(axis=(0, 1)) @ I[y, x] + b[ys, xs].mean(axis=(0, 1))
    return q


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", gr.COUPLINGS)
def test_the_oracle_is_the_average_of_the_ridge_fits_of_every_window(coupling):
    pic = gf_picture(9, 11)
    eps = float(np.float32(1e-2))
    for r in (1, 2, 6):                                  # 6: every window is clipped, most to the whole picture
        ref = gr.guided_filter(pic, r, eps, 0.0, coupling)
        err = worst(ref, fitted(pic, r, eps, coupling))
        print("guided_ref %s r %d against the ridge fits: %.3e" % (coupling, r, err))
        assert ref.dtype == np.float64 and ref.shape == pic.shape and err <= 1e-12, (r, err)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", gr.COUPLINGS)
def test_a_constant_picture_is_a_fixed_point(coupling, dtype):
    """0.375 x [1, 0.5, 2] - 0.5 has at most 3 significant bits: every box sum of it and of its products is exact (n x a few bits,
    n <= 65^2), so is the division by n, and every variance and covariance is exactly 0.  "channel": a = 0 / (0 + eps) = 0, b = mu,
    q = (0 + mu) + 0.5 = I for any eps.  "vector": M = eps E, A_ii = 1 - eps (eps^2 / (eps eps^2)); with eps a power of two these
    products and quotients are exact and A = 0 (another eps may leave an A_ii of one ulp of 1, which is then not a few-bit number)."""
    const = np.full((11, 13, 3), 0.375, np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    for r in (1, 4, 32):
        for eps in (2.0 ** -7, 2.0 ** -13) + ((1e-2, 1e-4) if coupling == "channel" else ()):
            for detail in (0.0, 1.5, -2.0):
                out = gr.guided_filter(const, r, eps, detail, coupling, dtype=dtype)
                assert out.dtype == dtype and np.array_equal(out, const.astype(dtype)), (r, eps, detail)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", gr.COUPLINGS)
def test_a_huge_eps_gives_the_box_mean_of_the_box_mean(coupling, dtype):
    """eps = 1e6 against variances <= 1/4: |a| <= 2.5e-7, so q = mean(mean(I)) up to 2.5e-7 x (|I'| + |mu|) <= 2.5e-7 a channel (three
    in "vector") and the float32 roundings of the two means"""
    for H, W, r in ((33, 40, 4), (5, 7, 3), (65, 97, 16)):
        pic = gf_picture(H, W)
        q = gr.guided_filter(pic, r, 1e6, 0.0, coupling, dtype=dtype)
        mm = gr.box_mean(gr.box_mean(pic.astype(np.float64), r), r)
        assert worst(q, mm) <= 1e-5, (H, W, r, worst(q, mm))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", gr.COUPLINGS)
def test_detail_one_returns_the_picture_and_detail_zero_the_base_layer(coupling, dtype):
    pic = gf_picture(33, 40)
    ulp = np.spacing(np.ones((), dtype))                 # of values in [1, 2): an upper bound for every value of the test
    q = gr.base_layer(pic, 4, 1e-3, coupling, dtype=dtype)
    assert np.array_equal(gr.guided_filter(pic, 4, 1e-3, 0.0, coupling, dtype=dtype), q)     # q itself, no blend
    assert worst(q, pic) > 1e-2
    assert worst(gr.guided_filter(pic, 4, 1e-3, 1.0, coupling, dtype=dtype), pic) <= ulp     # q + (I - q)
    lifted = gr.guided_filter(pic, 4, 1e-3, 1.5, coupling)
    assert worst(lifted - pic, 0.5 * (pic - gr.base_layer(pic, 4, 1e-3, coupling))) <= 1e-15


def test_channel_coupling_keeps_the_channels_apart_and_vector_coupling_does_not():
    pic = gf_picture(33, 40)
    other = pic.copy()
    other[..., 1] = pic[::-1, ::-1, 1]
    a, b = gr.guided_filter(pic, 3, 1e-3, 0.0, "channel"), gr.guided_filter(other, 3, 1e-3, 0.0, "channel")
    assert np.array_equal(a[..., 0], b[..., 0]) and np.array_equal(a[..., 2], b[..., 2]) and not np.array_equal(a[..., 1], b[..., 1])
    a, b = gr.guided_filter(pic, 3, 1e-3, 0.0, "vector"), gr.guided_filter(other, 3, 1e-3, 0.0, "vector")
    assert not np.array_equal(a[..., 0], b[..., 0]) and not np.array_equal(a[..., 2], b[..., 2])
    out = gr.guided_filter(pic, 3, 1e-3, 1.5, "channel", dtype=np.float32)
    for order in ([2, 0, 1], [1, 0, 2]):                 # per channel: a permutation of the channels permutes the output exactly
        assert np.array_equal(gr.guided_filter(np.ascontiguousarray(pic[..., order]), 3, 1e-3, 1.5, "channel", dtype=np.float32), out[..., order])


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_function_and_the_constants():
    from lib import _native
    raw = open(HEADER).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    assert "int ics_img_guided(const ics_img *src, int radius, float eps, float detail, int coupling, int route, ics_img **out);" in text
    assert "#define ICS_ABI_VERSION 4 " in text
    kh = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")).read()
    for src in (raw, kh):
        assert int(re.search(r"#define ICS_IMG_GUIDED_MAX_RADIUS (\d+)", src).group(1)) == _native.IMG_GUIDED_MAX_RADIUS == gr.MAX_RADIUS == 32
        assert int(re.search(r"#define ICS_IMG_GUIDED_FUSED_RADIUS (\d+)", src).group(1)) == _native.IMG_GUIDED_FUSED_RADIUS
    assert 1 <= _native.IMG_GUIDED_FUSED_RADIUS < _native.IMG_GUIDED_MAX_RADIUS


def test_native_binds_it_and_refuses_bad_arguments_before_any_device_work():
    from lib import _native
    lib = _native.load()
    vp, ci, cf, pvp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)
    assert lib.ics_img_guided.argtypes == [vp, ci, cf, cf, ci, ci, pvp] and lib.ics_img_guided.restype is ci
    out = C.c_void_p()
    fake = C.c_void_p(8)    # never dereferenced: the arguments are checked first
    assert lib.ics_img_guided(None, 4, 1e-3, 0.0, 1, 0, C.byref(out)) == _native.ICS_EINVAL and b"NULL" in lib.ics_last_error()
    assert lib.ics_img_guided(fake, 4, 1e-3, 0.0, 1, 0, None) == _native.ICS_EINVAL
    F = _native.IMG_GUIDED_FUSED_RADIUS
    for radius, eps, detail, coupling, route, word in (
            (0, 1e-3, 0.0, 1, 0, b"radius"), (33, 1e-3, 0.0, 1, 0, b"radius"), (-4, 1e-3, 0.0, 1, 0, b"radius"),
            (4, 0.0, 0.0, 1, 0, b"eps"), (4, -1e-3, 0.0, 1, 0, b"eps"), (4, float("nan"), 0.0, 1, 0, b"eps"), (4, float("inf"), 0.0, 1, 0, b"eps"),
            (4, 1e-3, float("nan"), 1, 0, b"detail"), (4, 1e-3, float("-inf"), 0, 0, b"detail"),
            (4, 1e-3, 0.0, 2, 0, b"coupling"), (4, 1e-3, 0.0, -1, 0, b"coupling"), (4, 1e-3, 0.0, 1, 3, b"route"), (4, 1e-3, 0.0, 1, -1, b"route"),
            (F + 1, 1e-3, 0.0, 1, 2, b"route"), (32, 1e-3, 0.0, 0, 2, b"route")):
        out = C.c_void_p(1)
        assert lib.ics_img_guided(fake, radius, eps, detail, coupling, route, C.byref(out)) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error() and out.value is None, (word, lib.ics_last_error(), out.value)


BAD_ARGUMENTS = [
    (dict(radius=0), "radius"), (dict(radius=33), "radius"), (dict(radius=2.5), "radius"), (dict(radius=float("nan")), "radius"), (dict(radius="4"), "radius"),
    (dict(radius=None), "radius"), (dict(radius=True), "radius"),
    (dict(eps=0.0), "eps"), (dict(eps=-1e-3), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=1e-60), "eps"),
    (dict(eps=None), "eps"),
    (dict(detail=float("nan")), "detail"), (dict(detail=float("inf")), "detail"), (dict(detail=1e39), "detail"), (dict(detail="much"), "detail"),
    (dict(coupling="colour"), "coupling"), (dict(coupling=1), "coupling"),
    (dict(route=3), "route"), (dict(route=-1), "route"), (dict(route=2, radius=9), "route")]


def test_guided_args_device_image_and_utils_raise_value_errors_before_any_native_call(monkeypatch):
    from lib import _native, utils
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("a native call"))
    img = _native.DeviceImage(None, None)                                # no handle: nothing to destroy
    for kw, word in BAD_ARGUMENTS:
        full = dict(dict(radius=4, eps=1e-3), **kw)
        with pytest.raises(ValueError, match=word):
            _native.guided_args(**full)
        with pytest.raises(ValueError, match=word):
            img.guided_filter(**full)
        if "route" not in kw:
            with pytest.raises(ValueError, match=word):
                utils.guided_filter(np.zeros((8, 9, 3), np.float32), **full)
    for bad in (np.zeros((8, 9)), np.zeros((8, 9, 4)), np.zeros((3, 8, 9, 3)), np.zeros(7)):
        with pytest.raises(ValueError, match="H x W x 3"):
            utils.guided_filter(bad, 4, 1e-3)
    assert _native.guided_args(4, 1e-3) == (4, 1e-3, 0.0, "vector", 0)
    assert _native.guided_args(np.int64(8), np.float32(0.25), 2, "channel", 2) == (8, 0.25, 2.0, "channel", 2)
    assert _native.guided_args(32.0, 1, -1.5, "vector", 1) == (32, 1.0, -1.5, "vector", 1)


# ---- deblur_module(detail=...) ----------------------------------------------------------------------------------------------------
def test_deblur_module_validates_detail_before_it_touches_a_device(monkeypatch):
    import deconvolve as dv
    from lib import _native
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("a native call"))
    pic = np.full((64, 64, 3), 128, np.uint8)
    for bad, word in (((), "detail"), (1.5, "detail"), ((8, 1e-3), "detail"), ((8, 1e-3, 1.5, "vector", 1), "detail"), ((0, 1e-3, 1.5), "radius"),
                      ((33, 1e-3, 1.5), "radius"), ((2.5, 1e-3, 1.5), "radius"), ((8, 0.0, 1.5), "eps"), ((8, float("nan"), 1.5), "eps"),
                      ((8, float("inf"), 1.5), "eps"), ((8, 1e-3, float("nan")), "detail"), ((8, 1e-3, 1.5, "colour"), "coupling")):
        for resident in (None, False, True):
            with pytest.raises(ValueError, match="detail") as info:
                dv.deblur_module(pic, "x", ".", 5, save=False, display=False, device_resident=resident, detail=bad)
            assert word in str(info.value)
        with pytest.raises(ValueError, match=word):
            dv._detail_args(bad)
    assert dv._detail_args(None) is None
    assert dv._detail_args((8, 1e-3, 1.5)) == (8, 1e-3, 1.5, "vector")
    assert dv._detail_args([16, 0.01, 0.5, "channel"]) == (16, 0.01, 0.5, "channel")


def _recording_solver(calls):
    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd, **kw):
        calls.append((image.copy(), u.copy(), psf.copy(), (top, bottom, left, right, tau, M, N, C_, MK, iterations, step, lambd), kw))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]
    return solver


def test_deblur_module_host_driver_applies_detail_after_local_contrast_and_before_the_mask(monkeypatch, capsys):
    """detail=None never calls utils.guided_filter and changes nothing; with all four arguments the host driver hands the deblurred
    gamma-encoded frame to tv_denoise, its result to wavelet_equalizer, that to guided_filter and that to USM, then clips (stand-ins
    record the order and answer with the oracles: no GPU here)"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    import tv_denoise_ref as tvr
    import utils_oracle as uo
    import wavelet_ref as wr
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)
    seen, frames = [], {}

    def tv(src, weight=0.1, iterations=50, coupling="vector"):
        seen.append(("tv", src.shape, src.dtype, weight, iterations, coupling))
        return tvr.tv_denoise(src, weight, iterations, coupling, dtype=np.float32)

    def wavelet(src, gains, thresholds=None, residual=1.0, coupling="vector"):
        seen.append(("wavelet", src.shape, src.dtype, tuple(gains), thresholds, residual, coupling))
        frames["wavelet"] = wr.wavelet_equalize(src, gains, thresholds, residual, coupling, dtype=np.float32)
        return frames["wavelet"]

    def guided(src, radius, eps, detail=0.0, coupling="vector"):
        seen.append(("guided", src.shape, src.dtype, radius, eps, detail, coupling))
        frames["guided_in"] = src.copy()
        frames["guided"] = gr.guided_filter(src, radius, eps, detail, coupling, dtype=np.float32)
        return frames["guided"]

    def usm(src, radius, strength, amount, method="bessel"):
        seen.append(("usm", src.shape))
        frames.setdefault("usm_in", []).append(np.array(src))
        return uo.USM(np.asarray(src, np.float64), radius, strength, amount, method)
    monkeypatch.setattr(dv.utils, "tv_denoise", tv)
    monkeypatch.setattr(dv.utils, "wavelet_equalizer", wavelet)
    monkeypatch.setattr(dv.utils, "guided_filter", guided)
    monkeypatch.setattr(dv.utils, "USM", usm)
    pic = (np.random.default_rng(0).random((90, 100, 3)) * 255).astype(np.uint8)
    kw = dict(mask=[46, 50], mask_size=41, display=False, pyramid=False, save=False, iterations=7)
    base, none, full = [], [], []
    out0, psf0 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(base), **kw)
    out1, psf1 = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(none), detail=None, **kw)
    assert seen == [] and out0.dtype == out1.dtype and np.array_equal(out0, out1) and np.array_equal(psf0, psf1)
    assert len(base) == len(none) == 2                                    # detail=None: the solver is called exactly as without the keyword
    for x, y in zip(base, none):
        assert x[3] == y[3] and x[4] == y[4] and all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))
    gains = (1.0, 1.6, 1.8)
    out2, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver(full), denoise=(0.05, 10), sharpen=(9, 4., 0.5),
                               local_contrast=(gains,), detail=(8, 1e-3, 1.5, "channel"), **kw)
    assert seen == [("tv", (93, 103, 3), np.float32, 0.05, 10, "vector"), ("wavelet", (93, 103, 3), np.float32, gains, None, 1.0, "vector"),
                    ("guided", (93, 103, 3), np.float32, 8, 1e-3, 1.5, "channel")] + [("usm", (93, 103))] * 3
    assert np.array_equal(frames["guided_in"], frames["wavelet"])         # the equalised frame goes in ...
    assert all(np.array_equal(frames["usm_in"][c], frames["guided"][..., c]) for c in range(3))      # ... and its result on to the mask
    assert len(full) == 2
    for x, y in zip(base, full):                                          # the solver sees nothing of it
        assert x[3] == y[3] and x[4] == y[4] and all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))
    assert out2.shape == out0.shape and out2.min() >= 0 and out2.max() <= 65535 and not np.array_equal(out0, out2)
    # alone, with gain 1: the gamma-encoded frame comes back within an ulp, then the clip and the power
    seen.clear()
    out3, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), detail=(4, 1e-2, 1.0), **kw)
    assert seen == [("guided", (93, 103, 3), np.float32, 4, 1e-2, 1.0, "vector")]
    assert frames["guided_in"].min() >= 0 and frames["guided_in"].max() <= 1.0 + 1e-6                   # gamma-encoded, not 16-bit
    assert float(np.abs(out3.astype(np.float64) - out0).max()) / 65535 <= (2.2 * 2 + 4) * 2.0 ** -24     # d(x^2.2) <= 2.2 dx on [0, 1]; + the float32 roundings of the two power steps
    seen.clear()
    out4, _ = dv.deblur_module(pic, "x", ".", 5, solver=_recording_solver([]), detail=[4, 1e-2, 3.0], **kw)
    assert seen == [("guided", (93, 103, 3), np.float32, 4, 1e-2, 3.0, "vector")]
    assert out4.min() >= 0 and out4.max() <= 65535 and not np.array_equal(out4, out0)                    # lifted, and clipped afterwards
