"""GPU: the wavelet equaliser of device-resident H x W x 3 float32 images (csrc/ics_img_wavelet.hip, DeviceImage.wavelet_equalize,
lib.utils.wavelet_equalizer, deblur_module(local_contrast=...)) against the float64 oracle tests/wavelet_ref.py.

Gate against the oracle: 4 x the worst |float32 restatement - float64 oracle| of the parameter set over the test's own pictures,
measured on the CPU without the code under test (F32_RESTATEMENT_ERROR below; `python tests/test_gpu_wavelet.py` prints them).  The
factor 4 covers what the device may do differently from numpy's float32 (the order inside the vector magnitude, its square root and
division).  The operator is a chain of averages followed by a weighted sum, so the constants stay below 1e-6 even for eight scales
with gain 4; one above 1e-6 would mean that its input amplifies rounding, and the input would have to go, not the gate.

Shapes: 1 x 9, 9 x 1 and 5 x 7 fold every offset (several times from the third scale on); 33 x 1030 and 1030 x 33 are thinner than
the 14 px halo of the fused route; 301 x 287 has several 48 x 32 tiles both ways with ragged last ones; 64 x 96 sits exactly on two
tiles per axis and 65 x 97 one pixel past them; 700 x 513.  The per-scale route and the fused route must agree bit for bit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
import wavelet_ref as wr
from test_gpu_img_filters import picture

TILE_W, TILE_H = 48, 32                                 # the fused route's output tile (csrc/ics_img_wavelet.hip)
SIZES = [(1, 9), (9, 1), (5, 7), (33, 1030), (1030, 33), (301, 287), (2 * TILE_H, 2 * TILE_W), (2 * TILE_H + 1, 2 * TILE_W + 1), (700, 513)]
PARAMS = {"identity": ((1.0,) * 5, None),
          "lift": ((2.5, 2.0, 1.5, 1.2, 1.0), (0.0,) * 5),
          "denoise": ((0.0, 0.5, 1.0, 1.0, 1.0), (0.05, 0.02, 0.01, 0.0, 0.0)),
          "widest": ((4.0,) * 8, (0.01,) * 8)}
F = 3                                                   # lib._native.IMG_WAVELET_FUSED (checked below)
MIXED = ((2.5, 2.0, 1.5, 1.2, 1.0, 0.8, 1.1, 0.9), (0.05, 0.02, 0.01, 0.0, 0.0, 0.005, 0.0, 0.01), 0.9)    # gains, thresholds, residual


def wv_picture(H, W):
    return picture(H, W, seed=3000 + 3 * H + W)


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@functools.lru_cache(maxsize=None)
def oracle(H, W, name, coupling):
    """the float64 oracle of a parameter set on the test's picture, computed once and never written"""
    gains, thr = PARAMS[name]
    ref = wr.wavelet_equalize(wv_picture(H, W), gains, thr, 1.0, coupling)
    ref.setflags(write=False)
    return ref


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| per (coupling, parameter set) over the pictures of the test (CPU only)"""
    res = {}
    for coupling in wr.COUPLINGS:
        for name, (gains, thr) in PARAMS.items():
            res[coupling, name] = max(worst(wr.wavelet_equalize(wv_picture(H, W), gains, thr, 1.0, coupling, dtype=np.float32), oracle(H, W, name, coupling))
                                      for H, W in SIZES)
    return res


# Measured on the CPU by `python tests/test_gpu_wavelet.py`, without the code under test.
F32_RESTATEMENT_ERROR = {
    ("channel", "identity"): 1.490e-08, ("channel", "lift"): 2.790e-07, ("channel", "denoise"): 1.382e-07, ("channel", "widest"): 8.911e-07,
    ("vector", "identity"): 1.490e-08, ("vector", "lift"): 2.790e-07, ("vector", "denoise"): 1.445e-07, ("vector", "widest"): 7.038e-07}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
def test_matches_the_float64_oracle(ctx, coupling, name):
    from lib._native import DeviceImage
    gate = 4 * F32_RESTATEMENT_ERROR[coupling, name]
    assert 0 < gate <= 4e-6                              # see the module docstring
    gains, thr = PARAMS[name]
    for H, W in SIZES:
        pic = wv_picture(H, W)
        ref = oracle(H, W, name, coupling)
        img = DeviceImage.from_host(pic, ctx)
        for route in (0, 1, 2):
            out = img.wavelet_equalize(gains, thr, 1.0, coupling, route=route).to_host()
            err = worst(out, ref)
            print("wavelet %s %s %d x %d route %d: error %.3e, gate %.3e, ratio %.3f" % (coupling, name, H, W, route, err, gate, err / gate))
            assert out.dtype == np.float32 and out.shape == pic.shape
            assert err <= gate, (H, W, route, err, gate)
        assert np.array_equal(img.to_host(), pic)        # the source is never written


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
@pytest.mark.parametrize("H,W", SIZES)
def test_the_fused_route_is_bit_identical_to_the_per_scale_route(ctx, H, W, coupling):
    from lib import _native
    assert _native.IMG_WAVELET_FUSED == F and _native.IMG_WAVELET_MAX_SCALES == 8
    pic = wv_picture(H, W)
    img = _native.DeviceImage.from_host(pic, ctx)
    for J in (1, F - 1, F, F + 1, 8):
        gains, thr, residual = MIXED[0][:J], MIXED[1][:J], MIXED[2]
        a = img.wavelet_equalize(gains, thr, residual, coupling, route=1).to_host()
        b = img.wavelet_equalize(gains, thr, residual, coupling, route=2).to_host()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (J, worst(a, b))
        assert np.array_equal(img.wavelet_equalize(gains, thr, residual, coupling, route=0).to_host().view(np.uint32), a.view(np.uint32))
        for route, first in ((1, a), (2, b)):            # two runs, identical bits
            assert np.array_equal(img.wavelet_equalize(gains, thr, residual, coupling, route=route).to_host().view(np.uint32), first.view(np.uint32))
        assert np.array_equal(img.to_host(), pic)        # the source image is unchanged after every call


@pytest.mark.gpu
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("coupling", wr.COUPLINGS)
def test_exact_properties_on_the_device(ctx, coupling, route):
    from lib._native import DeviceImage
    # a constant with few significant bits: every product and sum of the passes is exact (tests/test_wavelet.py), so it is a fixed point
    const = np.full((37, 45, 3), np.float32(0.375), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    for gains, thr in (((2.5, -1.0, 0.0, 4.0, 1.0), (0.0, 0.01, 0.0, 0.0, 0.02)), ((1.0,) * 8, None), ((3.0,), None)):
        assert np.array_equal(DeviceImage.from_host(const, ctx).wavelet_equalize(gains, thr, 1.0, coupling, route=route).to_host(), const)
    pic = wv_picture(70, 53)
    img = DeviceImage.from_host(pic, ctx)
    J = 4
    gains, thr = MIXED[0][:J], MIXED[1][:J]
    out = img.wavelet_equalize(gains, thr, 1.0, coupling, route=route).to_host()
    assert not np.array_equal(out, pic)
    for order in ([2, 0, 1], [1, 0, 2]):                 # permuting the channels permutes the output
        perm = np.ascontiguousarray(pic[..., order])
        assert np.array_equal(DeviceImage.from_host(perm, ctx).wavelet_equalize(gains, thr, 1.0, coupling, route=route).to_host(), out[..., order])
    # one-hot gains with residual 0 return the detail scale; a threshold above its maximum removes the scale exactly
    for j in range(J):
        w = img.wavelet_equalize(np.eye(J)[j], None, 0.0, coupling, route=route).to_host()
        assert w.any()
        t = list(thr)
        t[j] = 2.0 * float(np.abs(w).max())              # > sqrt(3) max |w|: above the vector magnitude too
        without = [g if i != j else 0.0 for i, g in enumerate(gains)]
        a = img.wavelet_equalize(gains, t, 1.0, coupling, route=route).to_host()
        b = img.wavelet_equalize(without, thr, 1.0, coupling, route=route).to_host()
        assert np.array_equal(a, b), (j, worst(a, b))
    # gains 0: residual * c_J, whatever the thresholds
    a = img.wavelet_equalize([0.0] * J, [0.1] * J, 0.5, coupling, route=route).to_host()
    assert worst(a, 0.5 * wr.decompose(pic, J)[1]) <= 4 * 4 * 6 * 2.0 ** -24      # 6 roundings per scale of values <= 1
    assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
def test_utils_dispatch_errors_and_kernel_time(ctx):
    from lib import _native, utils
    pic = wv_picture(120, 131)
    img = _native.DeviceImage.from_host(pic, ctx)
    gains, thr = PARAMS["denoise"]
    res = utils.wavelet_equalizer(img, gains, thr, 0.9, "channel")
    assert isinstance(res, _native.DeviceImage) and res.shape == (120, 131, 3)
    assert ctx.last_kernel_ms() > 0.0                    # the queued filter's own kernel time
    dev = res.to_host()
    host = utils.wavelet_equalizer(pic.astype(np.float64), gains, thr, 0.9, "channel")                 # an array: one upload, one download
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host.view(np.uint32), dev.view(np.uint32))
    assert np.array_equal(utils.wavelet_equalizer(img, gains).to_host(), img.wavelet_equalize(gains, None, 1.0, "vector").to_host())   # the defaults
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.wavelet_equalizer(np.zeros((8, 9)), gains)
    with pytest.raises(ValueError, match="coupling"):
        img.wavelet_equalize(gains, coupling="colour")
    # bad arguments through the C entry: an error code, a text that names the argument, no image
    lib = _native.load()
    ok = np.ones(8, np.float32)
    nan, neg = ok.copy(), ok.copy()
    nan[1], neg[0] = np.nan, -1.0
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    for scales, g, t, residual, coupling, route, word in ((0, ok, None, 1.0, 1, 0, b"scales"), (9, ok, None, 1.0, 1, 0, b"scales"), (5, None, None, 1.0, 1, 0, b"gains"),
                                                          (5, nan, None, 1.0, 1, 0, b"gains[1]"), (5, ok, nan, 1.0, 1, 0, b"thresholds[1]"), (5, ok, neg, 1.0, 1, 0, b"thresholds[0]"),
                                                          (5, ok, None, float("inf"), 1, 0, b"residual"), (5, ok, None, 1.0, 2, 0, b"coupling"), (5, ok, None, 1.0, 0, 3, b"route")):
        out = C.c_void_p()
        assert lib.ics_img_wavelet_equalize(img._h, scales, ptr(g), ptr(t), residual, coupling, route, C.byref(out)) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error() and out.value is None, (word, lib.ics_last_error())
    assert np.array_equal(img.to_host(), pic)


# ---- deblur_module(local_contrast=...) ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deblur_module_local_contrast_on_the_resident_frame(capsys, monkeypatch):
    """The resident driver with local_contrast equals the resident driver without it followed by the operator on the gamma-encoded
    frame (taken from the plain call just before its final gamma step), the clip, the power 2.2 and the crop done in numpy.  Both
    apply the same device operator to the same bits; what differs is float32 powf, device against numpy, which is what
    tests/test_driver.py allows its two drivers: 2e-5 of the 16-bit range."""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib._native import DeviceImage
    case = orc.synth_case(99, 101, 5, seed=4)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=41, display=False, iterations=2, pyramid=False, save=False, device_resident=True)
    lc = ((1.0, 1.6, 1.8, 1.4, 1.0), (0.02, 0.01, 0.0, 0.0, 0.0), "channel")
    plain, _ = dv.deblur_module(pic, "a", ".", 5, **kw)
    none, _ = dv.deblur_module(pic, "a", ".", 5, local_contrast=None, **kw)
    assert np.array_equal(plain, none)                   # None: bit-equal to the call without the argument
    gamma, frames = DeviceImage.gamma, []

    def capturing_gamma(self, div, exponent, mul=1.0, clip01=False):
        if clip01:
            frames.append(self.to_host())
        return gamma(self, div, exponent, mul, clip01)
    monkeypatch.setattr(DeviceImage, "gamma", capturing_gamma)
    again, _ = dv.deblur_module(pic, "a", ".", 5, **kw)
    monkeypatch.setattr(DeviceImage, "gamma", gamma)
    assert len(frames) == 1 and np.array_equal(again, plain)
    eq = DeviceImage.from_host(frames[0]).wavelet_equalize(*lc[:2], 1.0, lc[2]).to_host()
    expect = (np.clip(eq, 0., 1.) ** 2.2 * (2 ** 16 - 1))[1:-1, 1:-1]     # 99 + 2 and 101 + 2 are odd: no further padding to undo
    count = {"up": 0, "down": 0}
    order = []
    from_host, to_host, wavelet = DeviceImage.from_host.__func__, DeviceImage.to_host, DeviceImage.wavelet_equalize
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    monkeypatch.setattr(DeviceImage, "wavelet_equalize", lambda self, *a, **k: (order.append(a), wavelet(self, *a, **k))[1])
    out, _ = dv.deblur_module(pic, "a", ".", 5, local_contrast=lc, **kw)
    assert count == {"up": 1, "down": 1}, count          # the frame still crosses PCIe exactly twice
    assert order == [(lc[0], lc[1], 1.0, "channel")], order
    assert out.shape == plain.shape == expect.shape and out.min() >= 0 and out.max() <= 65535 and not np.array_equal(out, plain)
    diff = float(np.abs(out.astype(np.float64) - expect).max()) / 65535
    print("deblur_module(local_contrast): resident vs plain + operator %.3e of the 16-bit range, gate 2e-5, ratio %.3f" % (diff, diff / 2e-5))
    assert diff <= 2e-5, diff


if __name__ == "__main__":
    for prm, err in measure_f32_restatement().items():
        print(prm, "%.3e" % err)
