"""GPU: TV denoising of device-resident H x W x 3 float32 images (csrc/ics_img_tvdenoise.hip, DeviceImage.tv_denoise,
lib.utils.tv_denoise, deblur_module(denoise=...)) against the float64 oracle tests/tv_denoise_ref.py.

Gate against the oracle: 4 x the worst |float32 restatement - float64 oracle| of the parameter set over the test's own pictures,
measured on the CPU without the code under test (F32_RESTATEMENT_ERROR below; `python tests/test_gpu_tv_denoise.py` prints them).
The factor 4 covers what the device may do differently from numpy's float32: the order of the four terms of div and of the three
terms of the vector sum.  With tau = 1/8 the iteration does not amplify rounding errors, so the constants stay near 1e-7 for 20 as
for 200 iterations; one above 1e-6 would mean that its input amplifies rounding, and the input would have to go, not the gate.

The per-iteration route and the blocked route (IMG_TV_BLOCK iterations per launch on LDS tiles) must agree bit for bit."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
import tv_denoise_ref as tvr
from test_gpu_img_filters import picture, uo, usm_bound

SIZES = [(301, 287), (33, 1030), (1030, 33), (5, 7), (1, 9), (9, 1)]
PARAMS = [(0.02, 20), (0.1, 50), (0.5, 100), (0.1, 200)]
LARGE = (2048, 2048, "vector", 0.1, 50)
T = 4                                                   # lib._native.IMG_TV_BLOCK (checked below)


def tv_picture(H, W):
    return picture(H, W, seed=2000 + 3 * H + W)


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| per (coupling, weight, iterations) over the pictures of the test (CPU only)"""
    res = {}
    for coupling in tvr.COUPLINGS:
        for weight, iterations in PARAMS:
            res[coupling, weight, iterations] = max(
                worst(tvr.tv_denoise(p, weight, iterations, coupling, dtype=np.float32), tvr.tv_denoise(p, weight, iterations, coupling))
                for p in (tv_picture(H, W) for H, W in SIZES))
    return res


def measure_f32_restatement_large():
    H, W, coupling, weight, iterations = LARGE
    p = tv_picture(H, W)
    return worst(tvr.tv_denoise(p, weight, iterations, coupling, dtype=np.float32), tvr.tv_denoise(p, weight, iterations, coupling))


# Measured on the CPU by `python tests/test_gpu_tv_denoise.py`, without the code under test.
F32_RESTATEMENT_ERROR = {
    ("channel", 0.02, 20): 5.420e-08, ("channel", 0.1, 50): 1.100e-07, ("channel", 0.5, 100): 1.060e-07, ("channel", 0.1, 200): 1.170e-07,
    ("vector", 0.02, 20): 4.959e-08, ("vector", 0.1, 50): 8.518e-08, ("vector", 0.5, 100): 1.090e-07, ("vector", 0.1, 200): 8.605e-08}
F32_RESTATEMENT_ERROR_LARGE = 1.004e-07


@pytest.mark.gpu
@pytest.mark.parametrize("weight,iterations", PARAMS)
@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
def test_matches_the_float64_oracle(ctx, coupling, weight, iterations):
    from lib._native import DeviceImage
    gate = 4 * F32_RESTATEMENT_ERROR[coupling, weight, iterations]
    assert gate <= 4e-6                                  # see the module docstring
    for H, W in SIZES:
        pic = tv_picture(H, W)
        ref = tvr.tv_denoise(pic, weight, iterations, coupling)
        img = DeviceImage.from_host(pic, ctx)
        for route in (0, 1, 2):
            out = img.tv_denoise(weight, iterations, coupling, route=route).to_host()
            err = worst(out, ref)
            print("tv_denoise %s weight=%g iterations=%d %d x %d route %d: error %.3e, gate %.3e, ratio %.3f"
                  % (coupling, weight, iterations, H, W, route, err, gate, err / gate))
            assert out.dtype == np.float32 and out.shape == pic.shape
            assert err <= gate, (H, W, route, err, gate)
        assert np.array_equal(img.to_host(), pic)        # the source is never written


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
@pytest.mark.parametrize("H,W", SIZES + [(700, 513)])
def test_the_blocked_route_is_bit_identical_to_the_per_iteration_route(ctx, H, W, coupling):
    from lib import _native
    assert _native.IMG_TV_BLOCK == T
    pic = tv_picture(H, W)
    img = _native.DeviceImage.from_host(pic, ctx)
    for iterations in (1, T - 1, T, T + 1, 3 * T + 2):
        a = img.tv_denoise(0.1, iterations, coupling, route=1).to_host()
        b = img.tv_denoise(0.1, iterations, coupling, route=2).to_host()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (iterations, worst(a, b))
        assert np.array_equal(img.tv_denoise(0.1, iterations, coupling, route=0).to_host().view(np.uint32), a.view(np.uint32))
        for route, first in ((1, a), (2, b)):            # two runs, identical bits
            assert np.array_equal(img.tv_denoise(0.1, iterations, coupling, route=route).to_host().view(np.uint32), first.view(np.uint32))
    assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("coupling", tvr.COUPLINGS)
def test_exact_properties_on_the_device(ctx, coupling, route):
    from lib._native import DeviceImage
    const = np.full((37, 45, 3), np.float32(0.37), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    for iterations in (1, 7, 50):
        assert np.array_equal(DeviceImage.from_host(const, ctx).tv_denoise(0.1, iterations, coupling, route=route).to_host(), const)
    pic = tv_picture(70, 53)
    img = DeviceImage.from_host(pic, ctx)
    zero = img.tv_denoise(0.1, 0, coupling, route=route)
    assert zero._h.value != img._h.value and np.array_equal(zero.to_host().view(np.uint32), pic.view(np.uint32))      # a copy, bit for bit
    out = img.tv_denoise(0.1, 30, coupling, route=route).to_host()
    assert not np.array_equal(out, pic)
    for order in ([2, 0, 1], [1, 0, 2]):                 # permuting the channels permutes the output
        perm = np.ascontiguousarray(pic[..., order])
        assert np.array_equal(DeviceImage.from_host(perm, ctx).tv_denoise(0.1, 30, coupling, route=route).to_host(), out[..., order])
    same = np.ascontiguousarray(np.repeat(pic[..., :1], 3, axis=2))                                                   # three equal planes stay equal
    o = DeviceImage.from_host(same, ctx).tv_denoise(0.1, 30, coupling, route=route).to_host()
    assert np.array_equal(o[..., 0], o[..., 1]) and np.array_equal(o[..., 0], o[..., 2])
    if coupling == "channel":                            # and a channel does not see the others
        assert np.array_equal(o[..., 0], out[..., 0])
    # div q of the stored q sums to zero exactly, so a channel mean moves by no more than the rounding of one output value: the three
    # additions of div and the one of f + div, each <= 2^-25 of a value <= 2
    for c in range(3):
        assert abs(float(out[..., c].astype(np.float64).mean()) - float(pic[..., c].astype(np.float64).mean())) <= 8 * 2.0 ** -24


@pytest.mark.gpu
def test_one_large_picture_matches_the_float32_restatement(ctx):
    """2048^2, vector, 50 iterations.  The device is allowed 4 E from the oracle and numpy's float32 is E from it (E =
    F32_RESTATEMENT_ERROR_LARGE, measured on this picture on the CPU), so the two are within 5 E of each other."""
    from lib._native import DeviceImage
    H, W, coupling, weight, iterations = LARGE
    pic = tv_picture(H, W)
    ref = tvr.tv_denoise(pic, weight, iterations, coupling, dtype=np.float32)
    gate = 5 * F32_RESTATEMENT_ERROR_LARGE
    assert gate <= 5e-6
    img = DeviceImage.from_host(pic, ctx)
    outs = [img.tv_denoise(weight, iterations, coupling, route=route).to_host() for route in (1, 2, 0)]
    err = worst(outs[0], ref)
    print("tv_denoise %s weight=%g iterations=%d %d x %d against numpy float32: error %.3e, gate %.3e, ratio %.3f" % (coupling, weight, iterations, H, W, err, gate, err / gate))
    assert err <= gate
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)) and np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
def test_utils_dispatch_errors_and_kernel_time(ctx):
    from lib import _native, utils
    pic = tv_picture(120, 131)
    img = _native.DeviceImage.from_host(pic, ctx)
    res = utils.tv_denoise(img, 0.1, 20, "channel")
    assert isinstance(res, _native.DeviceImage) and res.shape == (120, 131, 3)
    assert ctx.last_kernel_ms() > 0.0                    # the queued filter's own kernel time
    dev = res.to_host()
    host = utils.tv_denoise(pic.astype(np.float64), 0.1, 20, "channel")                                # an array: one upload, one download
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host, dev)
    assert np.array_equal(utils.tv_denoise(img).to_host(), img.tv_denoise(0.1, 50, "vector").to_host())  # the defaults
    for bad in (np.zeros((8, 9)), np.zeros((8, 9, 4))):
        with pytest.raises(ValueError, match="H x W x 3"):
            utils.tv_denoise(bad)
    with pytest.raises(ValueError, match="coupling"):
        img.tv_denoise(0.1, 5, "colour")
    for kw in (dict(weight=0.0), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(iterations=-1), dict(route=3), dict(route=-1)):
        with pytest.raises(_native.NativeError) as ei:
            img.tv_denoise(**kw)
        assert ei.value.code == _native.ICS_EINVAL, kw
    assert np.array_equal(img.to_host(), pic)


# ---- deblur_module(denoise=...) ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pyramid", [False, True])
def test_deblur_module_denoise(pyramid, capsys, monkeypatch):
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib import utils
    from lib._native import DeviceImage
    case = orc.synth_case(301, 287, 5, seed=4)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=101, display=False, iterations=2, pyramid=pyramid, save=False)
    plain = {}
    for resident in (False, True):       # denoise=None: bit-equal to the call without the argument, in both drivers
        a, pa = dv.deblur_module(pic, "a", ".", 5, device_resident=resident, **kw)
        b, pb = dv.deblur_module(pic, "b", ".", 5, device_resident=resident, denoise=None, **kw)
        assert a.dtype == b.dtype and np.array_equal(a, b) and np.array_equal(pa, pb)
        plain[resident] = a
    denoise = (0.05, 20)
    out_h, _ = dv.deblur_module(pic, "h", ".", 5, device_resident=False, denoise=denoise, **kw)
    count = {"up": 0, "down": 0}
    order = []
    from_host, to_host, tv, usm = DeviceImage.from_host.__func__, DeviceImage.to_host, DeviceImage.tv_denoise, DeviceImage.usm

    def counting_from_host(cls, *a, **k):
        count["up"] += 1
        return from_host(cls, *a, **k)

    def counting_to_host(self):
        count["down"] += 1
        return to_host(self)

    def recording_tv(self, *a, **k):
        order.append(("tv",) + a)
        return tv(self, *a, **k)

    def recording_usm(self, *a, **k):
        order.append(("usm",) + a)
        return usm(self, *a, **k)
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(counting_from_host))
    monkeypatch.setattr(DeviceImage, "to_host", counting_to_host)
    monkeypatch.setattr(DeviceImage, "tv_denoise", recording_tv)
    monkeypatch.setattr(DeviceImage, "usm", recording_usm)
    out_d, _ = dv.deblur_module(pic, "d", ".", 5, device_resident=True, denoise=denoise, **kw)
    assert count == {"up": 1, "down": 1}, count                 # the frame still crosses PCIe exactly twice
    assert order == [("tv", 0.05, 20, "vector")], order
    assert out_d.shape == out_h.shape == (301, 287, 3)
    assert out_d.min() >= 0 and out_d.max() <= 65535 and out_h.min() >= 0 and out_h.max() <= 65535
    assert not np.array_equal(out_d, plain[True]) and not np.array_equal(out_h, plain[False])
    diff = float(np.abs(out_d.astype(np.float64) - out_h).max()) / 65535
    print("deblur_module(denoise) pyramid=%s: resident vs host %.3e of the 16-bit range, gate 2e-5, ratio %.3f" % (pyramid, diff, diff / 2e-5))
    assert diff <= 2e-5, diff                                   # what the two drivers are allowed (tests/test_driver.py)
    # denoise and sharpen together: first the denoiser, then the mask, on the resident frame ...
    del order[:]
    both_d, _ = dv.deblur_module(pic, "d", ".", 5, device_resident=True, denoise=(0.05, 20, "channel"), sharpen=(9, 4., 0.5), **kw)
    assert order == [("tv", 0.05, 20, "channel"), ("usm", 9, 4., 0.5, "bessel")], order
    assert not np.array_equal(both_d, out_d)
    # ... and on the host driver (utils.tv_denoise on the frame, then utils.USM per channel)
    host_order = []
    utv, uusm = utils.tv_denoise, utils.USM
    monkeypatch.setattr(dv.utils, "tv_denoise", lambda *a, **k: (host_order.append("tv"), utv(*a, **k))[1])
    monkeypatch.setattr(dv.utils, "USM", lambda *a, **k: (host_order.append("usm"), uusm(*a, **k))[1])
    both_h, _ = dv.deblur_module(pic, "h", ".", 5, device_resident=False, denoise=(0.05, 20, "channel"), sharpen=(9, 4., 0.5), **kw)
    assert host_order == ["tv", "usm", "usm", "usm"], host_order
    diff = float(np.abs(both_d.astype(np.float64) - both_h).max()) / 65535
    gate = (1 + 2 * 0.5) * 2e-5 + usm_bound(uo.kaiser_kernel(9, 4.), 0.5, 1.0)     # as tests/test_gpu_img_filters.py::test_deblur_module_sharpen
    print("deblur_module(denoise, sharpen) pyramid=%s: resident vs host %.3e of the 16-bit range, gate %.3e, ratio %.3f" % (pyramid, diff, gate, diff / gate))
    assert diff <= gate, (diff, gate)


if __name__ == "__main__":
    for prm, err in measure_f32_restatement().items():
        print(prm, "%.3e" % err)
    print("large", LARGE, "%.3e" % measure_f32_restatement_large())
