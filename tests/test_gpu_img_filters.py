"""GPU: the lib.utils filters on device-resident H x W x 3 float32 images (csrc/ics_img_filters.hip) against the float64 oracle
(oracle/utils_oracle.py, pinned to the reference's own outputs by tests/test_utils.py::test_oracle_matches_reference_outputs),
each channel on its own.

Gates of the blurs and of USM are derived, not tuned.  The window kernels are non-negative and sum to 1; each pass is an FMA chain
of n terms on float32-rounded weights with a float32 intermediate, so a blur is within (KH + KW + 4) * 2^-24 * max|src| of the float64
result, USM within (1 + 2 |amount|) times that plus 4 * 2^-24 * (1 + 2 |amount|) * max|src|; a kernel that is not an outer product
runs as one chain of KH * KW terms: (KH * KW + 2) * 2^-24 * sum|w| * max|src|.

Measured on an MI355X, worst error / bound over the cases of each test (every test prints its own): blurs 0.161 (uniform 4 x 4 at
33 x 1030), the 5 x 5 kernel that is no outer product 0.076, USM 0.055, utils.USM(DeviceImage) against three float64 calls at 1024^2
0.042, bilateral 0.261 of its gate (radius 10 at 301 x 287), deblur_module(sharpen) resident against host 0.009."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import utils_oracle as uo

EPS = 2.0 ** -24
SIZES = [(301, 287), (33, 1030), (1030, 33), (5, 7)]


def picture(H, W, seed):
    """a seeded picture in [0, 1]: noise on a smooth ramp, so that both the flat and the busy case of a filter occur"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.25 * np.sin(x / 17.0)[..., None] * np.cos(y / 23.0)[..., None] * np.array([1.0, 0.8, 0.6])
    return np.clip(base + 0.25 * (rng.random((H, W, 3)) - 0.5) + 0.3 * (rng.random((H, W, 3)) > 0.97), 0, 1).astype(np.float32)


def window_kernels():
    return {"gaussian15": uo.gaussian_kernel(15, 2.5), "kaiser9": uo.kaiser_kernel(9, 4.), "poisson7": uo.poisson_kernel(7, 2.),
            "uniform4": uo.uniform_kernel(4)}


def random_kernel():
    k = np.random.default_rng(55).random((5, 5)) - 0.3      # not an outer product, mixed signs
    return k / np.abs(k).sum()


def blur_bound(kern, smax):
    return (kern.shape[0] + kern.shape[1] + 4) * EPS * smax


def usm_bound(kern, amount, smax):
    return (1 + 2 * abs(amount)) * blur_bound(kern, smax) + 4 * EPS * (1 + 2 * abs(amount)) * smax


def worst(dev, ref):
    return float(np.max(np.abs(dev.astype(np.float64) - ref)))


def per_channel(f, pic):
    return np.dstack([f(pic[..., c].astype(np.float64)) for c in range(3)])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES + [(2048, 2048)])
def test_blurs_match_the_float64_oracle_within_the_derived_bound(ctx, H, W):
    from lib._native import DeviceImage
    pic = picture(H, W, seed=H * 7 + W)
    smax = float(np.abs(pic).max())
    img = DeviceImage.from_host(pic, ctx)
    kernels = window_kernels()
    if (H, W) == (2048, 2048):
        kernels = {"gaussian15": kernels["gaussian15"]}            # (scipy's convolve2d needs seconds per channel at this size)
    ratios = {}
    for name, kern in kernels.items():
        out = img.convolve(kern).to_host()
        ratios[name] = worst(out, per_channel(lambda ch: uo.conv2d_symm(ch, kern), pic)) / blur_bound(kern, smax)
    kr = random_kernel()
    out = img.convolve(kr).to_host()
    ratios["random5x5"] = worst(out, per_channel(lambda ch: uo.conv2d_symm(ch, kr), pic)) / ((kr.size + 2) * EPS * np.abs(kr).sum() * smax)
    assert np.array_equal(img.to_host(), pic)                       # the source is left untouched
    print("blur %d x %d: error / bound %s" % (H, W, {k: round(v, 3) for k, v in ratios.items()}))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES + [(2048, 2048)])
def test_usm_and_named_blurs_match_the_float64_oracle(ctx, H, W):
    from lib._native import DeviceImage
    pic = picture(H, W, seed=H * 11 + W)
    smax = float(np.abs(pic).max())
    img = DeviceImage.from_host(pic, ctx)
    ratios = {}
    cases = [(15, 2.5, 0.8, "gauss"), (9, 4., 0.5, "bessel"), (9, 4., -0.4, "bessel"), (4, 1.0, 1.5, "gauss")]
    if (H, W) == (2048, 2048):
        cases = cases[:1]
    for radius, strength, amount, method in cases:
        kern = {"gauss": uo.gaussian_kernel, "bessel": uo.kaiser_kernel}[method](radius, strength)
        out = img.usm(radius, strength, amount, method).to_host()
        ref = per_channel(lambda ch: uo.USM(ch, radius, strength, amount, method), pic)
        ratios["usm", radius, amount, method] = worst(out, ref) / usm_bound(kern, amount, smax)
    if (H, W) != (2048, 2048):
        out = img.gaussian_blur(15, 2.5).to_host()
        ratios["gaussian_blur"] = worst(out, per_channel(lambda ch: uo.gaussian_blur(ch, 15, 2.5), pic)) / blur_bound(uo.gaussian_kernel(15, 2.5), smax)
        out = img.bessel_blur(9, 4.).to_host()
        ratios["bessel_blur"] = worst(out, per_channel(lambda ch: uo.bessel_blur(ch, 9, 4.), pic)) / blur_bound(uo.kaiser_kernel(9, 4.), smax)
    print("usm %d x %d: error / bound %s" % (H, W, {k: round(v, 3) for k, v in ratios.items()}))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.gpu
def test_one_dimensional_and_oversized_kernels(ctx):
    """1 x K and K x 1 kernels (no outer product to split), a kernel wider than the frame on the 2-D path, and the LDS limit"""
    from lib import _native
    pic = picture(9, 11, seed=5)
    smax = float(pic.max())
    img = _native.DeviceImage.from_host(pic, ctx)
    rng = np.random.default_rng(8)
    for shape in ((1, 7), (7, 1), (1, 1), (13, 15), (2, 31)):
        k = rng.random(shape); k /= k.sum()
        out = img.convolve(k).to_host()
        err = worst(out, per_channel(lambda ch: uo.conv2d_symm(ch, k), pic))
        assert err <= (k.size + 2) * EPS * smax, (shape, err)
    big = rng.random((80, 80))
    with pytest.raises(_native.NativeError) as ei:
        img.convolve(big)
    assert ei.value.code == _native.ICS_ENOSUP and "LDS" in str(ei.value)
    with pytest.raises(_native.NativeError) as ei:
        img.bilateral(35, 0.1, 2.0)
    assert ei.value.code == _native.ICS_ENOSUP


# ---- bilateral ---------------------------------------------------------------------------------------------------------------------
def bilateral_f32(source, radius, std_i, std_s):
    """utils_oracle.bilateral_filter restated in numpy float32: same formula, same offset order (x offset j slow, y offset i fast)"""
    f = np.float32
    source = np.asarray(source, dtype=f)
    filtered, W = np.zeros_like(source), np.zeros_like(source)
    pad = np.pad(source, (radius, radius), mode="symmetric")
    two_si, two_ss = f(2.0) * f(std_i) * f(std_i), f(2.0) * f(std_s) * f(std_s)
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            neighbour = pad[radius + i: radius + i + source.shape[0], radius + j: radius + j + source.shape[1]]
            d = neighbour - source
            w = np.exp(-(d * d) / two_si) * np.exp(-f(i * i + j * j) / two_ss)
            filtered += neighbour * w
            W += w
    assert filtered.dtype == f and W.dtype == f
    return filtered / W


BILATERAL_SIZES = [(64, 64), (301, 287)]
BILATERAL_PARAMS = [(3, 0.1, 2.), (5, 6.0, 3.0), (10, 6.0, 3.0)]


def bilateral_picture(H, W):
    return picture(H, W, seed=1000 + H + W)


def measure_f32_restatement():
    """worst |bilateral_f32 - utils_oracle.bilateral_filter| per parameter set over the pictures of the test (CPU only)"""
    res = {}
    for prm in BILATERAL_PARAMS:
        res[prm] = max(worst(bilateral_f32(p[..., c], *prm), uo.bilateral_filter(p[..., c].astype(np.float64), *prm))
                       for p in (bilateral_picture(H, W) for H, W in BILATERAL_SIZES) for c in range(3))
    return res


# Worst absolute difference of the numpy float32 restatement above against the float64 oracle on the test's own pictures, measured
# on the CPU, without the code under test, by
#     python tests/test_gpu_img_filters.py
# The gate is 4 x these: the device sums the (2 r + 1)^2 terms with FMA and its expf may differ from numpy's by an ulp.
F32_RESTATEMENT_ERROR = {(3, 0.1, 2.): 5.480e-07, (5, 6.0, 3.0): 6.933e-07, (10, 6.0, 3.0): 1.403e-06}


@pytest.mark.gpu
@pytest.mark.parametrize("radius,std_i,std_s", BILATERAL_PARAMS)
def test_bilateral_matches_the_float64_restatement(ctx, radius, std_i, std_s):
    from lib._native import DeviceImage
    gate = 4 * F32_RESTATEMENT_ERROR[(radius, std_i, std_s)]
    for H, W in BILATERAL_SIZES:
        pic = bilateral_picture(H, W)
        out = DeviceImage.from_host(pic, ctx).bilateral(radius, std_i, std_s).to_host()
        err = worst(out, per_channel(lambda ch: uo.bilateral_filter(ch, radius, std_i, std_s), pic))
        print("bilateral r=%d std_i=%g std_s=%g %d x %d: error %.3e, gate %.3e, ratio %.3f" % (radius, std_i, std_s, H, W, err, gate, err / gate))
        assert err <= gate, (H, W, err, gate)


@pytest.mark.gpu
def test_bilateral_properties_are_exact(ctx):
    from lib._native import DeviceImage
    for radius, std_i, std_s in BILATERAL_PARAMS + [(0, 0.2, 1.5)]:
        const = np.full((37, 45, 3), np.float32(0.37), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
        assert np.array_equal(DeviceImage.from_host(const, ctx).bilateral(radius, std_i, std_s).to_host(), const)     # fixed point, bit for bit
        pic = picture(70, 53, seed=radius)
        out = DeviceImage.from_host(pic, ctx).bilateral(radius, std_i, std_s).to_host()
        for c in range(3):
            assert out[..., c].min() >= pic[..., c].min() and out[..., c].max() <= pic[..., c].max()
        if radius == 0:
            assert np.array_equal(out, pic)
        # channels do not mix: three copies of one plane give three equal planes, and permuting the channels permutes the output
        same = np.ascontiguousarray(np.repeat(pic[..., :1], 3, axis=2))
        o = DeviceImage.from_host(same, ctx).bilateral(radius, std_i, std_s).to_host()
        assert np.array_equal(o[..., 0], o[..., 1]) and np.array_equal(o[..., 0], o[..., 2]) and np.array_equal(o[..., 0], out[..., 0])
        perm = np.ascontiguousarray(pic[..., [2, 0, 1]])
        assert np.array_equal(DeviceImage.from_host(perm, ctx).bilateral(radius, std_i, std_s).to_host(), out[..., [2, 0, 1]])


# ---- the same answer as the per-channel float64 path -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_utils_dispatch_on_a_device_image_equals_three_per_channel_calls(ctx):
    from lib import utils
    from lib._native import DeviceImage
    pic = picture(1024, 1024, seed=77)
    smax = float(pic.max())
    img = DeviceImage.from_host(pic, ctx)
    res = utils.USM(img, 9, 4., 0.5)
    assert isinstance(res, DeviceImage) and res.shape == (1024, 1024, 3)
    out = res.to_host()
    ref = np.dstack([utils.USM(pic[..., c], 9, 4., 0.5) for c in range(3)])
    assert ref.dtype == np.float64
    ratio = worst(out, ref) / usm_bound(uo.kaiser_kernel(9, 4.), 0.5, smax)
    print("utils.USM(DeviceImage) vs three float64 utils.USM(channel), 1024^2: error / bound %.3f" % ratio)
    assert ratio <= 1.0
    assert np.array_equal(img.to_host(), pic)                                                   # source untouched
    assert np.array_equal(utils.USM(img, 9, 4., 0.5).to_host(), out)                            # two runs, identical bits
    for f, args, kern in ((utils.gaussian_blur, (15, 2.5), uo.gaussian_kernel(15, 2.5)), (utils.bessel_blur, (9, 4.), uo.kaiser_kernel(9, 4.))):
        r = f(img, *args)
        assert isinstance(r, DeviceImage)
        o = r.to_host()
        assert worst(o, np.dstack([f(pic[..., c], *args) for c in range(3)])) <= blur_bound(kern, smax)
        assert np.array_equal(f(img, *args).to_host(), o)
    b = utils.bilateral_filter(img, 5, 6.0, 3.0)
    assert isinstance(b, DeviceImage) and np.array_equal(utils.bilateral_filter(img, 5, 6.0, 3.0).to_host(), b.to_host())
    assert ctx.last_kernel_ms() > 0.0                                                           # the queued filter's own kernel time


# ---- deblur_module(sharpen=...) ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pyramid", [False, True])
def test_deblur_module_sharpen(pyramid, capsys, monkeypatch):
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib._native import DeviceImage
    case = orc.synth_case(301, 287, 5, seed=4)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=101, display=False, iterations=2, pyramid=pyramid, save=False)
    for resident in (False, True):       # sharpen=None: bit-equal to the call without the argument, in both drivers
        a, pa = dv.deblur_module(pic, "a", ".", 5, device_resident=resident, **kw)
        b, pb = dv.deblur_module(pic, "b", ".", 5, device_resident=resident, sharpen=None, **kw)
        assert a.dtype == b.dtype and np.array_equal(a, b) and np.array_equal(pa, pb)
        plain = a
    amount = 0.5
    out_h, _ = dv.deblur_module(pic, "h", ".", 5, device_resident=False, sharpen=(9, 4., amount), **kw)
    count = {"up": 0, "down": 0}
    from_host, to_host = DeviceImage.from_host.__func__, DeviceImage.to_host

    def counting_from_host(cls, *a, **k):
        count["up"] += 1
        return from_host(cls, *a, **k)

    def counting_to_host(self):
        count["down"] += 1
        return to_host(self)
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(counting_from_host))
    monkeypatch.setattr(DeviceImage, "to_host", counting_to_host)
    out_d, _ = dv.deblur_module(pic, "d", ".", 5, device_resident=True, sharpen=(9, 4., amount), **kw)
    assert count == {"up": 1, "down": 1}, count                 # the frame still crosses PCIe exactly twice
    assert out_d.shape == out_h.shape == (301, 287, 3)
    assert out_d.min() >= 0 and out_d.max() <= 65535 and out_h.min() >= 0 and out_h.max() <= 65535
    assert not np.array_equal(out_d, plain)
    # the two drivers are allowed 2e-5 of the 16-bit range (tests/test_driver.py), amplified by the gain of the mask, plus the float32
    # USM against the float64 one on a gamma-encoded frame (values in [0, 1])
    gate = (1 + 2 * amount) * 2e-5 + usm_bound(uo.kaiser_kernel(9, 4.), amount, 1.0)
    diff = float(np.abs(out_d.astype(np.float64) - out_h).max()) / 65535
    print("deblur_module(sharpen) pyramid=%s: resident vs host %.3e of the 16-bit range, gate %.3e, ratio %.3f" % (pyramid, diff, gate, diff / gate))
    assert diff <= gate, (diff, gate)


if __name__ == "__main__":
    for prm, err in measure_f32_restatement().items():
        print(prm, "%.3e" % err)
