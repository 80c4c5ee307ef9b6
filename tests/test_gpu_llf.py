"""GPU: the fast local Laplacian filter of device-resident H x W x 3 float32 images (csrc/ics_img_llf.hip,
DeviceImage.local_laplacian, lib.utils.local_laplacian, deblur_module(clarity=...)) against the float64 oracle tests/llf_ref.py.

Gate against the oracle: 4 x the worst |float32 restatement - float64 oracle| of (coupling, levels J, samples K) over the test's own
pictures and both argument sets, measured on the CPU without the code under test (F32_RESTATEMENT_ERROR below; `python
tests/test_gpu_llf.py` prints them).  The factor 4 covers what the device may do differently from numpy's float32 (expf, the
division k / (K - 1)).  Every entry must stay at or below 1e-6, every gate at or below 4e-6: an entry above that would mean that its
input amplifies rounding, and the input would have to go, not the gate.

Shapes: 1 x 9, 9 x 1 and 5 x 7 are smaller than the five taps; 33 x 1030 and 1030 x 33 are thin; 64 x 64 sits on the edge of a
32 x 32 tile of level 1 and 65 x 65 one pixel past it; 127 x 130 halves as the odd and even chains 127 -> 64 -> 32 ... and
130 -> 65 -> 33 -> 17 -> 9; 301 x 287 has ragged last tiles both ways; one picture is scaled to -0.1 .. 1.2 so that the clamp of t
runs.  J 1, 3, 6; K 2, 5, 8 and 16 once (J = 3); both couplings; (sigma 0.2, detail 2, edges 0.8) and (sigma 0.05, detail 0.5,
edges 1)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
import llf_ref as lr
from test_gpu_img_filters import picture

SIZES = [(1, 9), (9, 1), (5, 7), (33, 1030), (1030, 33), (64, 64), (65, 65), (127, 130), (301, 287)]
WIDE = (127, 130, "wide")                              # the picture scaled to -0.1 .. 1.2
LEVELS = [1, 3, 6]
ARGS = [(0.2, 2.0, 0.8), (0.05, 0.5, 1.0)]


def samples(J):
    return (2, 5, 8, 16) if J == 3 else (2, 5, 8)


@functools.lru_cache(maxsize=None)
def llf_picture(H, W, wide=None):
    pic = picture(H, W, seed=7000 + 3 * H + W)
    if wide:
        pic = ((pic - pic.min()) / (pic.max() - pic.min()) * np.float32(1.3) - np.float32(0.1)).astype(np.float32)
        assert pic.min() < -0.09 and pic.max() > 1.19
    pic.setflags(write=False)
    return pic


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@functools.lru_cache(maxsize=None)
def oracle(shape, args, J, K, coupling):
    """the float64 oracle of the test's picture, computed once and never written"""
    ref = lr.local_laplacian(llf_picture(*shape), *args, levels=J, samples=K, coupling=coupling)
    ref.setflags(write=False)
    return ref


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| per (coupling, J, K) over the pictures and argument sets of the test"""
    res = {}
    for coupling in lr.COUPLINGS:
        for J in LEVELS:
            for K in samples(J):
                res[coupling, J, K] = max(worst(lr.local_laplacian(llf_picture(*shape), *args, levels=J, samples=K, coupling=coupling, dtype=np.float32),
                                                oracle(shape, args, J, K, coupling)) for shape in SIZES + [WIDE] for args in ARGS)
    return res


# Measured on the CPU by `python tests/test_gpu_llf.py`, without the code under test.
F32_RESTATEMENT_ERROR = {
    ('channel', 1, 2): 2.001e-07, ('channel', 1, 5): 2.094e-07, ('channel', 1, 8): 2.001e-07,
    ('channel', 3, 2): 2.508e-07, ('channel', 3, 5): 2.668e-07, ('channel', 3, 8): 2.700e-07, ('channel', 3, 16): 2.883e-07,
    ('channel', 6, 2): 3.004e-07, ('channel', 6, 5): 3.285e-07, ('channel', 6, 8): 3.831e-07,
    ('vector', 1, 2): 2.395e-07, ('vector', 1, 5): 2.279e-07, ('vector', 1, 8): 2.527e-07,
    ('vector', 3, 2): 2.596e-07, ('vector', 3, 5): 2.493e-07, ('vector', 3, 8): 2.727e-07, ('vector', 3, 16): 2.735e-07,
    ('vector', 6, 2): 2.894e-07, ('vector', 6, 5): 3.447e-07, ('vector', 6, 8): 3.182e-07}


@pytest.mark.gpu
@pytest.mark.parametrize("J", LEVELS)
@pytest.mark.parametrize("coupling", lr.COUPLINGS)
def test_matches_the_float64_oracle_and_the_routes_agree_bit_for_bit(ctx, coupling, J):
    from lib import _native
    assert _native.IMG_LLF_MAX_LEVELS == lr.MAX_LEVELS == 10 and _native.IMG_LLF_MAX_SAMPLES == lr.MAX_SAMPLES == 16
    for shape in SIZES + [WIDE]:
        pic = llf_picture(*shape)
        img = _native.DeviceImage.from_host(pic, ctx)
        for K in samples(J):
            gate = 4 * F32_RESTATEMENT_ERROR[coupling, J, K]
            assert 0 < gate <= 4e-6                      # see the module docstring
            for args in ARGS:
                ref = oracle(shape, args, J, K, coupling)
                outs = {}
                for route in (0, 1, 2):
                    out = outs[route] = img.local_laplacian(*args, levels=J, samples=K, coupling=coupling, route=route).to_host()
                    err = worst(out, ref)
                    print("llf %s J %d K %d %s %s route %d: error %.3e, gate %.3e, ratio %.3f" % (coupling, J, K, args, shape, route, err, gate, err / gate))
                    assert out.dtype == np.float32 and out.shape == pic.shape
                    assert err <= gate, (shape, K, args, route, err, gate)
                    again = img.local_laplacian(*args, levels=J, samples=K, coupling=coupling, route=route).to_host()     # two runs, identical bits
                    assert np.array_equal(again.view(np.uint32), out.view(np.uint32)), (shape, K, args, route)
                    assert np.array_equal(img.to_host(), pic)        # the source is unchanged after every call
                for route in (1, 2):
                    assert np.array_equal(outs[route].view(np.uint32), outs[0].view(np.uint32)), (shape, K, args, route, worst(outs[route], outs[0]))
        img.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", lr.COUPLINGS)
def test_exact_properties_on_the_device(ctx, coupling):
    from lib._native import DeviceImage
    # a constant picture, whatever the arguments: every pyramid of a constant is that constant exactly (the 6 of the taps is split
    # into 2 + 4), so every Laplacian coefficient is +0 and the collapse returns G (tests/test_llf.py)
    const = np.full((37, 45, 3), np.float32(0.375), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    img = DeviceImage.from_host(const, ctx)
    for J in (1, 3, 6):
        for route in (1, 2):
            for args, K in (((0.2, 2.0, 0.8), 8), ((0.05, 0.5, 1.0), 5), ((0.3, 1.7, 0.9), 8), ((1.0, 3.0, 1.0), 2), ((0.01, 0.0, 0.25), 16)):
                out = img.local_laplacian(*args, levels=J, samples=K, coupling=coupling, route=route).to_host()
                assert np.array_equal(out.view(np.uint32), const.view(np.uint32)), (J, route, args, K, worst(out, const))
    # detail = edges = 1 on values in {0, 1/4, 1/2, 3/4} with K = 5: the samples are the values, every intermediate is exactly
    # representable and the picture comes back bit for bit.  Per channel only: the luma of such a pixel has a full mantissa.
    if coupling == "channel":
        for H, W in ((37, 45), (1, 9), (9, 1), (5, 7), (64, 64), (65, 65)):
            pic = (np.random.default_rng(H * 100 + W).integers(0, 4, (H, W, 3)) / 4.0).astype(np.float32)
            img = DeviceImage.from_host(pic, ctx)
            for J in (1, 2):
                for route in (1, 2):
                    out = img.local_laplacian(0.2, 1.0, 1.0, levels=J, samples=5, coupling=coupling, route=route).to_host()
                    assert np.array_equal(out.view(np.uint32), pic.view(np.uint32)), (H, W, J, route, worst(out, pic))
            assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
def test_utils_dispatch_default_levels_errors_and_kernel_time(ctx, monkeypatch):
    from lib import _native, utils
    pic = llf_picture(120, 131)
    img = _native.DeviceImage.from_host(pic, ctx)
    res = utils.local_laplacian(img, 0.2, 1.8, 1.0, None, 8, "channel")
    assert isinstance(res, _native.DeviceImage) and res.shape == (120, 131, 3)
    assert ctx.last_kernel_ms() > 0.0                    # the queued filter's own kernel time
    dev = res.to_host()
    assert _native.llf_levels(120, 131) == lr.default_levels(120, 131) == 4      # 131 -> 66 -> 33 -> 17 -> 9
    assert np.array_equal(dev.view(np.uint32), img.local_laplacian(0.2, 1.8, levels=4, coupling="channel").to_host().view(np.uint32))
    count = {"up": 0, "down": 0}
    from_host, to_host = _native.DeviceImage.from_host.__func__, _native.DeviceImage.to_host
    monkeypatch.setattr(_native.DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(_native.DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    host = utils.local_laplacian(pic.astype(np.float64), 0.2, 1.8, 1.0, None, 8, "channel")          # an array: one upload, one download
    monkeypatch.undo()
    assert count == {"up": 1, "down": 1}, count
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host.view(np.uint32), dev.view(np.uint32))
    assert np.array_equal(utils.local_laplacian(img, 0.2, 1.8).to_host(), img.local_laplacian(0.2, 1.8, 1.0, 4, 8, "vector").to_host())   # the defaults
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.local_laplacian(np.zeros((8, 9)), 0.2, 1.8)
    with pytest.raises(ValueError, match="coupling"):
        img.local_laplacian(0.2, 1.8, coupling="colour")
    # bad arguments through the C entry: an error code, a text that names the argument, no image
    lib = _native.load()
    ok = (0.2, 1.8, 1.0, 3, 8, 1, 0)
    nan, inf = float("nan"), float("inf")
    for pos, value, word in ((0, 0.0, b"sigma"), (0, -0.2, b"sigma"), (0, nan, b"sigma"), (0, inf, b"sigma"), (1, -0.5, b"detail"), (1, nan, b"detail"),
                             (1, inf, b"detail"), (2, 0.0, b"edges"), (2, -1.0, b"edges"), (2, nan, b"edges"), (2, inf, b"edges"),
                             (1, float(np.nextafter(np.float32(3), np.float32(4))), b"detail"), (3, 0, b"levels"), (3, 11, b"levels"), (4, 1, b"samples"),
                             (4, 17, b"samples"), (5, 2, b"coupling"), (5, -1, b"coupling"), (6, 3, b"route"), (6, -1, b"route")):
        a = list(ok)
        a[pos] = value
        out = C.c_void_p(1)
        assert lib.ics_img_local_laplacian(img._h, *a, C.byref(out)) == _native.ICS_EINVAL, (word, a)
        assert word in lib.ics_last_error() and out.value is None, (word, lib.ics_last_error())
    assert np.array_equal(img.to_host(), pic)


# ---- deblur_module(clarity=...) ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deblur_module_clarity_resident_against_the_host_frame_path(capsys, monkeypatch):
    """The same picture through deblur_module(clarity=...) with the frames on the host and resident in HBM: both hand the deblurred
    gamma-encoded frame to the same device operator; they differ by float32 powf of the gamma steps, numpy against device, which
    is what tests/test_driver.py allows its two drivers: 2e-5 of the 16-bit range."""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib._native import DeviceImage
    case = orc.synth_case(99, 101, 5, seed=4)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=41, display=False, iterations=2, pyramid=False, save=False)
    clarity = (0.2, 1.8, 0.9, "channel")
    plain, _ = dv.deblur_module(pic, "a", ".", 5, device_resident=True, **kw)
    none, _ = dv.deblur_module(pic, "a", ".", 5, device_resident=True, clarity=None, **kw)
    assert np.array_equal(plain, none)                   # None: bit-equal to the call without the argument
    host, _ = dv.deblur_module(pic, "a", ".", 5, device_resident=False, clarity=clarity, **kw)
    count = {"up": 0, "down": 0}
    order = []
    from_host, to_host = DeviceImage.from_host.__func__, DeviceImage.to_host
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    for name in ("tv_denoise", "local_laplacian", "wavelet_equalize", "guided_filter", "usm"):
        monkeypatch.setattr(DeviceImage, name, (lambda name, fn: lambda self, *a, **k: (order.append((name,) + a), fn(self, *a, **k))[1])(name, getattr(DeviceImage, name)))
    out, _ = dv.deblur_module(pic, "a", ".", 5, device_resident=True, clarity=clarity, **kw)
    assert count == {"up": 1, "down": 1}, count          # the frame still crosses PCIe exactly twice
    assert order == [("local_laplacian", 0.2, 1.8, 0.9, None, 8, "channel")], order
    assert out.shape == plain.shape == host.shape and out.min() >= 0 and out.max() <= 65535 and not np.array_equal(out, plain)
    diff = float(np.abs(out.astype(np.float64) - host).max()) / 65535
    print("deblur_module(clarity): resident vs host frames %.3e of the 16-bit range, gate 2e-5, ratio %.3f" % (diff, diff / 2e-5))
    assert diff <= 2e-5, diff
    # with the other steps: denoise -> clarity -> local_contrast -> detail -> sharpen
    order.clear()
    dv.deblur_module(pic, "a", ".", 5, device_resident=True, denoise=(0.05, 4), clarity=(0.2, 1.0, 0.6), local_contrast=((1.0, 1.5),), detail=(8, 1e-3, 1.5),
                     sharpen=(5, 2., 0.5), **kw)
    assert [o[0] for o in order] == ["tv_denoise", "local_laplacian", "wavelet_equalize", "guided_filter", "usm"], order
    assert order[1] == ("local_laplacian", 0.2, 1.0, 0.6, None, 8, "vector")


if __name__ == "__main__":
    rows = measure_f32_restatement()
    for coupling in lr.COUPLINGS:
        for J in LEVELS:
            print("    " + " ".join("(%r, %d, %d): %.3e," % (coupling, J, K, rows[coupling, J, K]) for K in samples(J)))
