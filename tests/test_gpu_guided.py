"""GPU: the guided filter of device-resident H x W x 3 float32 images (csrc/ics_img_guided.hip, DeviceImage.guided_filter,
lib.utils.guided_filter, deblur_module(detail=...)) against the float64 oracle tests/guided_ref.py.

Gate against the oracle: 4 x the worst |float32 restatement - float64 oracle| of (coupling, radius, eps) over the test's own pictures
and both detail settings, measured on the CPU without the code under test (F32_RESTATEMENT_ERROR below; `python
tests/test_gpu_guided.py` prints them).  The factor 4 covers what the device may do differently from numpy's float32 (the order inside
the determinant, the divisions).  Every entry must stay at or below 1e-6, every gate at or below 4e-6: an entry above that would mean
that its input amplifies rounding, and the input would have to go, not the gate.

Shapes: 1 x 9, 9 x 1 and 5 x 7 are smaller than every window; 33 x 1030 and 1030 x 33 are thinner than the halo of the fused route;
64 x 64 sits exactly on two 32 x 32 tiles per axis and 65 x 65 one pixel past them; 301 x 287 has ragged last tiles both ways.
Radii: 1, 4, the largest the fused route takes, one above it (two-launch route only) and 32."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
import guided_ref as gr
from test_gpu_img_filters import picture

TILE = 32                                               # the output tile of every route (csrc/ics_img_guided.hip)
FUSED = 8                                               # lib._native.IMG_GUIDED_FUSED_RADIUS (checked below)
SIZES = [(1, 9), (9, 1), (5, 7), (33, 1030), (1030, 33), (2 * TILE, 2 * TILE), (2 * TILE + 1, 2 * TILE + 1), (301, 287)]
RADII = [1, 4, FUSED, FUSED + 1, 32]
EPS = [1e-2, 1e-4]
DETAILS = [0.0, 1.5]


def gf_picture(H, W):
    return picture(H, W, seed=5000 + 3 * H + W)


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def routes(r):
    return (0, 1, 2) if r <= FUSED else (0, 1)


@functools.lru_cache(maxsize=None)
def base(H, W, coupling, r, eps):
    """the float64 base layer of the test's picture, computed once and never written"""
    q = gr.base_layer(gf_picture(H, W), r, eps, coupling)
    q.setflags(write=False)
    return q


def oracle(H, W, coupling, r, eps, detail):
    q = base(H, W, coupling, r, eps)
    return q if detail == 0 else q + np.float64(np.float32(detail)) * (gf_picture(H, W).astype(np.float64) - q)


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| per (coupling, radius, eps) over the pictures and detail settings of the test"""
    res = {}
    for coupling in gr.COUPLINGS:
        for r in RADII:
            for eps in EPS:
                res[coupling, r, eps] = max(worst(gr.guided_filter(gf_picture(H, W), r, eps, d, coupling, dtype=np.float32), oracle(H, W, coupling, r, eps, d))
                                            for H, W in SIZES for d in DETAILS)
    return res


# Measured on the CPU by `python tests/test_gpu_guided.py`, without the code under test.
F32_RESTATEMENT_ERROR = {
    ('channel', 1, 0.01): 9.437e-08, ('channel', 1, 0.0001): 1.008e-07,
    ('channel', 4, 0.01): 9.226e-08, ('channel', 4, 0.0001): 1.324e-07,
    ('channel', 8, 0.01): 1.034e-07, ('channel', 8, 0.0001): 1.458e-07,
    ('channel', 9, 0.01): 1.151e-07, ('channel', 9, 0.0001): 1.328e-07,
    ('channel', 32, 0.01): 2.322e-07, ('channel', 32, 0.0001): 3.306e-07,
    ('vector', 1, 0.01): 1.044e-07, ('vector', 1, 0.0001): 1.196e-07,
    ('vector', 4, 0.01): 1.024e-07, ('vector', 4, 0.0001): 1.300e-07,
    ('vector', 8, 0.01): 1.031e-07, ('vector', 8, 0.0001): 1.507e-07,
    ('vector', 9, 0.01): 1.084e-07, ('vector', 9, 0.0001): 1.357e-07,
    ('vector', 32, 0.01): 2.072e-07, ('vector', 32, 0.0001): 3.584e-07}


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("coupling", gr.COUPLINGS)
def test_matches_the_float64_oracle_and_the_routes_agree_bit_for_bit(ctx, coupling, r):
    from lib import _native
    assert _native.IMG_GUIDED_FUSED_RADIUS == FUSED and _native.IMG_GUIDED_MAX_RADIUS == 32
    for H, W in SIZES:
        pic = gf_picture(H, W)
        img = _native.DeviceImage.from_host(pic, ctx)
        for eps in EPS:
            gate = 4 * F32_RESTATEMENT_ERROR[coupling, r, eps]
            assert 0 < gate <= 4e-6                      # see the module docstring
            for d in DETAILS:
                ref = oracle(H, W, coupling, r, eps, d)
                outs = {}
                for route in routes(r):
                    out = outs[route] = img.guided_filter(r, eps, d, coupling, route=route).to_host()
                    err = worst(out, ref)
                    print("guided %s r %d eps %g detail %g %d x %d route %d: error %.3e, gate %.3e, ratio %.3f" % (coupling, r, eps, d, H, W, route, err, gate, err / gate))
                    assert out.dtype == np.float32 and out.shape == pic.shape
                    assert err <= gate, (H, W, eps, d, route, err, gate)
                    again = img.guided_filter(r, eps, d, coupling, route=route).to_host()         # two runs, identical bits
                    assert np.array_equal(again.view(np.uint32), out.view(np.uint32)), (H, W, eps, d, route)
                    assert np.array_equal(img.to_host(), pic)        # the source is unchanged after every call
                for route in routes(r)[1:]:
                    assert np.array_equal(outs[route].view(np.uint32), outs[0].view(np.uint32)), (H, W, eps, d, route, worst(outs[route], outs[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", gr.COUPLINGS)
def test_exact_properties_on_the_device(ctx, coupling):
    from lib._native import DeviceImage
    # a constant with few significant bits and eps a power of two: every sum, product and quotient is exact (tests/test_guided.py)
    const = np.full((37, 45, 3), np.float32(0.375), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    img = DeviceImage.from_host(const, ctx)
    for r in (1, FUSED, 32):
        for route in routes(r):
            for eps, d in ((2.0 ** -7, 0.0), (2.0 ** -13, 1.5)):
                assert np.array_equal(img.guided_filter(r, eps, d, coupling, route=route).to_host(), const), (r, route, eps, d)
    pic = gf_picture(70, 53)
    img = DeviceImage.from_host(pic, ctx)
    for r in (3, 12):
        for route in routes(r)[1:]:
            q = img.guided_filter(r, 1e-3, 0.0, coupling, route=route).to_host()
            assert worst(q, pic) > 1e-2
            if coupling == "channel":                    # every channel by itself: permuting the channels permutes the output bit for bit
                out = img.guided_filter(r, 1e-3, 1.5, coupling, route=route).to_host()
                for order in ([2, 0, 1], [1, 0, 2]):
                    perm = DeviceImage.from_host(np.ascontiguousarray(pic[..., order]), ctx)
                    assert np.array_equal(perm.guided_filter(r, 1e-3, 1.5, coupling, route=route).to_host().view(np.uint32), out[..., order].view(np.uint32))
            # detail 0 is q itself and not a blend: q recovered from the detail-2 output, 2 I - (q + 2 (I - q)), is the same layer.  The
            # detail-2 output carries the roundings of I - q (2 x 2^-25 after the doubling) and of the final sum (2^-23 below 4).
            out2 = img.guided_filter(r, 1e-3, 2.0, coupling, route=route).to_host()
            assert worst(q, 2.0 * pic.astype(np.float64) - out2) <= 1.5 * 2.0 ** -23, (r, route)
            assert np.array_equal(img.guided_filter(r, 1e-3, -0.0, coupling, route=route).to_host().view(np.uint32), q.view(np.uint32))
            one = img.guided_filter(r, 1e-3, 1.0, coupling, route=route).to_host()
            assert worst(one, pic) <= 2.0 ** -23             # q + (I - q): an ulp of values below 2
    assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
def test_utils_dispatch_errors_and_kernel_time(ctx, monkeypatch):
    from lib import _native, utils
    pic = gf_picture(120, 131)
    img = _native.DeviceImage.from_host(pic, ctx)
    res = utils.guided_filter(img, 6, 1e-3, 1.5, "channel")
    assert isinstance(res, _native.DeviceImage) and res.shape == (120, 131, 3)
    assert ctx.last_kernel_ms() > 0.0                    # the queued filter's own kernel time
    dev = res.to_host()
    count = {"up": 0, "down": 0}
    from_host, to_host = _native.DeviceImage.from_host.__func__, _native.DeviceImage.to_host
    monkeypatch.setattr(_native.DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(_native.DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    host = utils.guided_filter(pic.astype(np.float64), 6, 1e-3, 1.5, "channel")                        # an array: one upload, one download
    monkeypatch.undo()
    assert count == {"up": 1, "down": 1}, count
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host.view(np.uint32), dev.view(np.uint32))
    assert np.array_equal(utils.guided_filter(img, 6, 1e-3).to_host(), img.guided_filter(6, 1e-3, 0.0, "vector").to_host())   # the defaults
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.guided_filter(np.zeros((8, 9)), 6, 1e-3)
    with pytest.raises(ValueError, match="coupling"):
        img.guided_filter(6, 1e-3, coupling="colour")
    # bad arguments through the C entry: an error code, a text that names the argument, no image
    lib = _native.load()
    for radius, eps, detail, coupling, route, word in ((0, 1e-3, 0.0, 1, 0, b"radius"), (33, 1e-3, 0.0, 1, 0, b"radius"), (4, 0.0, 0.0, 1, 0, b"eps"),
                                                       (4, -1.0, 0.0, 1, 0, b"eps"), (4, float("nan"), 0.0, 1, 0, b"eps"), (4, float("inf"), 0.0, 1, 0, b"eps"),
                                                       (4, 1e-3, float("nan"), 1, 0, b"detail"), (4, 1e-3, 0.0, 2, 0, b"coupling"), (4, 1e-3, 0.0, 1, 3, b"route"),
                                                       (FUSED + 1, 1e-3, 0.0, 1, 2, b"route")):
        out = C.c_void_p(1)
        assert lib.ics_img_guided(img._h, radius, eps, detail, coupling, route, C.byref(out)) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error() and out.value is None, (word, lib.ics_last_error())
    assert np.array_equal(img.to_host(), pic)


# ---- deblur_module(detail=...) -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deblur_module_detail_on_the_resident_frame(capsys, monkeypatch):
    """The resident driver with detail equals the resident driver without it followed by the operator on the gamma-encoded frame
    (taken from the plain call just before its final gamma step), the clip, the power 2.2 and the crop done in numpy.  Both apply the
    same device operator to the same bits; what differs is float32 powf, device against numpy, which is what tests/test_driver.py
    allows its two drivers: 2e-5 of the 16-bit range."""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib._native import DeviceImage
    case = orc.synth_case(99, 101, 5, seed=4)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=41, display=False, iterations=2, pyramid=False, save=False, device_resident=True)
    detail = (8, 1e-3, 1.5, "channel")
    plain, _ = dv.deblur_module(pic, "a", ".", 5, **kw)
    none, _ = dv.deblur_module(pic, "a", ".", 5, detail=None, **kw)
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
    gf = DeviceImage.from_host(frames[0]).guided_filter(*detail).to_host()
    expect = (np.clip(gf, 0., 1.) ** 2.2 * (2 ** 16 - 1))[1:-1, 1:-1]     # 99 + 2 and 101 + 2 are odd: no further padding to undo
    count = {"up": 0, "down": 0}
    order = []
    from_host, to_host = DeviceImage.from_host.__func__, DeviceImage.to_host
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    for name in ("tv_denoise", "wavelet_equalize", "guided_filter", "usm"):
        monkeypatch.setattr(DeviceImage, name, (lambda name, fn: lambda self, *a, **k: (order.append((name,) + a), fn(self, *a, **k))[1])(name, getattr(DeviceImage, name)))
    out, _ = dv.deblur_module(pic, "a", ".", 5, detail=detail, **kw)
    assert count == {"up": 1, "down": 1}, count          # the frame still crosses PCIe exactly twice
    assert order == [("guided_filter",) + detail], order
    assert out.shape == plain.shape == expect.shape and out.min() >= 0 and out.max() <= 65535 and not np.array_equal(out, plain)
    diff = float(np.abs(out.astype(np.float64) - expect).max()) / 65535
    print("deblur_module(detail): resident vs plain + operator %.3e of the 16-bit range, gate 2e-5, ratio %.3f" % (diff, diff / 2e-5))
    assert diff <= 2e-5, diff
    # with the other steps: denoise -> local_contrast -> detail -> sharpen
    order.clear()
    dv.deblur_module(pic, "a", ".", 5, denoise=(0.05, 4), local_contrast=((1.0, 1.5),), detail=detail[:3], sharpen=(5, 2., 0.5), **kw)
    assert [o[0] for o in order] == ["tv_denoise", "wavelet_equalize", "guided_filter", "usm"], order
    assert order[2] == ("guided_filter", 8, 1e-3, 1.5, "vector")


if __name__ == "__main__":
    rows = measure_f32_restatement()
    for coupling in gr.COUPLINGS:
        for r in RADII:
            print("    " + " ".join("(%r, %d, %g): %.3e," % (coupling, r, eps, rows[coupling, r, eps]) for eps in EPS))
