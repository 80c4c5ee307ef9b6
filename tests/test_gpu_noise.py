"""GPU: the noise estimate of device-resident H x W x 3 float32 images (csrc/ics_img_noise.hip, DeviceImage.noise_estimate,
lib.utils.noise_estimate) and the automatic thresholds of the wavelet equaliser built on it (thresholds="auto" through
DeviceImage.wavelet_equalize, lib.utils.wavelet_equalizer and deblur_module(local_contrast=...)), against tests/noise_ref.py.

The median is an order statistic of values each of which is a chain of single, correctly rounded float32 operations in a stated
order (wavelet_ref.axis_pass along x, then y; the subtraction; for "vector" three products, two sums smallest first, one square root):
the device must return the bits of the float32 restatement (np.partition at rank (n - 1) // 2), on every shape, in both couplings, by
every route.  A difference is a bug, not a tolerance.  Beside that the house protocol: the median within 4 x the worst |float32
restatement - float64 oracle| over the test's own pictures, measured on the CPU without the code under test (F32_RESTATEMENT_ERROR
below; `python tests/test_gpu_noise.py` prints it).

Shapes: 1 x 1 (n = 1); 1 x 2 (n even: the lower median); 1 x 9, 9 x 1 and 5 x 7 fold every offset; 3 x 1030 and 1030 x 3 are thinner
than tile and halo of the keys route; 32 x 128 sits exactly on two of its 16 x 64 tiles per axis and 33 x 129 one pixel past them;
301 x 287 and 700 x 513 have ragged last tiles and give several persistent workgroups of route 1 (4 x 64 tiles, at most cus x 3 or
cus x 4 workgroups) several tiles each; route 2 (16 x 64 tiles and 1024-key units, 396 and 351 of them at most) stays below its caps on
256 CUs there.  It wraps on 1030 x 1100 (tests/trips_ref.py BIG: 1170 tiles and 1107 key units for at most 1024 workgroups, asserted from
the device's CU count), and on 301 x 287 with the max_wgs switch at 2 and at 1, where one workgroup walks every tile and unit."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests"), os.path.join(root, "image-cases-studies_amd")]
import noise_ref as nr
import trips_ref as tr
from test_noise import noisy_ramp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_H, TILE_W = 16, 64                                 # the keys route's tile (csrc/ics_img_noise.hip, asserted below)
SIZES = [(1, 1), (1, 2), (1, 9), (9, 1), (5, 7), (3, 1030), (1030, 3), (2 * TILE_H, 2 * TILE_W), (2 * TILE_H + 1, 2 * TILE_W + 1), (301, 287),
         (700, 513), tr.BIG]
ROUTES = (0, 1, 2)


def ns_picture(H, W):
    return noisy_ramp(H, W, 0.02, seed=5000 + 3 * H + W)


def bits(values):
    return [int(np.float32(v).view(np.uint32)) for v in values]


@functools.lru_cache(maxsize=None)
def reference(H, W, coupling):
    """(float32 restatement, float64 oracle) medians of the test's picture, computed once"""
    pic = ns_picture(H, W)
    return tuple(nr.medians(pic, coupling, np.float32)), tuple(nr.medians(pic, coupling, np.float64))


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| of the median per coupling over the pictures of the test (CPU only)"""
    return {coupling: max(abs(float(a) - float(b)) for H, W in SIZES for a, b in zip(*reference(H, W, coupling))) for coupling in nr.COUPLINGS}


# Measured on the CPU by `python tests/test_gpu_noise.py`, without the code under test (on 1030 x 1100 alone: 8.149e-09 and 1.303e-08).
F32_RESTATEMENT_ERROR = {"channel": 4.843e-08, "vector": 4.641e-08}


def check(est, pic, coupling):
    """an estimate against the restatement of the picture: the median's bits, and level and sigma by the host formula from that median"""
    ref = nr.medians(pic, coupling, np.float32)
    assert len(est.median) == len(est.level) == len(est.sigma) == len(ref) == (3 if coupling == "channel" else 1)
    assert all(isinstance(v, float) for v in est.median + est.level + est.sigma)
    assert bits(est.median) == bits(ref), (est.median, ref)
    derived = [nr.derived(m, coupling) for m in est.median]
    assert bits(est.level) == bits(d[0] for d in derived) and bits(est.sigma) == bits(d[1] for d in derived)


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", nr.COUPLINGS)
@pytest.mark.parametrize("H,W", SIZES)
def test_median_has_the_bits_of_the_restatement_by_every_route(ctx, H, W, coupling):
    from lib._native import DeviceImage, NoiseEstimate
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_noise.hip")).read()
    assert {m: int(v) for m, v in re.findall(r"#define (NSTW|NSTH) (\d+)", src)} == {"NSTW": TILE_W, "NSTH": TILE_H}
    gate = 4 * F32_RESTATEMENT_ERROR[coupling]
    assert 0 < gate <= 4e-6                              # c_1 carries six roundings of values <= 1 (2^-24 each), w_0 one more; the median is one w_0
    pic = ns_picture(H, W)
    ref32, ref64 = reference(H, W, coupling)
    img = DeviceImage.from_host(pic, ctx)
    got = {}
    if (H, W) == tr.BIG:                                 # the frame that is here for the caps: it must exceed them on this device
        for route in (1, 2):
            for kernel, (units, cap) in tr.noise_grids(H, W, coupling, route, ctx.compute_units).items():
                print("noise %s %d x %d on %d CUs, %s: %d units for %d workgroups" % (coupling, H, W, ctx.compute_units, kernel, units, cap))
                assert units > cap, (kernel, units, cap)
    for route in ROUTES:
        est = img.noise_estimate(coupling, route=route)
        assert isinstance(est, NoiseEstimate)
        assert bits(est.median) == bits(ref32), (route, est.median, ref32)
        check(est, pic, coupling)
        err = max(abs(a - float(b)) for a, b in zip(est.median, ref64))
        print("noise %s %d x %d route %d: median %s, error to the oracle %.3e, gate %.3e" % (coupling, H, W, route, est.median, err, gate))
        assert err <= gate, (route, err, gate)
        got[route] = est
        assert img.noise_estimate(coupling, route=route) == est        # two runs, identical bits
        assert np.array_equal(img.to_host(), pic)                      # the source is never written
    assert got[1] == got[2] == got[0]                                  # the routes agree bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", nr.COUPLINGS)
def test_two_workgroups_and_one_that_walk_every_tile_give_the_same_bits(ctx, debug_switch, coupling):
    """the max_wgs switch caps every persistent grid of the launcher: on 301 x 287 (380 tiles of route 1; 95 tiles and 85 key units of
    route 2) two workgroups, then one, take every tile and unit in turn and add them to one live LDS histogram.  The counts are
    integers: the median has the bits of the uncapped run and of the restatement whoever walks the tiles."""
    from lib._native import DeviceImage
    H, W = 301, 287
    for route in (1, 2):
        assert all(units > 2 for units, _ in tr.noise_grids(H, W, coupling, route).values())
    pic = ns_picture(H, W)
    ref32, _ = reference(H, W, coupling)
    img = DeviceImage.from_host(pic, ctx)
    full = {route: img.noise_estimate(coupling, route=route) for route in ROUTES}
    for cap in (2, 1):
        debug_switch("max_wgs", cap)
        capped = {route: img.noise_estimate(coupling, route=route) for route in ROUTES}
        debug_switch("max_wgs", 0)
        for route in ROUTES:
            assert bits(capped[route].median) == bits(ref32), (route, cap, capped[route].median, ref32)
            assert capped[route] == full[route], (route, cap)
            check(capped[route], pic, coupling)
    assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("coupling", nr.COUPLINGS)
def test_inputs_that_aim_at_the_select(ctx, coupling, route):
    from lib._native import DeviceImage, auto_thresholds
    n = 3 if coupling == "channel" else 1
    # a constant: every key is 0, the rank lies in bin 0 of every pass
    const = np.full((37, 45, 3), np.float32(0.375), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    est = DeviceImage.from_host(const, ctx).noise_estimate(coupling, route=route)
    assert est.median == est.level == est.sigma == (0.0,) * n and bits(est.median) == [0] * n
    assert not auto_thresholds(est.level, 5).any()
    # four levels, multiples of 1 / 8, one per column and channel: w_0 is exact and takes at most one value per column, each 131 times,
    # so the rank falls inside a bin of equal keys in every pass; and the same levels drawn per pixel, with fewer ties
    rng = np.random.default_rng(17)
    cols = np.ascontiguousarray(np.broadcast_to(rng.integers(0, 4, (1, 97, 3)) / 8.0, (131, 97, 3)), dtype=np.float32)
    pops, med = nr.populations(cols, coupling, np.float32), nr.medians(cols, coupling, np.float32)
    assert all(np.unique(p).size <= 97 and int(np.sum(p == m)) >= 131 and m > 0 for p, m in zip(pops, med))
    for quant in (cols, (rng.integers(0, 4, (131, 97, 3)) / 8.0).astype(np.float32)):
        img = DeviceImage.from_host(quant, ctx)
        check(img.noise_estimate(coupling, route=route), quant, coupling)
        assert np.array_equal(img.to_host(), quant)
    # noise on a ramp, and the same times 2^-7 and 2^3: other exponent bins, medians scaled exactly
    pic = ns_picture(301, 287)
    base = DeviceImage.from_host(pic, ctx).noise_estimate(coupling, route=route)
    check(base, pic, coupling)
    for k in (-7, 3):
        scaled = pic * np.float32(2.0 ** k)
        est = DeviceImage.from_host(scaled, ctx).noise_estimate(coupling, route=route)
        check(est, scaled, coupling)
        assert bits(est.median) == bits(m * 2.0 ** k for m in base.median)


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", nr.COUPLINGS)
def test_automatic_thresholds_are_the_estimate_put_into_the_equaliser(ctx, coupling):
    from lib import _native, utils
    gains = (1.0, 1.6, 1.8, 1.4, 1.0)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))     # noqa: E731
    pic = ns_picture(120, 131)
    img = _native.DeviceImage.from_host(pic, ctx)
    est = img.noise_estimate(coupling)
    for form, strength in (("auto", 3.0), (("auto", 1.5), 1.5)):
        thr = _native.auto_thresholds(est.level, len(gains), strength)
        assert thr[0] > 0
        explicit = img.wavelet_equalize(gains, thr, 1.0, coupling).to_host()
        assert same(img.wavelet_equalize(gains, form, 1.0, coupling).to_host(), explicit)
        assert same(utils.wavelet_equalizer(img, gains, form, 1.0, coupling).to_host(), explicit)
        assert same(utils.wavelet_equalizer(pic, gains, form, 1.0, coupling), explicit)
    plain = img.wavelet_equalize(gains, None, 1.0, coupling).to_host()
    assert not same(plain, explicit)
    assert same(img.wavelet_equalize(gains, ("auto", 0.0), 1.0, coupling).to_host(), plain)       # strength 0: no thresholds, on any picture
    const = np.full((37, 45, 3), np.float32(0.375), np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    cimg = _native.DeviceImage.from_host(const, ctx)
    assert same(cimg.wavelet_equalize(gains, "auto", 1.0, coupling).to_host(), cimg.wavelet_equalize(gains, None, 1.0, coupling).to_host())
    with pytest.raises(ValueError, match="thresholds"):
        img.wavelet_equalize(gains, "automatic")
    assert np.array_equal(img.to_host(), pic)


@pytest.mark.gpu
def test_utils_dispatch_errors_and_kernel_time(ctx):
    from lib import _native, utils
    pic = ns_picture(120, 131)
    img = _native.DeviceImage.from_host(pic, ctx)
    for coupling in nr.COUPLINGS:
        dev = utils.noise_estimate(img, coupling)
        assert ctx.last_kernel_ms() > 0.0                # the estimate's own kernel time
        assert isinstance(dev, _native.NoiseEstimate) and utils.noise_estimate(pic.astype(np.float64), coupling) == dev     # an array: one upload
        check(dev, pic, coupling)
    assert utils.noise_estimate(img) == img.noise_estimate("vector", 0)      # the defaults
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.noise_estimate(np.zeros((8, 9)))
    with pytest.raises(ValueError, match="coupling"):
        img.noise_estimate("colour")
    with pytest.raises(ValueError, match="route"):
        img.noise_estimate("vector", route=3)
    # bad arguments through the C entry: an error code and a text that names the argument
    lib = _native.load()
    buf = lambda: (C.c_float * 3)()                      # noqa: E731
    for src, coupling, route, med, lev, sig, word in ((None, 1, 0, buf(), buf(), buf(), b"src"), (img._h, 1, 0, None, buf(), buf(), b"median"),
                                                      (img._h, 1, 0, buf(), None, buf(), b"level"), (img._h, 1, 0, buf(), buf(), None, b"sigma"),
                                                      (img._h, 2, 0, buf(), buf(), buf(), b"coupling"), (img._h, -1, 0, buf(), buf(), buf(), b"coupling"),
                                                      (img._h, 0, 3, buf(), buf(), buf(), b"route"), (img._h, 0, -1, buf(), buf(), buf(), b"route")):
        assert lib.ics_img_noise_estimate(src, coupling, route, med, lev, sig) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error(), (word, lib.ics_last_error())
    assert np.array_equal(img.to_host(), pic)


# ---- deblur_module(local_contrast=(gains, "auto", coupling)) ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_deblur_module_automatic_local_contrast_on_the_resident_frame(capsys, monkeypatch):
    """As tests/test_gpu_wavelet.py's local-contrast test: the resident driver with local_contrast=(gains, "auto", "channel") equals the
    resident driver without it followed, on the gamma-encoded frame taken from the plain call just before its final gamma step, by
    the estimate, the explicit thresholds made of it, the equaliser, and the clip, the power 2.2 and the crop in numpy.  Both apply the
    same device operators to the same bits; what differs is float32 powf, device against numpy: 2e-5 of the 16-bit range."""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib._native import DeviceImage, auto_thresholds
    case = orc.synth_case(99, 101, 5, seed=4)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=41, display=False, iterations=2, pyramid=False, save=False, device_resident=True)
    gains = (1.0, 1.6, 1.8, 1.4, 1.0)
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
    frame = DeviceImage.from_host(frames[0])
    thr = auto_thresholds(frame.noise_estimate("channel").level, len(gains))
    assert thr[0] > 0
    eq = frame.wavelet_equalize(gains, thr, 1.0, "channel").to_host()
    expect = (np.clip(eq, 0., 1.) ** 2.2 * (2 ** 16 - 1))[1:-1, 1:-1]     # 99 + 2 and 101 + 2 are odd: no further padding to undo
    count = {"up": 0, "down": 0}
    order = []
    from_host, to_host, wavelet, noise = DeviceImage.from_host.__func__, DeviceImage.to_host, DeviceImage.wavelet_equalize, DeviceImage.noise_estimate
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    monkeypatch.setattr(DeviceImage, "wavelet_equalize", lambda self, *a, **k: (order.append(("wavelet_equalize",) + a), wavelet(self, *a, **k))[1])
    monkeypatch.setattr(DeviceImage, "noise_estimate", lambda self, *a, **k: (order.append(("noise_estimate",) + a), noise(self, *a, **k))[1])
    out, _ = dv.deblur_module(pic, "a", ".", 5, local_contrast=(gains, "auto", "channel"), **kw)
    assert count == {"up": 1, "down": 1}, count          # the frame still crosses PCIe exactly twice
    assert order == [("wavelet_equalize", gains, ("auto", 3.0), 1.0, "channel"), ("noise_estimate", "channel")], order    # the equaliser asks for the estimate
    assert out.shape == plain.shape == expect.shape and out.min() >= 0 and out.max() <= 65535 and not np.array_equal(out, plain)
    diff = float(np.abs(out.astype(np.float64) - expect).max()) / 65535
    print("deblur_module(local_contrast auto): resident vs plain + estimate + operator %.3e of the 16-bit range, gate 2e-5, ratio %.3f" % (diff, diff / 2e-5))
    assert diff <= 2e-5, diff


if __name__ == "__main__":
    for coupling, err in measure_f32_restatement().items():
        print(coupling, "%.3e" % err)
