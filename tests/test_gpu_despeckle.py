"""GPU: the despeckle filter of device-resident H x W x 3 float32 images (csrc/ics_img_despeckle.hip, DeviceImage.despeckle,
lib.utils.despeckle / median_filter, deblur_module(despeckle=...)) against tests/despeckle_ref.py.

The output is a selection among the input's values by an integer order and the decision rests on one correctly rounded float32
subtraction, so every gate is bit equality (compared as uint32, so NaNs count): device against the reference, route against route,
run against run.  There is no tolerance to measure.

Shapes, T = 32 the tile edge of the LDS route: 1 x 9, 9 x 1 and 5 x 7 are smaller than a window; 33 x 1030 and 1030 x 33 thinner than
tile plus halo; 2 T x 2 T and (2 T + 1) x (2 T + 1) on and one past the tile seam; 301 x 287 has ragged last tiles both ways."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import despeckle_ref as dr
from test_despeckle import auto_threshold, bits, planted, same, special_frame, PLANTED, SIGMAS
from test_gpu_img_filters import picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32                                                  # csrc/ics_img_despeckle.hip DST, asserted below
SIZES = [(1, 9), (9, 1), (5, 7), (33, 1030), (1030, 33), (2 * T, 2 * T), (2 * T + 1, 2 * T + 1), (301, 287)]
ROUTES = (0, 1, 2)
THRESHOLDS = {"vector": (0.0, 0.1), "channel": (0.0, 0.1, (0.05, 0.1, 0.2))}


@functools.lru_cache(maxsize=None)
def frame(H, W, kind):
    f = picture(H, W, 100 + 3 * H + W)
    if kind == "ties":
        f = (np.round(f * 8) / 8).astype(np.float32)                     # multiples of 1 / 8: masses of equal values
    f.setflags(write=False)
    return f


def run_all(ctx, f, radius, coupling, threshold):
    """the reference once; every route twice: bits, counts, repeatability, agreement, the source untouched"""
    from lib._native import DeviceImage
    ref, ref_counts = dr.despeckle(f, threshold, radius, coupling)
    img = DeviceImage.from_host(f, ctx)
    first = None
    for route in ROUTES:
        out, counts = img.despeckle(threshold, radius, coupling, route=route, count=True)
        got = out.to_host()
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(ref)), (route, radius, coupling, threshold, int((bits(got) != bits(ref)).sum()))
        assert counts == ref_counts and all(isinstance(n, int) for n in counts), (route, counts, ref_counts)
        again = img.despeckle(threshold, radius, coupling, route=route)   # without the counts: the call that stays queued
        assert np.array_equal(bits(again.to_host()), bits(got))
        first = got if first is None else first
        assert np.array_equal(bits(first), bits(got))                     # the routes agree bit for bit
    assert np.array_equal(bits(img.to_host()), bits(f))                   # the source is never written
    return ref_counts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["salt", "ties"])
@pytest.mark.parametrize("H,W", SIZES)
def test_output_and_counts_have_the_bits_of_the_reference_by_every_route(ctx, H, W, kind):
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_despeckle.hip")).read()
    assert int(re.search(r"#define DST (\d+)", src).group(1)) == T
    f = frame(H, W, kind)
    for radius in (1, 2):
        for coupling in dr.COUPLINGS:
            for threshold in THRESHOLDS[coupling]:
                counts = run_all(ctx, f, radius, coupling, threshold)
                if kind == "salt" and threshold == 0.1 and H * W > 1000:     # both branches run: some values replaced, most kept
                    n = H * W * (3 if coupling == "channel" else 1)
                    assert 0.02 * n < sum(counts) < 0.6 * n, (counts, n)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2])
def test_special_values_signed_zeros_nans_infinities_and_impulses_at_every_edge(ctx, radius):
    f = special_frame()
    assert f.shape == (37, 45, 3) and np.isnan(f).sum() >= 28 and np.isinf(f).sum() == 2 and np.signbit(f[2, 5]).all()
    for coupling in dr.COUPLINGS:
        for threshold in THRESHOLDS[coupling]:
            run_all(ctx, f, radius, coupling, threshold)


@pytest.mark.gpu
@pytest.mark.parametrize("coupling", dr.COUPLINGS)
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("H,W", PLANTED)
def test_auto_is_the_devices_own_estimate_and_replaces_exactly_the_planted_impulses(ctx, H, W, sigma, coupling):
    from lib import _native
    pic, mask = planted(H, W, sigma)
    img = _native.DeviceImage.from_host(pic, ctx)
    est = img.noise_estimate(coupling)
    for form, strength in (("auto", 6.0), (("auto", 6.0), 6.0), (("auto", 8.5), 8.5)):
        t = auto_threshold(est.sigma, strength)
        thr = tuple(float(v) for v in t) if coupling == "channel" else float(t[0])
        out, counts = img.despeckle(form, 1, coupling, count=True)
        got = out.to_host()
        explicit, explicit_counts = img.despeckle(thr, 1, coupling, count=True)
        assert same(got, explicit.to_host()) and counts == explicit_counts
        ref, ref_counts = dr.despeckle(pic, t if coupling == "channel" else t[0], 1, coupling)
        assert same(got, ref) and counts == ref_counts
    out, counts = img.despeckle("auto", 1, coupling, count=True)              # strength 6: exactly the planted set
    changed = bits(out.to_host()) != bits(pic)
    if coupling == "channel":
        assert np.array_equal(changed, mask) and counts == tuple(int(mask[..., c].sum()) for c in range(3))
    else:
        assert np.array_equal(changed.any(axis=2), mask.any(axis=2)) and counts == (40,)
    assert same(img.to_host(), pic)


@pytest.mark.gpu
def test_utils_dispatch_errors_and_kernel_time(ctx, monkeypatch):
    from lib import _native, utils
    pic = frame(65, 65, "salt")
    img = _native.DeviceImage.from_host(pic, ctx)
    dev = utils.despeckle(img, 0.1, 2, "channel")
    assert ctx.last_kernel_ms() > 0.0                    # the filter's own kernel time
    assert isinstance(dev, _native.DeviceImage)
    ref, ref_counts = dr.despeckle(pic, 0.1, 2, "channel")
    assert same(dev.to_host(), ref)
    count = {"up": 0, "down": 0}
    from_host, to_host = _native.DeviceImage.from_host.__func__, _native.DeviceImage.to_host
    monkeypatch.setattr(_native.DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(_native.DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    host = utils.despeckle(pic.astype(np.float64), 0.1, 2, "channel")
    assert count == {"up": 1, "down": 1} and isinstance(host, np.ndarray) and host.dtype == np.float32 and same(host, ref)
    host, counts = utils.despeckle(pic, 0.1, 2, "channel", count=True)
    assert same(host, ref) and counts == ref_counts
    monkeypatch.undo()
    for radius in (1, 2):
        med = utils.median_filter(pic, radius)
        assert same(med, dr.median(pic, radius)) and same(med, utils.despeckle(pic, 0.0, radius, "channel"))
        assert same(utils.median_filter(img, radius).to_host(), med)
    assert same(utils.despeckle(img, 0.1).to_host(), img.despeckle(0.1, 1, "vector", 0).to_host())      # the defaults
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.despeckle(np.zeros((8, 9)), 0.1)
    with pytest.raises(ValueError, match="radius"):
        img.despeckle(0.1, 3)
    with pytest.raises(ValueError, match="route"):
        img.despeckle(0.1, 1, "vector", route=3)
    # bad arguments through the C entry on a real image: an error code, a text that names the argument, *out NULL
    lib = _native.load()
    thr = lambda *v: (C.c_float * 3)(*v)                 # noqa: E731
    nan, inf = float("nan"), float("inf")
    for src, radius, t, coupling, route, with_out, word in (
            (None, 1, thr(0.1, 0.1, 0.1), 1, 0, True, b"NULL"), (img._h, 1, thr(0.1, 0.1, 0.1), 1, 0, False, b"NULL"), (img._h, 1, None, 1, 0, True, b"threshold"),
            (img._h, 0, thr(0.1, 0.1, 0.1), 1, 0, True, b"radius"), (img._h, 3, thr(0.1, 0.1, 0.1), 0, 0, True, b"radius"),
            (img._h, 1, thr(-0.1, 0.1, 0.1), 1, 0, True, b"threshold"), (img._h, 1, thr(nan, 0.1, 0.1), 1, 0, True, b"threshold"),
            (img._h, 1, thr(0.1, 0.1, inf), 0, 0, True, b"threshold"), (img._h, 2, thr(0.1, -0.1, 0.1), 0, 1, True, b"threshold"),
            (img._h, 1, thr(0.1, 0.1, 0.1), 2, 0, True, b"coupling"), (img._h, 1, thr(0.1, 0.1, 0.1), -1, 0, True, b"coupling"),
            (img._h, 1, thr(0.1, 0.1, 0.1), 1, 3, True, b"route"), (img._h, 2, thr(0.1, 0.1, 0.1), 0, -1, True, b"route")):
        out, got = C.c_void_p(1), (C.c_uint * 3)()
        assert lib.ics_img_despeckle(src, radius, t, coupling, route, C.byref(out) if with_out else None, got) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error() and (out.value is None or not with_out), (word, lib.ics_last_error(), out.value)
    # "vector" reads threshold[0] only and leaves the other two counters 0
    out, got = C.c_void_p(), (C.c_uint * 3)(7, 7, 7)
    assert lib.ics_img_despeckle(img._h, 1, thr(0.1, nan, -1.0), 1, 0, C.byref(out), got) == _native.ICS_OK
    res = _native.DeviceImage(out, ctx)
    ref, ref_counts = dr.despeckle(pic, 0.1, 1, "vector")
    assert same(res.to_host(), ref) and list(got) == [ref_counts[0], 0, 0]
    assert same(img.to_host(), pic)


# ---- deblur_module(despeckle=...) ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deblur_module_despeckles_the_input_frame_before_both_phases(capsys, monkeypatch):
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib._native import DeviceImage
    case = orc.synth_case(99, 101, 5, seed=4)
    clean_pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    spots = [(14, 15, 0), (20, 60, 1), (45, 30, 2), (50, 85, 0), (80, 20, 1), (84, 70, 2)]      # >= 12 px from the border and from each other
    pic = clean_pic.copy()
    for y, x, c in spots:
        assert clean_pic[y, x, c] < 200
        pic[y, x, c] = 255
    kw = dict(mask_size=41, display=False, iterations=2, pyramid=False, save=False)
    res = dict(kw, device_resident=True)
    capsys.readouterr()
    plain, _ = dv.deblur_module(pic, "a", ".", 5, **res)
    text_plain = capsys.readouterr().out
    none, _ = dv.deblur_module(pic, "a", ".", 5, despeckle=None, **res)
    text_none = capsys.readouterr().out
    assert np.array_equal(plain, none) and "Despeckle" not in text_none and "Despeckle" not in text_plain      # None: the same bits, no new line
    clean, _ = dv.deblur_module(clean_pic, "a", ".", 5, **res)

    # the method is called once, with these arguments, before the first resize; its output is the reference of its input
    calls, frames = [], {}
    despeckle, resize = DeviceImage.despeckle, DeviceImage.resize

    def capturing(self, *a, **k):
        calls.append(("despeckle", a, k))
        frames["in"] = self.to_host()
        out = despeckle(self, *a, **k)
        frames["out"] = out[0].to_host()
        frames["counts"] = out[1]
        return out
    monkeypatch.setattr(DeviceImage, "despeckle", capturing)
    monkeypatch.setattr(DeviceImage, "resize", lambda self, *a: (calls.append(("resize", a, {})), resize(self, *a))[1])
    capsys.readouterr()
    out, _ = dv.deblur_module(pic, "a", ".", 5, despeckle=(0.1, 1, "channel"), **res)
    text = capsys.readouterr().out
    monkeypatch.setattr(DeviceImage, "despeckle", despeckle)
    monkeypatch.setattr(DeviceImage, "resize", resize)
    assert [c[0] for c in calls].count("despeckle") == 1 and calls[0] == ("despeckle", (0.1, 1, "channel"), {"count": True}) and calls[1][0] == "resize"
    ref, ref_counts = dr.despeckle(frames["in"], 0.1, 1, "channel")
    assert frames["in"].shape == (101, 103, 3) and same(frames["out"], ref) and frames["counts"] == ref_counts
    assert all(n >= 2 for n in ref_counts) and "Despeckle : %s replaced" % ", ".join(str(n) for n in ref_counts) in text

    # the frame crosses PCIe once each way
    count = {"up": 0, "down": 0}
    from_host, to_host = DeviceImage.from_host.__func__, DeviceImage.to_host
    monkeypatch.setattr(DeviceImage, "from_host", classmethod(lambda cls, *a, **k: (count.__setitem__("up", count["up"] + 1), from_host(cls, *a, **k))[1]))
    monkeypatch.setattr(DeviceImage, "to_host", lambda self: (count.__setitem__("down", count["down"] + 1), to_host(self))[1])
    for form in ((0.1, 1, "channel"), ("auto",)):
        count.update(up=0, down=0)
        again, _ = dv.deblur_module(pic, "a", ".", 5, despeckle=form, **res)
        assert count == {"up": 1, "down": 1}, (form, count)
        if form[0] == 0.1:
            assert np.array_equal(again, out)
    monkeypatch.undo()

    # the host path and the resident path agree as tests/test_driver.py allows its two drivers
    host, _ = dv.deblur_module(pic, "a", ".", 5, despeckle=(0.1, 1, "channel"), device_resident=False, **kw)
    diff = float(np.abs(host.astype(np.float64) - out).max()) / 65535
    print("deblur_module(despeckle): host vs resident %.3e of the 16-bit range, gate 2e-5" % diff)
    assert host.shape == out.shape and diff <= 2e-5, diff

    # around the planted pixels the result is closer to that of the untouched picture with despeckle than without
    def worst(a):
        return max(float(np.abs(a[y - 4:y + 5, x - 4:x + 5].astype(np.float64) - clean[y - 4:y + 5, x - 4:x + 5]).max()) for y, x, _ in spots)
    print("deblur_module(despeckle): largest difference to the untouched picture's result around the planted pixels: %.1f with, %.1f without" % (worst(out), worst(plain)))
    assert worst(out) < worst(plain)

    # with the other steps: despeckle, the two phases, then denoise -> clarity -> local_contrast -> detail -> sharpen
    order = []
    for name in ("despeckle", "tv_denoise", "local_laplacian", "wavelet_equalize", "guided_filter", "usm"):
        fn = getattr(DeviceImage, name)
        monkeypatch.setattr(DeviceImage, name, lambda self, *a, _fn=fn, _name=name, **k: (order.append(_name), _fn(self, *a, **k))[1])
    rl = dv.dc.richardson_lucy_MM_device
    monkeypatch.setattr(dv.dc, "richardson_lucy_MM_device", lambda *a, **k: (order.append("blind" if k["blind"] else "non-blind"), rl(*a, **k))[1])
    full, _ = dv.deblur_module(pic, "a", ".", 5, despeckle=(0.1,), denoise=(0.05, 5), clarity=(0.2, 1.5), local_contrast=((1.0, 1.4, 1.2),),
                               detail=(4, 1e-3, 1.2), sharpen=(3, 1.0, 0.5), **res)
    assert order == ["despeckle", "blind", "non-blind", "tv_denoise", "local_laplacian", "wavelet_equalize", "guided_filter", "usm"], order
    assert full.shape == plain.shape and np.isfinite(full).all()
