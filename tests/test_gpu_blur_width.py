"""GPU: the derivative autocorrelation of device-resident H x W x 3 float32 images (csrc/ics_img_blurwidth.hip,
DeviceImage.blur_profile) and the blur width read from it (lib.utils.estimate_blur_width, deblur_module(blur_width="auto")), against
tests/blur_width_ref.py.

Profiles, the house protocol: for every lag |device - float64 oracle| <= 4 x F32_RESTATEMENT_ERROR x A(0), the constant being the
worst |float32 restatement - oracle| / A(0) over this test's own frames, measured on the CPU without the code under test
(`python tests/test_gpu_blur_width.py` prints it).  The margin is 4 because the device sums a tile in another order than numpy's
pairwise sum, at the same depth.  The pair counts are integers and must be equal.

Shapes (t = the tile, ACTH x ACTW): 1 x 1 (no difference at all); 1 x 9 and 9 x 1 (one axis has none); 5 x 7 with lags beyond the
frame; t and t + 1 pixels a side (one tile of difference values, and the pixel that completes it); 2 t and 2 t + 1 (two tiles per axis,
and one pixel past them); 70 x 200 at the largest lag (the halo longer than the tile and, along y, than the frame); 301 x 287 (ragged
tiles, several per workgroup -- many with the max_wgs switch at 2); a window with an odd origin inside a frame whose outside is 1e30."""
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
import blur_width_ref as br
import test_blur_width as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_H, T_W = br.ACTH, br.ACTW
# (H, W, L, max_wgs switch)
SHAPES = [(1, 1, 0, 0), (1, 9, 4, 0), (9, 1, 4, 0), (5, 7, 8, 0), (T_H, T_W, 16, 0), (T_H + 1, T_W + 1, 16, 0), (2 * T_H, 2 * T_W, 16, 0),
          (2 * T_H + 1, 2 * T_W + 1, 16, 0), (70, 200, 128, 0), (301, 287, 64, 0), (301, 287, 64, 2)]
WINDOW_CASE = ((200, 260), (13, 150, 7, 230), 32)


@functools.lru_cache(maxsize=None)
def bw_picture(H, W):
    """a picture whose differences correlate over a few pixels: the 3 x 3 box mean of uniform noise on a ramp"""
    rng = np.random.default_rng(7000 + 3 * H + W)
    base = rng.random((H + 2, W + 2, 3))
    box = sum(base[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    ramp = 0.25 * (np.arange(W)[None, :, None] / float(W) + np.arange(H)[:, None, None] / float(H))
    pic = (0.5 * box + ramp).astype(np.float32)
    pic.setflags(write=False)
    return pic


def frames():
    """(picture, window, L) of every profile comparison in this file"""
    out = [(bw_picture(H, W), (0, H, 0, W), L) for H, W, L, _ in SHAPES]
    (H, W), window, L = WINDOW_CASE
    out.append((bw_picture(H, W), window, L))
    out.append((bw_picture(65, 97), (0, 65, 0, 97), 16))                       # the pool-check case
    return out


@functools.lru_cache(maxsize=None)
def oracle(H, W, window, L):
    return br.profiles(bw_picture(H, W), window, L, np.float64)


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| / A(0) over the lags, axes and frames of this file (CPU only)"""
    worst = 0.0
    for pic, window, L in frames():
        o, r = br.profiles(pic, window, L, np.float64), br.profiles(pic, window, L, np.float32)
        assert o[2].tolist() == r[2].tolist() and o[3].tolist() == r[3].tolist()
        for a64, a32 in zip(o[:2], r[:2]):
            if a64[0] > 0:
                worst = max(worst, float(np.abs(a32 - a64).max() / a64[0]))
    return worst


# Measured on the CPU by `python tests/test_gpu_blur_width.py`, without the code under test.
F32_RESTATEMENT_ERROR = 5.721e-07


def check_profile(prof, ref, what):
    """a device profile against the oracle's: counts equal, every lag within the gate"""
    gate = 4 * F32_RESTATEMENT_ERROR
    # a luma carries three roundings at values <= 1 (2^-24 each), so a difference d is off by some 1e-7 and a product by 2e-7 / |d| of
    # itself: 1e-5 at |d| = 0.02; the mean over n pairs brings that down by sqrt(n), so the smallest frames set the constant
    assert 0 < gate <= 1e-5
    Ax, Ay, nx, ny = ref
    assert prof.ax.dtype == prof.ay.dtype == np.float64 and prof.nx.dtype == prof.ny.dtype == np.int64
    assert prof.nx.tolist() == nx.tolist() and prof.ny.tolist() == ny.tolist(), what
    for name, got, want in (("x", prof.ax, Ax), ("y", prof.ay, Ay)):
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        print("blur profile %s axis %s: A(0) %.4e, error to the oracle %.3e, gate %.3e" % (what, name, want[0], err, gate * want[0]))
        assert err <= gate * want[0], (what, name, err, gate * want[0])
        assert not got[want == 0].any()                   # no pair: exactly 0


def same(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,L,max_wgs", SHAPES)
def test_profiles_against_the_oracle(ctx, debug_switch, H, W, L, max_wgs):
    from lib._native import BlurProfile, DeviceImage
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_blurwidth.hip")).read()
    assert {m: int(v) for m, v in re.findall(r"#define (ACTW|ACTH) (\d+)", src)} == {"ACTW": T_W, "ACTH": T_H}
    if max_wgs:
        debug_switch("max_wgs", max_wgs)
    pic = bw_picture(H, W)
    img = DeviceImage.from_host(pic, ctx)
    prof = img.blur_profile(L)
    assert isinstance(prof, BlurProfile) and ctx.last_kernel_ms() > 0.0
    check_profile(prof, oracle(H, W, (0, H, 0, W), L), "%d x %d L %d wgs %d" % (H, W, L, max_wgs))
    assert same(img.blur_profile(L, (0, H, 0, W)), prof)                       # the window spelled out, and a second run: identical bits
    assert np.array_equal(img.to_host(), pic)                                  # the source is never written


@pytest.mark.gpu
def test_the_capped_grid_returns_the_bits_of_the_full_one(ctx, debug_switch):
    from lib._native import DeviceImage
    img = DeviceImage.from_host(bw_picture(301, 287), ctx)
    full = img.blur_profile(64)
    debug_switch("max_wgs", 2)
    assert same(img.blur_profile(64), full)                                    # the partials are per tile: who walks them does not matter


@pytest.mark.gpu
def test_two_calls_return_the_same_bits(ctx):
    from lib._native import DeviceImage
    img = DeviceImage.from_host(bw_picture(301, 287), ctx)
    first = img.blur_profile(64)
    other = DeviceImage.from_host(bw_picture(70, 200), ctx).blur_profile(128)  # other work on the pool in between
    assert other.ax.shape == (129,)
    assert same(img.blur_profile(64), first)


@pytest.mark.gpu
def test_window_with_an_odd_origin_sees_nothing_outside_it(ctx):
    from lib._native import DeviceImage
    (H, W), window, L = WINDOW_CASE
    y0, y1, x0, x1 = window
    pic = bw_picture(H, W)
    walled = np.full((H, W, 3), np.float32(1e30), np.float32)
    walled[y0:y1, x0:x1] = pic[y0:y1, x0:x1]
    prof = DeviceImage.from_host(walled, ctx).blur_profile(L, window)
    check_profile(prof, oracle(H, W, window, L), "window %s of %d x %d L %d" % (window, H, W, L))
    crop = DeviceImage.from_host(np.ascontiguousarray(pic[y0:y1, x0:x1]), ctx).blur_profile(L)
    assert same(prof, crop)                                                    # bit for bit the cropped frame's
    assert same(DeviceImage.from_host(pic, ctx).blur_profile(L, window), crop)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", tb.SEEDS)
def test_estimates_equal_the_oracle(ctx, seed):
    from lib import _native, utils
    for kind, w, _ in tb.CASES:
        width, ex, ey, _, _ = tb.oracle(seed, kind, w)
        frame = tb.dead_leaves(seed, tb.H, tb.W, kind, w)
        img = _native.DeviceImage.from_host(frame, ctx)
        for est in (utils.estimate_blur_width(img, tb.L - 1), utils.estimate_blur_width(frame, tb.L - 1)):
            assert isinstance(est, utils.BlurWidth)
            print("seed %d %s %d: device %d (x %.4f, y %.4f), oracle %d (x %.4f, y %.4f)" % (seed, kind, w, est.width, est.extent_x, est.extent_y, width, ex, ey))
            assert est.width == width and abs(est.extent_x - ex) <= 1e-3 and abs(est.extent_y - ey) <= 1e-3
        assert np.array_equal(img.to_host(), frame)


@pytest.mark.gpu
def test_saturation_errors_and_the_c_entry(ctx):
    from lib import _native, utils
    frame = tb.dead_leaves(tb.SEEDS[0], tb.H, tb.W, "box", 25)
    img = _native.DeviceImage.from_host(frame, ctx)
    for src in (img, frame):
        with pytest.raises(ValueError, match="blur wider than max_width"):
            utils.estimate_blur_width(src, 15)
    assert utils.estimate_blur_width(img, 63).width >= 19                      # within the lags it is read
    bad = np.array(frame)
    bad[80, 90, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        _native.DeviceImage.from_host(bad, ctx).blur_profile(8)
    with pytest.raises(ValueError, match="max_lag"):
        img.blur_profile(129)
    with pytest.raises(ValueError, match="window"):
        img.blur_profile(8, (0, tb.H + 1, 0, tb.W))
    lib = _native.load()
    n = 5
    ax, ay, nx, ny = (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)(), (C.c_longlong * n)()
    H, W = tb.H, tb.W
    for args, word in (((None, 0, H, 0, W, 4, ax, ay, nx, ny), b"src"), ((img._h, 0, H, 0, W, 4, None, ay, nx, ny), b"output"),
                       ((img._h, 0, H, 0, W, 4, ax, ay, nx, None), b"output"), ((img._h, 5, 5, 0, W, 4, ax, ay, nx, ny), b"window"),
                       ((img._h, 0, H + 1, 0, W, 4, ax, ay, nx, ny), b"window"), ((img._h, 0, H, -1, W, 4, ax, ay, nx, ny), b"window"),
                       ((img._h, 0, H, 7, 3, 4, ax, ay, nx, ny), b"window"), ((img._h, 0, H, 0, W, -1, ax, ay, nx, ny), b"max_lag"),
                       ((img._h, 0, H, 0, W, 129, ax, ay, nx, ny), b"max_lag")):
        assert lib.ics_img_blur_profile(*args) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error(), (word, lib.ics_last_error())
    assert lib.ics_img_blur_profile(img._h, 0, H, 0, W, 4, ax, ay, nx, ny) == _native.ICS_OK and nx[0] == H * (W - 1) and ny[4] == W * (H - 5)


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [True, False])
def test_deblur_module_auto_equals_the_explicit_width(capsys, resident):
    import deconvolve as dv
    seed = tb.SEEDS[0]
    assert tb.oracle(seed, "box", 9)[0] == 9
    frame = tb.dead_leaves(seed, tb.H, tb.W, "box", 9)
    pic = (np.clip(frame, 0.0, 1.0).astype(np.float64) ** 2.2 * 255.0).astype(np.float32)
    kw = dict(pyramid=False, iterations=1, save=False, display=False, mask_size=63, device_resident=resident)
    auto, psf_auto = dv.deblur_module(pic, "a", ".", "auto", **kw)
    printed = capsys.readouterr().out
    assert printed.count("Blur width : 9 (x ") == 1, printed
    nine, psf_nine = dv.deblur_module(pic, "a", ".", 9, **kw)
    assert "Blur width" not in capsys.readouterr().out
    assert psf_auto.shape == (9, 9, 3) and auto.shape == (tb.H, tb.W, 3)
    assert auto.dtype == nine.dtype and auto.tobytes() == nine.tobytes()       # bit for bit
    assert np.asarray(psf_auto).tobytes() == np.asarray(psf_nine).tobytes()
    wide, _ = dv.deblur_module(pic, "a", ".", ("auto", 15), **kw)              # the other form, and the mask window
    assert wide.tobytes() == nine.tobytes()
    masked, psf_m = dv.deblur_module(pic, "a", ".", "auto", mask=[80, 96], **kw)
    assert psf_m.shape == (9, 9, 3) and "Blur width : 9 (x " in capsys.readouterr().out
    with pytest.raises(ValueError, match="blur wider than max_width"):
        dv.deblur_module(pic, "a", ".", ("auto", 5), **kw)


@pytest.mark.gpu
def test_profiles_on_poisoned_pool_blocks(ctx, debug_switch):
    """the pool in check mode, switched as tests/test_gpu_pool_check.py switches it: the partials buffer and the result block come
    filled with 0xFF (NaN) or 0x7F (3.4e38); every partial is written before it is read, nothing is stored past a block"""
    import test_gpu_pool_check as pc
    from lib import _native
    ok, seen = pc.selftest()
    assert ok, seen
    pic = bw_picture(65, 97)

    def run():
        img = _native.DeviceImage.from_host(pic, ctx)
        try:
            return tuple(img.blur_profile(16))
        finally:
            img.close()

    pc.quiesce()
    pc.overruns()
    ref = run()
    pc.quiesce()
    for byte in (0xFF, 0x7F):
        debug_switch("pool_check", byte)
        got = run()
        pc.quiesce()
        assert same(got, ref), "fill %#x changes the profiles" % byte
    debug_switch("pool_check", -1)
    pc.quiesce()
    ctx.conv2d_symm(np.zeros((2, 2)), np.ones((1, 1)))                         # returns the context's last check-mode scratch block to the pool
    assert pc.overruns() == 0
    check_profile(_native.BlurProfile(*ref), oracle(65, 97, (0, 65, 0, 97), 16), "65 x 97 L 16")


if __name__ == "__main__":
    print("%.3e" % measure_f32_restatement())
