"""GPU: every size-, radius- and channel-selected form of the bicubic resize (csrc/ics_resize.hip) and the strided form of
k_img_pad_edge (csrc/ics_img.hip) against scipy.ndimage (oracle/resize_oracle.py: resize_scipy, float64).

tests/test_resize.py pins the resize up to 513 x 771, where a prefilter line has at most 795 samples, every row kernel makes one
trip and the anti-aliasing taps fit the LDS table.  The forms beyond that are chosen by the launcher from the shape alone, so thin
strips reach them with a few kilobytes of data:
  * prefilter segments of 32 / 64 / 128 samples (rs_seg: padded line length n = H + 24 or W + 24 below 1024, from 1024, from 4096),
    with the ragged last segment and the exact initialisation next to both ends of the line, on the y pass and -- after the
    transpose -- on the x pass;
  * row grids capped at 64 workgroups (W C > 16384): k_rs_pad, k_rs_gauss_y and k_rs_gauss_x stride, the last restaging its LDS run;
  * the flat Gaussian k_rs_gauss<AXIS, InT> from 2 r + 1 > 64 taps, on both axes, next to the last radius of the LDS table;
  * launch_resize_t<float, float> (DeviceImage.resize, the resident driver's route) through all of the above;
  * C != 3: k_rs_transpose and the second half of k_rs_eval over several 32 x 32 tiles with ragged edges, growing and shrinking.
No gate is new: 1e-12 (tests/test_resize.py) where the anti-aliasing radius is 0 or 1, EXTREME_GATE for the wide kernels,
RESIZE_GATE (tests/test_driver.py) for float32 frames.  The CPU side of the segment rule: tests/test_resize_segments.py."""
import functools
import gc

import numpy as np
import pytest

import resize_oracle as ro
from test_driver import RESIZE_GATE
from test_resize import EXTREME_GATE

pytestmark = pytest.mark.gpu

GATE = 1e-12      # tests/test_resize.py::test_gpu_resize_matches_the_oracle

# (source, destination, anti-aliasing radius on y and x, gate, what it reaches)
SEGMENTS = [
    ((999, 5), (705, 7), (1, 0), GATE, "n = 1023: segments of 32, ragged last segment"),
    ((1000, 5), (1415, 4), (0, 1), GATE, "n = 1024: the first line of 64-sample segments"),
    ((4071, 4), (2879, 6), (1, 0), GATE, "n = 4095: segments of 64, ragged last segment"),
    ((4072, 4), (5759, 3), (0, 1), GATE, "n = 4096: the first line of 128-sample segments"),
    ((5, 4072), (7, 2879), (0, 1), GATE, "n = 4096 on the x pass, behind the transpose"),
    ((1501, 6), (1061, 6), (1, 0), GATE, "n = 1525: between the boundaries, no multiple of 64"),
]
STRIDED = [
    ((6, 5600), (9, 3960), (0, 1), GATE, "W C = 16800: k_rs_pad strides, k_rs_gauss_x restages its run"),
    ((6, 5600), (5, 7920), (0, 0), GATE, "W C = 16800: k_rs_pad and k_rs_gauss_y stride"),
]
FLAT = [
    ((330, 9), (20, 9), (31, 0), EXTREME_GATE, "r = 31 on y: the last radius of the LDS table"),
    ((340, 9), (20, 9), (32, 0), EXTREME_GATE, "r = 32 on y: the flat form"),
    ((9, 330), (9, 20), (0, 31), EXTREME_GATE, "r = 31 on x"),
    ((9, 340), (9, 20), (0, 32), EXTREME_GATE, "r = 32 on x"),
    ((700, 9), (20, 12), (68, 0), EXTREME_GATE, "r = 68, flat on y while x grows"),
    ((9, 700), (12, 20), (0, 68), EXTREME_GATE, "r = 68, flat on x while y grows"),
]
CASES = SEGMENTS + STRIDED + FLAT
CHANNEL_CASES = [((70, 45), (99, 64), (0, 0), GATE, "several tiles, ragged edges, growing"),
                 ((99, 64), (70, 45), (1, 1), GATE, "several tiles, ragged edges, shrinking"),
                 SEGMENTS[1], FLAT[3]]


def ident(case):
    return "%dx%d-%dx%d" % (*case[0], *case[1])


def radii(src, dst):
    return tuple(int(4 * ro.aa_sigma(a, b) + 0.5) for a, b in zip(src, dst))


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pictures(src, dst, channels=3):
    """the float64 picture and its reference, the float32 picture and its reference: computed once, shared, read-only"""
    img = np.random.default_rng(src[0] * 10007 + src[1] * 31 + dst[0]).random((*src, channels))
    img32 = img.astype(np.float32)
    ref32 = ro.resize_scipy(img32, dst).astype(np.float32) if channels == 3 else None
    return frozen(img), frozen(ro.resize_scipy(img, dst)), frozen(img32), ref32


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def report(what, err, gate):
    print("%s: worst |gpu - ref| = %.3e, gate %.1e (%.2g of it)" % (what, err, gate, err / gate))


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_float64_api(ctx, case):
    src, dst, r, gate, what = case
    assert radii(src, dst) == r, what            # a later edit of a shape cannot silently leave the boundary it was chosen for
    img, ref, _, _ = pictures(src, dst)
    got = ctx.resize_bicubic(img, dst)
    assert got.shape == (*dst, 3) and got.dtype == np.float64
    err = np.abs(got - ref).max()
    report("float64 %s [%s]" % (ident(case), what), err, gate)
    assert err < gate, what


def test_float64_api_on_16_bit_values(ctx):
    """data in [0, 65535] on the 128-sample segments: the gate scales with the data, the error must too"""
    src, dst = (4072, 4), (2879, 6)
    assert radii(src, dst) == (1, 0)
    img = np.random.default_rng(16).random((*src, 3)) * 65535.0
    ref = ro.resize_scipy(img, dst)
    err, gate = np.abs(ctx.resize_bicubic(img, dst) - ref).max(), GATE * np.abs(ref).max()
    report("float64 16-bit range %dx%d-%dx%d" % (*src, *dst), err, gate)
    assert err < gate


@pytest.mark.parametrize("case", CHANNEL_CASES, ids=ident)
def test_other_channel_counts(ctx, case):
    """C = 1, 2 and 4 against the oracle, and every plane of a multi-channel call equal, bit for bit, to the single-channel call on that
    plane: the arithmetic of a value does not depend on C (C = 3, whose transpose and evaluation are kernels of their own, included)"""
    src, dst, r, gate, what = case
    assert radii(src, dst) == r, what
    img, ref, _, _ = pictures(src, dst, 4)
    single = [ctx.resize_bicubic(np.ascontiguousarray(img[..., c]), dst) for c in range(4)]
    for c in range(4):
        assert single[c].shape == dst
    err = max(np.abs(single[c] - ref[..., c]).max() for c in range(4))
    report("C = 1 %s [%s]" % (ident(case), what), err, gate)
    assert err < gate, what
    for C in (2, 3, 4):
        got = ctx.resize_bicubic(np.ascontiguousarray(img[..., :C]), dst)
        assert got.shape == (*dst, C)
        err = np.abs(got - ref[..., :C]).max()
        report("C = %d %s [%s]" % (C, ident(case), what), err, gate)
        assert err < gate, (C, what)
        for c in range(C):
            assert np.array_equal(bits(got[..., c]), bits(single[c])), "plane %d of the C = %d call differs from the single-channel call" % (c, C)


def resize_f32(img32, dst):
    from lib import _native
    d = _native.DeviceImage.from_host(img32)
    r = d.resize(*dst)
    out = r.to_host()
    d.close(); r.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_float32_route(ctx, case):
    """DeviceImage.resize: k_rs_gauss_y / k_rs_gauss_x / k_rs_gauss<0> / k_rs_gauss<1> / k_rs_pad read float32, k_rs_eval writes it"""
    src, dst, r, _, what = case
    assert radii(src, dst) == r, what
    _, _, img32, ref32 = pictures(src, dst)
    got = resize_f32(img32, dst)
    assert got.shape == (*dst, 3) and got.dtype == np.float32
    err = np.abs(got - ref32).max()
    report("float32 %s [%s]" % (ident(case), what), err, RESIZE_GATE)
    assert err < RESIZE_GATE, what


def test_wide_pad_edge_equals_numpy(ctx):
    """3 (W + left + right) = 16929 values a row, more than 64 x 256: k_img_pad_edge strides"""
    from lib import _native
    a = np.random.default_rng(5).random((5, 5600, 3)).astype(np.float32)
    assert 3 * (a.shape[1] + 3 + 40) > 64 * 256
    d = _native.DeviceImage.from_host(a)
    p = d.pad_edge(1, 2, 3, 40)
    got = p.to_host()
    d.close(); p.close()
    want = np.pad(a, ((1, 2), (3, 40), (0, 0)), mode="edge")
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def test_on_poisoned_red_zoned_pool_blocks(ctx, debug_switch):
    """pool check mode (csrc/ics_pool.h), as tests/test_gpu_wiener.py: every block a call takes is filled with 0xFF (NaN) and its red
    zone verified when it goes back.  A segment that warmed up from scratch memory nobody wrote, or a strided trip that staged past
    its run, would spread NaN; a store past a buffer's end would be counted."""
    from lib import _native
    from lib import deconvolution as dc
    from test_gpu_pool_check import selftest
    ok, seen = selftest()                        # the check mode demonstrably fills what it hands out and finds a planted byte
    assert ok, seen
    cases = [SEGMENTS[3], STRIDED[0], FLAT[3]]

    def run():
        out = []
        for src, dst, _, _, _ in cases:
            img, _, img32, _ = pictures(src, dst)
            out.append((ctx.resize_bicubic(img, dst), resize_f32(img32, dst)))
        return out

    clean = run()
    dc._drop_jobs(); gc.collect()
    _native.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned = run()
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    ctx.conv2d_symm(np.zeros((2, 2)), np.ones((1, 1)))       # returns the context's last check-mode scratch block (tests/test_gpu_pool_check.py)
    assert _native.debug_set("pool_overruns", 0) == 0
    for case, (c64, c32), (p64, p32) in zip(cases, clean, poisoned):
        src, dst, _, gate, what = case
        _, ref, _, ref32 = pictures(src, dst)
        assert np.array_equal(bits(p64), bits(c64)) and np.array_equal(bits(p32), bits(c32)), what
        assert np.abs(p64 - ref).max() < gate and np.abs(p32 - ref32).max() < RESIZE_GATE, what
