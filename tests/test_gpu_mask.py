"""GPU: the choice of the PSF-estimation window on device-resident H x W x 3 float32 images (csrc/ics_img_mask.hip,
DeviceImage.window_scores, lib.utils.best_mask, deblur_module(mask="auto")), against tests/mask_ref.py.

Scores, the house protocol: for every candidate |device score - float64 oracle| <= 4 x F32_RESTATEMENT_ERROR x the oracle's trace of
that candidate (the trace of the chosen box, the one that comes back, under the same gate), the constant being the worst
|float32 restatement - oracle| / trace over this file's own frames, measured on the CPU without the code under test
(`python tests/test_gpu_mask.py` prints it).  The margin is 4 because the device sums a cell in another order than numpy's pairwise
sum, at the same depth.  The clipped count is an integer and must be equal; the chosen (i, j) must be the oracle's (the frames leave
the best candidate a lead of at least twice the gate, asserted).

Shapes (T = the cell kernel's tile side): one cell; 16 x 17 and 17 x 16 (the pixel that completes a difference); 31 (off = 7);
33 x 49 with a box of 17 (2 x 3 candidates of one cell); T; T + 16 by T + 17 (a tile plus one cell, ragged); 2 T + 1 (two tiles per
axis and one pixel past them); 70 x 200; 301 x 287 with boxes of 63 (also with the max_wgs switch at 2) and of 255 (n = 15); 1360 x 1360
with a box of 16: 85 x 85 = 7225 candidates, between 7 and 8 times the pick's 1024 lanes, so that its lanes 0 .. 56 compare eight
candidates in one unrolled trip and the others seven in the tail (the oracle leaves the best candidate of this picture 4800 times the
lead the check asks for).  The tie rule across the two loop forms has a test of its own, on pictures whose ties are exact."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests"), os.path.join(root, "image-cases-studies_amd")]
import mask_ref as mr
import test_mask as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = mr.TILE
CLIP = 0.99
# (H, W, size, max_wgs switch)
SHAPES = [(16, 16, 16, 0), (16, 17, 16, 0), (17, 16, 16, 0), (31, 31, 31, 0), (33, 49, 17, 0), (T, T, T, 0), (T + 16, T + 17, T, 0),
          (2 * T + 1, 2 * T + 1, 48, 0), (70, 200, 63, 0), (301, 287, 63, 0), (301, 287, 63, 2), (301, 287, 255, 0), (1360, 1360, 16, 0)]
WALL_CASE = ((200, 260), (13, 150, 7, 230), 63)
POOL_CASE = (65, 97, 17)
PATCH_CASE = (96, 112, 16)


@functools.lru_cache(maxsize=None)
def mk_picture(H, W):
    """a picture with gradients in every direction and unusable pixels in most cells: the 3 x 3 box mean of uniform noise on a ramp,
    one channel of every fiftieth pixel or so at 1.0"""
    rng = np.random.default_rng(9000 + 3 * H + W)
    base = rng.random((H + 2, W + 2, 3))
    box = sum(base[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    ramp = 0.25 * (np.arange(W)[None, :, None] / float(W) + np.arange(H)[:, None, None] / float(H))
    pic = (0.5 * box + ramp).astype(np.float32)
    salt = rng.random((H, W)) < 0.02
    pic[salt, rng.integers(0, 3, int(salt.sum()))] = 1.0
    pic.setflags(write=False)
    return pic


@functools.lru_cache(maxsize=None)
def patch_picture():
    """a frame with a NaN, an inf and a patch at 1.0"""
    H, W, _ = PATCH_CASE
    pic = np.array(mk_picture(H, W))
    pic[pic == 1.0] = 0.5
    pic[21, 37, 0], pic[70, 90, 2] = np.nan, -np.inf
    pic[40:53, 18:30] = 1.0
    pic.setflags(write=False)
    return pic


def frames():
    """(picture, region, size) of every comparison with the oracle in this file"""
    out = [(mk_picture(H, W), (0, H, 0, W), size) for H, W, size, _ in SHAPES]
    (H, W), region, size = WALL_CASE
    out.append((mk_picture(H, W), region, size))
    H, W, size = POOL_CASE
    out.append((mk_picture(H, W), (0, H, 0, W), size))
    H, W, size = PATCH_CASE
    out.append((patch_picture(), (0, H, 0, W), size))
    return out


@functools.lru_cache(maxsize=None)
def oracle(H, W, region, size):
    return mr.scores(mk_picture(H, W), region, size, CLIP, np.float64)


def measure_f32_restatement():
    """worst |float32 restatement - float64 oracle| / trace over the candidates and frames of this file (CPU only), scores and traces"""
    worst = 0.0
    for pic, region, size in frames():
        o, r = mr.scores(pic, region, size, CLIP, np.float64), mr.scores(pic, region, size, CLIP, np.float32)
        assert o[2].tolist() == r[2].tolist()
        live = o[1] > 0
        for a64, a32 in zip(o[:2], r[:2]):
            worst = max(worst, float((np.abs(a32 - a64)[live] / o[1][live]).max()))
    return worst


# Measured on the CPU by `python tests/test_gpu_mask.py`, without the code under test.
F32_RESTATEMENT_ERROR = 8.133e-07     # (the one-cell boxes of 1360 x 1360; 4.518e-07 over the other frames)


def gate():
    g = 4 * F32_RESTATEMENT_ERROR
    # a luma carries three roundings at values <= 1 (2^-24 each), so a difference d is off by some 1e-7 and its square by 2e-7 / |d| of
    # itself: 1e-5 at |d| = 0.02; the sum over the 256 pixels of a cell brings that down by 16, more cells by more
    assert 0 < g <= 1e-5
    return g


def check(got, ref, region, size, what):
    """a WindowScores with its map against the oracle's (score, trace, clipped) maps"""
    score, trace, bad = ref
    g = gate()
    assert got.map is not None and got.map.dtype == np.float64 and got.map.shape == score.shape, what
    err = np.abs(got.map - score)
    print("mask %s: %d x %d candidates, worst score error %.3e of the trace, gate %.3e" % (what, score.shape[0], score.shape[1], float((err / np.maximum(trace, 1e-300)).max()), g))
    assert (err <= g * trace).all(), (what, float((err - g * trace).max()))
    i, j = np.unravel_index(int(np.argmax(score)), score.shape)
    if score.size > 1:                                     # a condition on the frame: rounding cannot flip the choice
        flat = np.sort(score.ravel())
        assert flat[-1] - flat[-2] >= 2 * g * trace[i, j], (what, flat[-1] - flat[-2], g * trace[i, j])
    assert (got.box_y, got.box_x) == (region[0] + mr.CELL * i, region[2] + mr.CELL * j), what
    assert got.score == got.map[i, j] and abs(got.trace - trace[i, j]) <= g * trace[i, j], what
    assert got.clipped == bad[i, j] and isinstance(got.clipped, int), what


def same(a, b):
    """two WindowScores bit for bit"""
    if (a.map is None) != (b.map is None) or (a.map is not None and not np.array_equal(a.map.view(np.uint64), b.map.view(np.uint64))):
        return False
    return a[:2] == b[:2] and np.array_equal(np.array(a[2:4]).view(np.uint64), np.array(b[2:4]).view(np.uint64)) and a.clipped == b.clipped


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,size,max_wgs", SHAPES)
def test_scores_against_the_oracle(ctx, debug_switch, H, W, size, max_wgs):
    from lib._native import DeviceImage, WindowScores
    if max_wgs:
        debug_switch("max_wgs", max_wgs)
    pic = mk_picture(H, W)
    img = DeviceImage.from_host(pic, ctx)
    got = img.window_scores(size, scores=True)
    assert isinstance(got, WindowScores) and ctx.last_kernel_ms() > 0.0
    check(got, oracle(H, W, (0, H, 0, W), size), (0, H, 0, W), size, "%d x %d box %d wgs %d" % (H, W, size, max_wgs))
    assert same(img.window_scores(size, (0, H, 0, W), CLIP, scores=True), got)       # the arguments spelled out, and a second run: identical bits
    plain = img.window_scores(size)
    assert plain.map is None and same(plain._replace(map=got.map), got)
    assert np.array_equal(img.to_host(), pic)                                        # the source is never written


@pytest.mark.gpu
def test_the_capped_grid_returns_the_bits_of_the_full_one(ctx, debug_switch):
    from lib._native import DeviceImage
    img = DeviceImage.from_host(mk_picture(301, 287), ctx)
    full = img.window_scores(63, scores=True)
    debug_switch("max_wgs", 2)
    assert same(img.window_scores(63, scores=True), full)                            # the sums are per cell: who walks the tiles does not matter
    debug_switch("max_wgs", 1)
    assert same(img.window_scores(63, scores=True), full)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [None] + list(tm.PICK_CASES))
def test_the_pick_takes_the_first_of_equal_maxima_in_both_loop_forms(ctx, name):
    """7225 candidates (tests/test_mask.py pick_picture): the pick's lanes 0 .. 56 compare eight candidates in one unrolled trip, the
    others seven in the tail.  A unique maximum in either form, exact ties across the two, and the picture on which every candidate
    ties.  The choice must be the first occurrence of the maximum in the device's own map: exact, whatever the rounding of a score."""
    from lib._native import DeviceImage
    raised = tm.PICK_CASES[name] if name else ()
    img = DeviceImage.from_host(tm.pick_picture(raised), ctx)
    try:
        got = img.window_scores(16, scores=True)
    finally:
        img.close()
    assert got.map.shape == (tm.PICK_N, tm.PICK_N) and 7 * 1024 < got.map.size < 8 * 1024
    flat = got.map.ravel()
    top = np.flatnonzero(flat == flat.max())
    first = int(np.argmax(flat))
    print("mask pick %s: maxima at candidates %s, chosen (%d, %d)" % (name or "every candidate equal", top.tolist() if top.size < 9 else "all %d" % top.size, got.box_y, got.box_x))
    assert top.tolist() == (sorted(raised) if raised else list(range(flat.size)))              # the picture's ties are exact on the device too
    assert first == (min(raised) if raised else 0)
    assert (got.box_y, got.box_x) == (16 * (first // tm.PICK_N), 16 * (first % tm.PICK_N)) and got.score == flat[first] and got.clipped == 0


@pytest.mark.gpu
def test_region_with_an_odd_origin_sees_nothing_outside_it(ctx):
    from lib._native import DeviceImage
    (H, W), region, size = WALL_CASE
    y0, y1, x0, x1 = region
    pic = mk_picture(H, W)
    crop = DeviceImage.from_host(np.ascontiguousarray(pic[y0:y1, x0:x1]), ctx).window_scores(size, scores=True)
    crop = crop._replace(box_y=crop.box_y + y0, box_x=crop.box_x + x0)
    walled = np.full((H, W, 3), np.float32(1e30), np.float32)                         # unusable: a read past the region shows in the count ...
    walled[y0:y1, x0:x1] = pic[y0:y1, x0:x1]
    noisy = np.random.default_rng(3).random((H, W, 3)).astype(np.float32) * 0.9       # ... usable: it shows in the sums
    noisy[y0:y1, x0:x1] = pic[y0:y1, x0:x1]
    for name, frame in (("wall", walled), ("noise", noisy), ("itself", pic)):
        got = DeviceImage.from_host(frame, ctx).window_scores(size, region, scores=True)
        assert same(got, crop), name                                                 # bit for bit the cropped frame's
    check(got, oracle(H, W, region, size), region, size, "region %s of %d x %d box %d" % (region, H, W, size))
    # the count is seen where a box is made to cover the region's last row and column: a one-candidate region
    edge = (y1 - 16, y1, x1 - 16, x1)
    got = DeviceImage.from_host(walled, ctx).window_scores(16, edge)
    assert got.clipped == mr.choice(pic, edge, 16, CLIP)[4] and (got.box_y, got.box_x) == (y1 - 16, x1 - 16)


@pytest.mark.gpu
def test_unusable_pixels_are_counted_and_left_out(ctx):
    from lib._native import DeviceImage
    H, W, size = PATCH_CASE
    pic = patch_picture()
    img = DeviceImage.from_host(pic, ctx)
    ref = mr.scores(pic, (0, H, 0, W), size, CLIP)
    assert ref[2].sum() == 2 + 13 * 12 and np.isfinite(ref[0]).all()
    got = img.window_scores(size, scores=True)
    check(got, ref, (0, H, 0, W), size, "NaN, inf and a patch at 1.0")
    assert np.isfinite(got.map).all() and np.isfinite([got.score, got.trace]).all()
    seen = 0
    for y in range(0, H, 16):                                                        # every cell as a region of its own: its count comes back
        for x in range(0, W, 16):
            one = img.window_scores(16, (y, y + 16, x, x + 16))
            want = mr.choice(pic, (y, y + 16, x, x + 16), 16, CLIP)
            assert one.clipped == want[4] and abs(one.score - want[2]) <= gate() * want[3] and abs(one.trace - want[3]) <= gate() * want[3], (y, x)
            seen += one.clipped
    assert seen == 2 + 13 * 12
    # clip = inf keeps the patch (flat: nothing to score) and still drops the NaN and the inf
    wide = img.window_scores(size, clip=np.inf, scores=True)
    ref = mr.scores(pic, (0, H, 0, W), size, np.inf)
    assert ref[2].sum() == 2 and np.isfinite(wide.map).all() and (np.abs(wide.map - ref[0]) <= gate() * ref[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", tm.SEEDS)
def test_best_mask_equals_the_oracle(ctx, seed):
    from lib import _native, utils
    for kind, clip in (("patch", 0.99), ("stripes", 0.99), ("checker", 0.99), ("checker", np.inf)):
        frame = tm.frame(seed, kind)
        want = mr.center(frame, tm.BOX, clip)
        img = _native.DeviceImage.from_host(frame, ctx)
        for got in (utils.best_mask(img, tm.BOX, clip), utils.best_mask(frame, tm.BOX, clip)):
            assert isinstance(got, utils.MaskChoice)
            print("seed %d %s clip %s: device [%d, %d] score %.4e clipped %.3f, oracle [%d, %d] score %.4e" % ((seed, kind, clip) + tuple(got[:3]) + (got.clipped,) + tuple(want[:3])))
            assert got[:2] == want[:2] and got.clipped == want[4]
            assert abs(got.score - want[2]) <= gate() * want[3] and abs(got.trace - want[3]) <= gate() * want[3]
        assert np.array_equal(img.to_host(), frame)
    sub = (16, 150, 30, 190)                                                         # a region, and a box of another size
    assert utils.best_mask(img, 33, np.inf, sub)[:2] == mr.center(frame, 33, np.inf, sub)[:2]


@pytest.mark.gpu
def test_the_c_entry_refuses_bad_arguments(ctx):
    from lib import _native
    H, W = 70, 200
    img = _native.DeviceImage.from_host(mk_picture(H, W), ctx)
    lib = _native.load()
    by, bx, sc, tr, bad = C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_longlong()
    out = (C.byref(by), C.byref(bx), C.byref(sc), C.byref(tr), C.byref(bad))
    grid = (C.c_double * 36)()                                                       # box 63: 1 x 9 candidates
    for args, word in (((None, 0, H, 0, W, 63, 0.99) + out + (None, 0, 0), b"src"),
                       ((img._h, 0, H, 0, W, 63, 0.99, None) + out[1:] + (None, 0, 0), b"output"),
                       ((img._h, 0, H, 0, W, 63, 0.99) + out[:4] + (None, None, 0, 0), b"output"),
                       ((img._h, 5, 5, 0, W, 16, 0.99) + out + (None, 0, 0), b"region"),
                       ((img._h, 0, H + 1, 0, W, 63, 0.99) + out + (None, 0, 0), b"region"),
                       ((img._h, 0, H, -1, W, 63, 0.99) + out + (None, 0, 0), b"region"),
                       ((img._h, 0, H, 90, 30, 16, 0.99) + out + (None, 0, 0), b"region"),
                       ((img._h, 0, H, 0, W, 15, 0.99) + out + (None, 0, 0), b"size"),
                       ((img._h, 0, H, 0, W, -63, 0.99) + out + (None, 0, 0), b"size"),
                       ((img._h, 0, H, 0, W, 71, 0.99) + out + (None, 0, 0), b"region"),
                       ((img._h, 0, H, 0, 62, 63, 0.99) + out + (None, 0, 0), b"size"),
                       ((img._h, 0, H, 0, W, 63, 0.0) + out + (None, 0, 0), b"clip"),
                       ((img._h, 0, H, 0, W, 63, -0.5) + out + (None, 0, 0), b"clip"),
                       ((img._h, 0, H, 0, W, 63, float("nan")) + out + (None, 0, 0), b"clip"),
                       ((img._h, 0, H, 0, W, 63, 0.99) + out + (grid, 9, 1), b"map"),
                       ((img._h, 0, H, 0, W, 63, 0.99) + out + (grid, 1, 8), b"map"),
                       ((img._h, 0, H, 0, W, 63, 0.99) + out + (grid, 0, 0), b"map")):
        assert lib.ics_img_window_scores(*args) == _native.ICS_EINVAL, word
        assert word in lib.ics_last_error(), (word, lib.ics_last_error())
    assert lib.ics_img_window_scores(*((img._h, 0, H, 0, W, 63, 0.99) + out + (grid, 1, 9))) == _native.ICS_OK
    ref = oracle(H, W, (0, H, 0, W), 63)
    assert by.value == 0 and bx.value == 16 * int(np.argmax(ref[0])) and sc.value == grid[bx.value // 16] and bad.value == ref[2][0, bx.value // 16]
    assert lib.ics_img_window_scores(*((img._h, 0, H, 0, W, 63, float("inf")) + out + (None, 0, 0))) == _native.ICS_OK and bad.value == 0
    with pytest.raises(ValueError, match="size"):
        img.window_scores(15)
    with pytest.raises(ValueError, match="region"):
        img.window_scores(63, (0, H + 1, 0, W))
    with pytest.raises(ValueError, match="clip"):
        img.window_scores(63, clip=0)


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [True, False])
def test_deblur_module_auto_equals_the_explicit_mask(capsys, resident):
    import deconvolve as dv
    seed = tm.SEEDS[0]
    frame = tm.frame(seed, "patch")
    i, j = mr.choice(frame, (0, tm.H, 0, tm.W), tm.BOX, 0.99)[:2]
    center = [1 + 16 * i + tm.BOX // 2, 1 + 16 * j + tm.BOX // 2]                    # in the frame the driver pads by a pixel
    pic = (np.clip(frame, 0.0, 1.0).astype(np.float64) ** 2.2 * 255.0).astype(np.float32)     # deblur_module encodes it back: frame up to rounding
    kw = dict(pyramid=False, iterations=1, save=False, display=False, mask_size=tm.BOX, device_resident=resident)
    auto, psf_auto = dv.deblur_module(pic, "a", ".", 9, mask="auto", **kw)
    printed = capsys.readouterr().out
    lines = [ln for ln in printed.splitlines() if ln.startswith("Mask : ")]
    assert len(lines) == 1 and lines[0].startswith("Mask : [%d, %d] (score " % tuple(center)) and lines[0].endswith(" %)") and ", clipped 0.0 %" in lines[0], printed
    assert printed.index("Mask : ") < printed.index("Mask size :")
    given, psf_given = dv.deblur_module(pic, "a", ".", 9, mask=center, **kw)
    assert "Mask : " not in capsys.readouterr().out
    assert psf_auto.shape == (9, 9, 3) and auto.shape == (tm.H, tm.W, 3)
    assert auto.dtype == given.dtype and auto.tobytes() == given.tobytes()           # bit for bit
    assert np.asarray(psf_auto).tobytes() == np.asarray(psf_given).tobytes()
    other, _ = dv.deblur_module(pic, "a", ".", 9, mask=("auto", 0.9), **kw)          # the other form
    assert "Mask : [" in capsys.readouterr().out and other.shape == auto.shape
    both, psf_both = dv.deblur_module(pic, "a", ".", "auto", mask="auto", **kw)      # nothing read off the picture by the user
    printed = capsys.readouterr().out
    assert printed.count("Mask : [%d, %d] (score " % tuple(center)) == 1 and printed.count("Blur width : ") == 1
    assert printed.index("Mask : ") < printed.index("Blur width : ") and both.shape == auto.shape
    with pytest.raises(ValueError, match="outside the picture boundaries"):
        dv.deblur_module(pic, "a", ".", 9, mask="auto", **dict(kw, mask_size=161))


@pytest.mark.gpu
def test_scores_on_poisoned_pool_blocks(ctx, debug_switch):
    """the pool in check mode, switched as tests/test_gpu_pool_check.py switches it: the cell table, the candidate table and the
    result block come filled with 0xFF (NaN) or 0x7F (3.4e38); every entry is written before it is read, nothing is stored past a block"""
    import test_gpu_pool_check as pc
    from lib import _native
    ok, seen = pc.selftest()
    assert ok, seen
    H, W, size = POOL_CASE
    pic = mk_picture(H, W)

    def run():
        img = _native.DeviceImage.from_host(pic, ctx)
        try:
            return img.window_scores(size, scores=True)
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
        assert same(got, ref), "fill %#x changes the scores" % byte
    debug_switch("pool_check", -1)
    pc.quiesce()
    ctx.conv2d_symm(np.zeros((2, 2)), np.ones((1, 1)))                         # returns the context's last check-mode scratch block to the pool
    assert pc.overruns() == 0
    check(ref, oracle(H, W, (0, H, 0, W), size), (0, H, 0, W), size, "%d x %d box %d" % (H, W, size))


if __name__ == "__main__":
    print("%.3e" % measure_f32_restatement())
