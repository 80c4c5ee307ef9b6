"""CPU: the float64 oracle and the float32 restatement of tests/blur_map_ref.py (the specification of csrc/ics_img_blurmap.hip), the
host rules of lib._native against it, and the argument handling of DeviceImage.blur_map, lib.utils.blur_map, best_mask(blur=...) and
deblur_module(mask=("auto", clip, (lo, hi))).

Test frames: analytic steps 0.2 + 0.6 Phi(d / sigma), and the "dead leaves" of tests/test_blur_width.py with the left half of the
frame blurred by a Gaussian of 1 and the right half by one of 3 (two blurred copies of one canvas, cut at the middle column), noise 0.01.

float32 against float64: the worst |sigma32 - sigma64| on the common kept pixels of the half-and-half frames is printed by
`python tests/test_blur_map.py` and recorded below as F32_RESTATEMENT_ERROR (a measurement of the specification, nothing is gated on it:
the device is held to the float32 restatement's bits in tests/test_gpu_blur_map.py)."""
import functools
import math
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests"), os.path.join(root, "image-cases-studies_amd")]
import blur_map_ref as bm
import test_blur_width as tb

H, W = tb.H, tb.W                      # 160 x 192
SEEDS = tb.SEEDS
LEFT, RIGHT = (0.8, 1.4), (2.3, 3.3)   # where the median cell reading of a half must lie (true sigma 1 and 3)
# Measured on the CPU by `python tests/test_blur_map.py`: worst |sigma32 - sigma64| over the common kept pixels of halves(seed), SEEDS.
F32_RESTATEMENT_ERROR = 2.968e-04


def gauss(s):
    r = int(math.ceil(4 * s))
    i = np.arange(-r, r + 1)
    g = np.exp(-i * i / (2.0 * s * s))
    return g / g.sum()


@functools.lru_cache(maxsize=None)
def halves(seed, left=1.0, right=3.0, noise=0.01):
    """the canvas of test_blur_width.dead_leaves, its left half blurred by a Gaussian of `left`, its right half by one of `right`"""
    rng = np.random.default_rng(seed)
    m = 24
    Hc, Wc = H + 2 * m, W + 2 * m
    c = np.full((Hc, Wc, 3), 0.5)
    for _ in range(300):
        h, ww = rng.integers(6, H // 3 + 1, 2)
        y, x = rng.integers(-h + 1, Hc), rng.integers(-ww + 1, Wc)
        c[max(y, 0):y + h, max(x, 0):x + ww] = rng.uniform(0.05, 0.95, 3)
    F = np.fft.fft2(c, axes=(0, 1))

    def blurred(s):
        g = gauss(s)
        ky, kx = np.zeros(Hc), np.zeros(Wc)
        ky[:g.size] = g
        kx[:g.size] = g
        K = np.fft.fft(np.roll(ky, -(g.size // 2)))[:, None] * np.fft.fft(np.roll(kx, -(g.size // 2)))[None, :]
        return np.real(np.fft.ifft2(F * K[..., None], axes=(0, 1)))[m:-m, m:-m]
    out = np.concatenate((blurred(left)[:, :W // 2], blurred(right)[:, W // 2:]), axis=1)
    out = (out + rng.normal(0.0, noise, (H, W, 3))).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(seed, dtype_name):
    return bm.blur_map(halves(seed), dtype=np.dtype(dtype_name).type)


def step(sigma, deg, h=64, w=96):
    y, x = np.mgrid[:h, :w].astype(np.float64)
    t = math.radians(deg)
    d = (x - (w - 1) / 2.0) * math.cos(t) + (y - (h - 1) / 2.0) * math.sin(t)
    phi = 0.5 * (1.0 + np.vectorize(math.erf)(d / (sigma * math.sqrt(2.0))))
    return np.repeat((0.2 + 0.6 * phi)[..., None], 3, axis=2).astype(np.float32)


@pytest.mark.parametrize("deg", [0, 30, 45, 90])
@pytest.mark.parametrize("sigma", [2, 3, 4, 5, 6])
def test_oracle_reads_analytic_edges(sigma, deg):
    _, sg, kept, _ = bm.pixels(step(sigma, deg), edge=0.01)
    inner = np.zeros_like(kept)
    inner[12:-12, 12:-12] = kept[12:-12, 12:-12]
    assert inner.sum() >= 30, inner.sum()
    err = float(np.abs(sg[inner] - sigma).max())
    print("step sigma %d at %d deg: %d edge pixels, worst error %.3f" % (sigma, deg, inner.sum(), err))
    assert err <= 0.2, (sigma, deg, err)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_on_half_and_half_dead_leaves(seed):
    r = reference(seed, "float64")
    cs = bm.cell_sigma(r["weight"], r["moment"], r["count"])
    assert cs.shape == (H // 16, W // 16) and r["bad"] == 0
    left, right = float(np.nanmedian(cs[:, :W // 32])), float(np.nanmedian(cs[:, W // 32:]))
    print("seed %d: median cell sigma left %.3f, right %.3f, %d edge pixels" % (seed, left, right, r["kept"].sum()))
    assert LEFT[0] <= left <= LEFT[1] and RIGHT[0] <= right <= RIGHT[1], (seed, left, right)
    # the cell rules: moment / weight lies between the cell's smallest and largest reading, count is the number of readings
    k = r["kept"][:16, :16]
    if k.any():
        assert r["count"][0, 0] == k.sum() and r["pixels"][:16, :16][k].min() - 1e-12 <= cs[0, 0] <= r["pixels"][:16, :16][k].max() + 1e-12
    assert (r["pixels"][~r["kept"]] == -1).all() and (r["pixels"][r["kept"]] >= 0).all()


def f32_against_f64(seed):
    a, b = reference(seed, "float64"), reference(seed, "float32")
    common = a["kept"] & b["kept"]
    return int((a["kept"] != b["kept"]).sum()), int(a["kept"].sum()), float(np.abs(a["pixels"][common] - b["pixels"][common].astype(np.float64)).max())


@pytest.mark.parametrize("seed", SEEDS)
def test_float32_restatement_keeps_the_oracles_pixels(seed):
    """a condition on the inputs, asserted on the reference alone: no decision of the rule is close on these frames"""
    differ, kept, err = f32_against_f64(seed)
    print("seed %d: kept sets differ in %d of %d pixels, worst |sigma32 - sigma64| %.3e" % (seed, differ, kept, err))
    assert differ <= 0.005 * kept, (seed, differ, kept)
    assert reference(seed, "float32")["weight"].dtype == np.float32


def test_sharp_frame_reads_below_one_and_the_window_is_the_cropped_frame():
    pic = tb.dead_leaves(SEEDS[0], H, W)
    r = bm.blur_map(pic)
    med = float(np.nanmedian(bm.cell_sigma(r["weight"], r["moment"], r["count"])))
    print("sharp frame: median cell sigma %.3f" % med)
    assert 0.4 <= med <= 0.8, med
    window = (13, 150, 7, 180)
    a, b = bm.blur_map(pic, window=window, dtype=np.float32), bm.blur_map(np.ascontiguousarray(pic[13:150, 7:180]), dtype=np.float32)
    assert all(np.array_equal(a[k], b[k]) for k in ("weight", "moment", "count", "pixels"))
    nan = np.array(pic)
    nan[40, 50, 1] = np.nan
    assert bm.blur_map(nan, dtype=np.float32)["bad"] == 1 and bm.blur_map(nan, window=(60, 160, 0, 192), dtype=np.float32)["bad"] == 0


def test_host_rules_against_the_specification():
    from lib import _native
    assert _native.IMG_BLURMAP_CELL == bm.CELL == _native.IMG_MASK_CELL and _native.IMG_BLURMAP_MAX_RADIUS == bm.MAX_RADIUS
    for s in (0.5, 1.0, 1.5, 2.0, 8 / 3, 0.7):
        g = _native.blur_map_taps(s)
        assert g.dtype == np.float32 and g.size == 2 * bm.radius(s) + 1 and np.array_equal(g, bm.taps(s, np.float32))
        assert np.array_equal(g, g[::-1]) and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-6
    assert bm.radius(8 / 3) == 8 and bm.radius(2.0) == 6 and bm.radius(1.0) == 3
    for sn, sa, k in ((0.01, 1.0, 5.0), (0.002, 1.5, 3.0), (0.0, 1.0, 5.0)):
        assert _native.blur_map_edge(sn, sa, k) == bm.edge_from_noise(sn, sa, k)
    # white noise through the two passes and the central difference: the formula against a simulation
    rng = np.random.default_rng(5)
    noise = rng.normal(0.0, 0.01, (256, 256, 3)).astype(np.float32)
    S = bm._smooth(bm.luma(noise, np.float64), bm.taps(1.0), np.float64)
    gx = 0.5 * (S[20:-20, 21:-19] - S[20:-20, 19:-21])
    assert abs(float(gx.std()) / bm.edge_from_noise(0.01, 1.0, 1.0) - 1.0) < 0.05
    r = reference(SEEDS[0], "float32")
    sigma = bm.cell_sigma(r["weight"], r["moment"], r["count"])
    got = _native.BlurMap(sigma, r["weight"], r["count"])
    assert got.pixels is None
    # fill: a grid with holes, one of them two rings from any reading
    holed, weight = sigma.copy(), r["weight"].copy()
    holed[2:7, 3:8] = np.nan
    holed[0, 0] = np.nan
    want = bm.filled(holed, weight)
    assert np.array_equal(_native.blur_map_fill(_native.BlurMap(holed, weight, r["count"])), want) and not np.isnan(want).any()
    assert np.array_equal(want[~np.isnan(holed)], holed[~np.isnan(holed)])
    ring = [(1, 2), (1, 3), (1, 4), (2, 2), (3, 2)]                           # the cells at distance 1 of (2, 3) that hold a reading
    assert abs(want[2, 3] - sum(float(weight[c]) * holed[c] for c in ring) / sum(float(weight[c]) for c in ring)) < 1e-12
    assert np.isnan(_native.blur_map_fill(_native.BlurMap(np.full((3, 4), np.nan), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.int32)))).all()
    # box_sigma: the candidate grid is window_scores'
    for side, extent in ((63, (H, W)), (48, (H, W)), (63, (H - 2, W - 2)), (129, (150, 171))):
        rr = bm.blur_map(halves(SEEDS[0])[:extent[0], :extent[1]], dtype=np.float32)
        sg = bm.cell_sigma(rr["weight"], rr["moment"], rr["count"])
        box = _native.blur_map_box_sigma(_native.BlurMap(sg, rr["weight"], rr["count"]), side, extent)
        assert np.array_equal(box, bm.box_sigma(sg, rr["weight"], rr["count"], side, extent), equal_nan=True)
        size, (y0, y1, x0, x1), _ = _native.window_scores_args(side, None, 0.99, extent)
        assert box.shape == ((y1 - y0 - size) // 16 + 1, (x1 - x0 - size) // 16 + 1)
    empty = _native.BlurMap(np.full((10, 12), np.nan), np.zeros((10, 12), np.float32), np.zeros((10, 12), np.int32))
    assert np.isnan(_native.blur_map_box_sigma(empty, 63, (H, W))).all()
    with pytest.raises(ValueError, match="do not lie"):
        _native.blur_map_box_sigma(empty, 63, (H + 40, W))


def test_argument_refusals_without_a_device(capsys):
    import deconvolve as dv
    from lib import _native, utils
    shape = (40, 50, 3)
    pic = np.zeros(shape, np.float32)
    assert _native.blur_map_args((1.0, 2.0), 0.02, 8.0, None, shape) == ((1.0, 2.0), float(np.float32(0.02)), 8.0, (0, 40, 0, 50))
    assert _native.blur_map_args((1, 8 / 3), 1, 1, (1, 2, 3, 4), shape)[0][1] == float(np.float32(8 / 3))
    for bad in ((0.4, 2.0), (2.0, 2.0), (2.0, 1.0), (1.0, 2.7), (1.0,), (1.0, 2.0, 3.0), "ab", None, (1.0, math.nan), (1.0, "2"), (True, 2.0)):
        with pytest.raises(ValueError, match="sigmas"):
            _native.blur_map_args(bad, 0.02, 8.0, None, shape)
        with pytest.raises(ValueError, match="sigmas"):
            utils.blur_map(pic, bad)
    for bad in (0, -1.0, math.nan, math.inf, None, "x", True):
        with pytest.raises(ValueError, match="edge"):
            _native.blur_map_args((1.0, 2.0), bad, 8.0, None, shape)
        with pytest.raises(ValueError, match="max_sigma"):
            _native.blur_map_args((1.0, 2.0), 0.02, bad, None, shape)
    for bad in ("automatic", ("auto",), ("auto", -1), ("auto", math.nan), ("manual", 3), ("auto", 5, 1)):
        with pytest.raises(ValueError, match="edge|strength"):
            utils.blur_map(pic, edge=bad)
    for window in ((0, 0, 0, 50), (0, 41, 0, 50), (-1, 40, 0, 50), (0, 40, 10, 10), (0, 40), "all", (0.5, 40, 0, 50)):
        with pytest.raises(ValueError, match="window"):
            utils.blur_map(pic, window=window)
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.blur_map(np.zeros((8, 9)))
    for bad in ((3.0, 2.0), (-1.0, 2.0), (1.0,), (1.0, 2.0, 3.0), "ab", 2.0, (1.0, math.inf), (math.nan, 2.0), (1.0, "2"), (True, 2.0)):
        with pytest.raises(ValueError, match="blur"):
            utils.best_mask(pic, 31, blur=bad)
        with pytest.raises(ValueError, match="mask: blur"):
            dv._mask_args(("auto", 0.99, bad))
    assert utils.mask_blur_args((2, 3.5)) == (2.0, 3.5) and utils.mask_blur_args([0, 0]) == (0.0, 0.0)
    with pytest.raises(ValueError, match="mask_size"):
        utils.best_mask(pic, 9, blur=(1.0, 2.0))                           # the checks of the plain form stay in front of the device
    with pytest.raises(ValueError, match="smaller than the box"):
        utils.best_mask(pic, 63, blur=(1.0, 2.0))
    assert utils.MaskChoice._fields == ("center_y", "center_x", "score", "trace", "clipped")
    assert utils.MaskChoiceBlur._fields == utils.MaskChoice._fields + ("sigma",)
    # deblur_module's forms: the old ones return what they returned, the new one its pair; bad ones are refused before anything is uploaded
    assert dv._mask_args(None) is None and dv._mask_args([3, 4]) is None and dv._mask_args("auto") == 0.99
    assert dv._mask_args(("auto", 0.5)) == 0.5 and dv._mask_args(("auto", 0.5, (2.3, 3.3))) == (0.5, (2.3, 3.3))
    u8 = np.zeros((40, 50, 3), np.uint8)

    def solver(*a, **k):
        raise AssertionError("the solver must not run")
    for resident in (True, False):
        for bad in (("auto", 0.99, (3.0, 2.0)), ("auto", 0.99, 2.0), ("auto", 0.0, (2.0, 3.0)), ("auto", 0.99, (2.0, 3.0), 1), ("box", 0.99, (2.0, 3.0))):
            with pytest.raises(ValueError, match="mask"):
                dv.deblur_module(u8, "x", ".", 5, mask=bad, save=False, display=False, solver=solver, device_resident=resident)
    assert "Mask :" not in capsys.readouterr().out


if __name__ == "__main__":
    print("%.3e" % max(f32_against_f64(seed)[2] for seed in SEEDS))
