"""CPU: the blur-width rule and the float64 oracle of tests/blur_width_ref.py (the specification of csrc/ics_img_blurwidth.hip and of
lib._native.blur_extent / blur_width_from), the host rule of the package against it, and the argument handling of
lib.utils.estimate_blur_width and deblur_module(blur_width="auto").  The last test runs the estimate and is marked gpu.

Test frames: "dead leaves" -- 300 axis-aligned rectangles painted over each other on a grey canvas, blurred by a circular FFT
convolution on a canvas 24 px larger on every side, the margin cut off, Gaussian noise of 0.01 added: sharp edges at every
orientation-free position, which is what the method assumes of the picture under the blur.  The seeds are chosen so that the float64
oracle ALONE meets what is asserted below (a condition on the inputs, re-checked here), and so that no decision of the rule is close:
no fitted extent within 0.05 px of an odd integer, no compared lag within 2e-3 P of its threshold -- float32 cannot flip the answer."""
import functools

import numpy as np
import pytest

import blur_width_ref as br

H, W, L = 160, 192, 40
SEEDS = (100, 109, 112, 113)        # of 100 .. 134, the first four that meet the conditions of test_oracle_on_dead_leaves
# (kind, size of the blur, the widths that count as right): exact for the sharp frame and the boxes of 5 and 9, one odd step for the rest
CASES = (("sharp", 1, (3,)), ("box", 5, (5,)), ("box", 9, (9,)), ("box", 15, (13, 15, 17)), ("disc", 15, (13, 15, 17)), ("hline", 11, (9, 11, 13)))


def blur_kernel(kind, w):
    if kind == "sharp":
        k = np.ones((1, 1))
    elif kind == "box":
        k = np.ones((w, w))
    elif kind == "disc":
        r = (w - 1) / 2.0
        y, x = np.mgrid[:w, :w] - r
        k = (x * x + y * y <= (r + 0.25) ** 2).astype(np.float64)
    elif kind == "hline":
        k = np.ones((1, w))
    else:
        raise ValueError(kind)
    return k / k.sum()


@functools.lru_cache(maxsize=None)
def dead_leaves(seed, H, W, kind="sharp", w=1):
    rng = np.random.default_rng(seed)
    m = 24
    Hc, Wc = H + 2 * m, W + 2 * m
    c = np.full((Hc, Wc, 3), 0.5)
    for _ in range(300):
        h, ww = rng.integers(6, H // 3 + 1, 2)
        y, x = rng.integers(-h + 1, Hc), rng.integers(-ww + 1, Wc)
        c[max(y, 0):y + h, max(x, 0):x + ww] = rng.uniform(0.05, 0.95, 3)
    k = blur_kernel(kind, w)
    pad = np.zeros((Hc, Wc))
    pad[:k.shape[0], :k.shape[1]] = k
    K = np.fft.rfft2(np.roll(pad, (-(k.shape[0] // 2), -(k.shape[1] // 2)), (0, 1)))
    c = np.stack([np.fft.irfft2(np.fft.rfft2(c[..., i]) * K, (Hc, Wc)) for i in range(3)], axis=2)
    out = (c[m:-m, m:-m] + rng.normal(0.0, 0.01, (H, W, 3))).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(seed, kind, w):
    """(width, extent_x, extent_y, Ax, Ay) of the float64 oracle on the whole frame, computed once"""
    Ax, Ay, _, _ = br.profiles(dead_leaves(seed, H, W, kind, w), (0, H, 0, W), L, np.float64)
    return br.blur_width(Ax, Ay), br.extent(Ax), br.extent(Ay), Ax, Ay


def margin(A):
    """the smallest distance, in units of P, between a lag the rule compares and the threshold it is compared with"""
    A = np.asarray(A, dtype=np.float64)
    P = A[2] + 2.0 * (A[2] - A[3])
    if not P > 0:
        return abs(P) / abs(A[0])
    m, h = [1.0], 1
    while h + 1 <= A.size - 1:
        m.append(abs(A[h + 1] - 0.5 * P) / P)
        if not A[h + 1] >= 0.5 * P:
            break
        h += 1
    if h < 3:
        for l in range(2, A.size):
            m.append(abs(A[l] - 0.05 * P) / P)
            if A[l] <= 0.05 * P:
                break
    return min(m)


def triangle(w, n, scale=3e-4):
    return scale * np.maximum(0.0, 1.0 - np.arange(n + 1) / float(w))


@pytest.mark.parametrize("rule", ["reference", "package"])
def test_rule_on_analytic_profiles(rule):
    if rule == "reference":
        extent, width, saturated = br.extent, br.blur_width, br.SATURATED
    else:
        from lib import _native
        extent, width, saturated = _native.blur_extent, _native.blur_width_from, _native.BLUR_SATURATED
    for w in (3, 5, 9, 64):
        A = triangle(w, 80)
        A[:2] += 1e-4                                    # white noise in the picture: lags 0 and 1 only, and the rule does not look there
        assert abs(extent(A) - w) < 1e-9, (w, extent(A))
        assert width(A, np.zeros(81)) == width(np.zeros(81), A) == (w if w % 2 else w + 1)
    assert extent(np.full(41, 2e-4)) == saturated        # never falls: half maximum everywhere, slope 0
    assert extent(triangle(64, 40)) == saturated         # falls, but crosses zero beyond the last lag
    assert extent(np.zeros(41)) == 1.0 and extent(-triangle(9, 40)) == 1.0       # flat: nothing correlates
    assert extent(triangle(9, 2)) == 1.0                 # fewer than 4 lags
    assert width(np.zeros(41), np.zeros(41)) == 3
    with pytest.raises(ValueError, match="saturated"):
        width(np.full(41, 2e-4), np.zeros(41))
    assert width(triangle(9.0000000005, 40), np.zeros(41)) == 9 and width(triangle(9.01, 40), np.zeros(41)) == 11      # the 1e-9 of the rounding
    if rule == "package":
        with pytest.raises(ValueError, match="not finite"):
            extent(np.array([1.0, np.nan, 0.5, 0.2, 0.0]))


def test_oracle_counts_and_definition():
    rng = np.random.default_rng(3)
    pic = rng.random((7, 9, 3))
    Ax, Ay, nx, ny = br.profiles(pic, (1, 6, 2, 9), 8)
    Y = pic[1:6, 2:9].sum(axis=2) / 3.0
    dx, dy = np.diff(Y, axis=1), np.diff(Y, axis=0)
    assert nx.tolist() == [5 * max(6 - l, 0) for l in range(9)] and ny.tolist() == [7 * max(4 - l, 0) for l in range(9)]
    for l in range(9):
        sx = sum(dx[y, x] * dx[y, x + l] for y in range(5) for x in range(6 - l))
        sy = sum(dy[y, x] * dy[y + l, x] for y in range(4 - l) for x in range(7))
        assert Ax[l] == pytest.approx(sx / nx[l] if nx[l] else 0.0, rel=1e-12, abs=1e-300)
        assert Ay[l] == pytest.approx(sy / ny[l] if ny[l] else 0.0, rel=1e-12, abs=1e-300)
    # the float32 restatement: same counts, profiles within float32 rounding of the oracle
    Bx, By, mx, my = br.profiles(pic, (1, 6, 2, 9), 8, np.float32)
    assert mx.tolist() == nx.tolist() and my.tolist() == ny.tolist() and Bx.dtype == By.dtype == np.float64
    assert np.abs(Bx - Ax).max() <= 1e-6 * Ax[0] and np.abs(By - Ay).max() <= 1e-6 * Ay[0]
    a = br.profiles(pic, (0, 1, 0, 1), 0)
    assert [v.tolist() for v in a] == [[0.0], [0.0], [0], [0]]
    for window in ((0, 0, 0, 9), (0, 8, 0, 9), (-1, 7, 0, 9), (3, 2, 0, 9)):
        with pytest.raises(ValueError, match="window"):
            br.profiles(pic, window, 4)
    with pytest.raises(ValueError, match="L ="):
        br.profiles(pic, (0, 7, 0, 9), 129)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_on_dead_leaves(seed):
    """what the seeds were chosen for, by the float64 oracle alone"""
    for kind, w, allowed in CASES:
        width, ex, ey, Ax, Ay = oracle(seed, kind, w)
        print("seed %d %s %d: width %d (x %.3f, y %.3f), margins %.2e %.2e" % (seed, kind, w, width, ex, ey, margin(Ax), margin(Ay)))
        assert width in allowed, (kind, w, width, ex, ey)
        if kind == "hline":
            assert ey < 3, ey
        for e in (ex, ey):
            if e != round(e):                            # a fitted extent: away from the odd integers, where the width changes
                assert abs(e - (2 * round((e - 1) / 2) + 1)) >= 0.05, (kind, w, e)
        assert min(margin(Ax), margin(Ay)) >= 2e-3, (kind, w, margin(Ax), margin(Ay))


def test_argument_validation_without_a_device():
    import deconvolve as dv
    from lib import _native, utils
    pic = np.zeros((40, 50, 3), np.float32)
    for bad in (2, 62, 1, 128, 129, 9.5, "9", None, True):
        with pytest.raises(ValueError, match="max_width"):
            utils.estimate_blur_width(pic, bad)
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.estimate_blur_width(np.zeros((8, 9)))
    for window in ((0, 0, 0, 50), (0, 41, 0, 50), (-1, 40, 0, 50), (0, 40, 10, 10), (0, 40), "all", (0.5, 40, 0, 50)):
        with pytest.raises(ValueError, match="window"):
            utils.estimate_blur_width(pic, 15, window)
    for bad in (-1, 129, 1.5, "4", None):
        with pytest.raises(ValueError, match="max_lag"):
            _native.blur_profile_args(bad, None, (40, 50, 3))
    assert _native.blur_profile_args(128, None, (40, 50, 3)) == (128, (0, 40, 0, 50)) and _native.IMG_BLURWIDTH_MAX_LAG == br.MAX_LAG
    assert dv._blur_width_args(9) is None and dv._blur_width_args("auto") == 63 and dv._blur_width_args(("auto", 15)) == 15
    # deblur_module: the reference's two errors stay for integers, the automatic forms are refused before anything is uploaded
    u8 = np.zeros((40, 50, 3), np.uint8)
    for resident in (True, False):
        with pytest.raises(ValueError, match="should be odd. You can use 5"):
            dv.deblur_module(u8, "x", ".", 4, save=False, display=False, device_resident=resident)
        with pytest.raises(ValueError, match="at least 3"):
            dv.deblur_module(u8, "x", ".", 1, save=False, display=False, device_resident=resident)
        for bad in (("auto", 2), ("auto", 64), ("auto", 129), ("auto",), ("auto", 9, 1), "automatic", ("width", 9)):
            with pytest.raises(ValueError, match="blur_width|max_width"):
                dv.deblur_module(u8, "x", ".", bad, save=False, display=False, device_resident=resident)


@pytest.mark.gpu
def test_deblur_module_auto_calls_the_solver_with_the_estimated_width(capsys):
    """blur_width="auto" on a box-9 frame: the printed line, and the solver sees MK = 9 at the last (only) level of both phases"""
    import deconvolve as dv
    seed = SEEDS[0]
    assert oracle(seed, "box", 9)[0] == 9
    frame = dead_leaves(seed, H, W, "box", 9)
    pic = (np.clip(frame, 0.0, 1.0).astype(np.float64) ** 2.2 * 255.0).astype(np.float32)     # deblur_module encodes it back: frame up to rounding
    calls = []

    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C, MK, iterations, step, lambd, **kw):
        calls.append((MK, psf.shape, bool(kw.get("blind"))))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]

    out, psf = dv.deblur_module(pic, "x", ".", "auto", mask_size=63, display=False, pyramid=False, solver=solver, save=False, iterations=1)
    printed = capsys.readouterr().out
    lines = [ln for ln in printed.splitlines() if ln.startswith("Blur width :")]
    assert len(lines) == 1 and lines[0].startswith("Blur width : 9 (x ") and lines[0].endswith(")"), printed
    assert calls == [(9, (9, 9, 3), True), (9, (9, 9, 3), False)], calls
    assert psf.shape == (9, 9, 3) and out.shape == (H, W, 3)
