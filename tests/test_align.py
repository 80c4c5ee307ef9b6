"""CPU: the specification of DeviceImage.align / align_sums / warp (tests/align_ref.py) does what it is for -- it leaves a registered
pair alone, copies pixels exactly under an identity or an integer shift, recovers known warps on dead-leaves pairs within the bounds
the feature was asked to meet, recovers a gain and a bias, refuses what it cannot align --, registration in front of the PSF estimate
repairs a misregistered pair, the float32 restatement stays within a quarter of every GPU gate, and the layers above the kernels
(argument checks, the plan, the C entries and the header) hold what include/ics_hip.h and lib/_native.py state.
tests/test_gpu_align.py gates the kernels against the specification."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_ref as ar
import psf_est_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_registered_pair_stays_at_the_identity():
    moving, fixed, _ = ar.pair("translation", 0)
    for model in ar.MODELS:
        for photometric in (True, False):
            res = ar.align(fixed, fixed, model, photometric)
            assert np.abs(res.matrix - np.eye(3)).max() <= 1e-9 and abs(res.gain - 1) <= 1e-9 and abs(res.bias) <= 1e-9, (model, photometric)
            assert res.levels == 2 and res.rms <= 1e-9


def test_warp_copies_pixels_exactly_under_the_identity_and_an_integer_shift():
    for dtype in (np.float64, np.float32):
        src = ar.warp_source((33, 65)).astype(dtype)
        assert np.array_equal(ar.warp(src, np.eye(3), dtype=dtype), src)
        out = ar.warp(src, ar.translation(3, -2), dtype=dtype)          # out[y][x] = src[y - 2][x + 3]
        assert np.array_equal(out[2:, :-3], src[:-2, 3:])
        big = ar.warp(src, ar.translation(-4, 5), (40, 80), dtype=dtype)  # another shape: out[y][x] = src[y + 5][x - 4]
        assert big.shape == (40, 80, 3) and np.array_equal(big[:28, 4:69], src[5:, :])
        assert np.array_equal(big[:28, 0], src[5:, 0]) and np.array_equal(big[39, 4:69], src[32])   # the edge repeats beyond the frame


@pytest.mark.parametrize("model,blur", ar.RECOVERY)
def test_known_warps_are_recovered(model, blur):
    """160 x 192 dead leaves as wiener_ref.dead_leaves draws them (hard edges, nothing smoothed), noise 0.002, moving sampled from the
    larger canvas by the cubic taps (blurred by a 9 px box first for blur = 9), corner motions of 13.6 px (translation), 11.9 px (affine,
    4 degrees, 3 %) and 6.7 px (homography); two levels.  Largest corner error measured, px: translation 0.0061 / 0.0363, affine 0.0236
    / 0.1876, homography 0.0363 / 0.3521 (sharp / blurred); bounds 0.1 / 0.2, 0.1 / 0.2, 0.1 / 0.5.  Without the binomial 1 2 1 on the
    lumas the affine pair under the box ends 0.2045 px off and misses its bound (0.0196 / 0.0341, 0.0083 / 0.2045, 0.0085 / 0.3503)."""
    moving, fixed, M = ar.pair(model, blur)
    res, per = ar.recovered(model, blur)
    start, err = ar.corner_error(np.eye(3), M, fixed.shape), ar.corner_error(res.matrix, M, fixed.shape)
    print("%s, box %d: corners start %.2f px off, end %.4f px off (bound %.2f); steps %s, gain %.4f, bias %.4f, rms %.4f, coverage %.2f" % (
        model, blur, start, err, ar.RECOVERY_BOUND[model, blur], per, res.gain, res.bias, res.rms, res.coverage))
    assert start <= 0.1 * max(fixed.shape[:2]) and start >= 5
    assert res.levels == 2 and len(per) == 2
    assert err <= ar.RECOVERY_BOUND[model, blur]


def test_a_gain_and_a_bias_are_recovered():
    """fixed = 1.3 moving + 0.05 on the smoothed canvas (ar.pair says why): measured gain 1.3048, bias 0.0482, corners 0.014 px off;
    without the photometric terms 0.85 px.  On the plain canvas, whose hard edges the cubic taps soften in `moving` alone: 1.310, 0.046"""
    moving, fixed, M = ar.pair("affine", 0, 1.3, 0.05, smooth=True)
    on, off = ar.align(moving, fixed, "affine"), ar.align(moving, fixed, "affine", photometric=False)
    e_on, e_off = ar.corner_error(on.matrix, M, fixed.shape), ar.corner_error(off.matrix, M, fixed.shape)
    print("gain %.4f, bias %.4f, corners %.4f px off; photometric=False: %.4f px off (rms %.4f against %.4f)" % (on.gain, on.bias, e_on, e_off, off.rms, on.rms))
    assert abs(on.gain / 1.3 - 1) <= 0.05 and abs(on.bias / 0.05 - 1) <= 0.05
    assert e_on <= 0.1 and e_off >= 10 * e_on and off.rms >= 10 * on.rms
    assert off.gain == 1.0 and off.bias == 0.0


def test_refusals():
    moving, fixed, _ = ar.pair("translation", 0)
    with pytest.raises(ValueError, match="do not overlap enough"):
        ar.align(moving, fixed, "affine", init=ar.translation(400, 0))             # disjoint
    with pytest.raises(ValueError, match="do not overlap enough"):
        ar.align(moving, fixed, "affine", init=ar.translation(0, 130))             # a fifth of the rows overlap
    for photometric in (True, False):
        with pytest.raises(ValueError, match="no texture to align on"):
            ar.align(np.full(moving.shape, 0.4, np.float32), fixed, "affine", photometric)
    for which in (0, 1):
        frames = [moving.copy(), fixed.copy()]
        frames[which][80, 90, 1] = np.nan
        with pytest.raises(ValueError, match="not finite: despeckle first"):
            ar.align(frames[0], frames[1], "translation")
    with pytest.raises(ValueError, match="16 px"):
        ar.align(moving, fixed, levels=5)                                          # 160 >> 4 = 10
    with pytest.raises(ValueError, match="16 px"):
        ar.align(moving[:15], fixed)


def test_registration_in_front_of_the_psf_estimate_repairs_a_misregistered_pair():
    """a 9 px box on 160 x 192, the sharp frame off by 1 degree and (2.3, -1.6) px.  The scene is that of ar.psf_pair(): dead leaves under the
    binomial 1 2 1, about the aperture of a pixel -- point-sampled hard edges are no picture a sensor gives, and resampling them twice
    (once to misregister, once to repair) softens them by more than the box estimate tolerates.  L1 to the true box, measured: from the
    registered pair 0.111, after align + warp 0.115 (corners 0.17 px off), from the misregistered pair as it is 0.600.  "Far off" is
    taken as twice the bound on the repaired estimate, four times the registered pair's distance."""
    K = 9
    sharp, blurred, off, M = ar.psf_pair(K)
    H, W = ar.PAIR_SHAPE
    k = np.ones((K, K, 3)) / K ** 2
    res = ar.align(off, blurred, "affine")
    back = ar.warp(off, res.matrix, (H, W))
    l1 = lambda est: max(np.abs(est[..., c] - k[..., c]).sum() for c in range(3))
    registered, repaired, left = l1(pr.estimate(blurred, sharp, K)), l1(pr.estimate(blurred, back, K)), l1(pr.estimate(blurred, off, K))
    print("L1 to the true box: registered %.4f, align + warp %.4f (corners %.3f px off), as it is %.4f" % (
        registered, repaired, ar.corner_error(res.matrix, M, (H, W)), left))
    assert repaired <= 2 * registered
    assert left >= 4 * registered


@pytest.mark.parametrize("case", range(len(ar.SUMS_CASES)))
def test_the_float32_sums_stay_within_a_quarter_of_the_gate(case):
    shape_f, shape_m, window = ar.SUMS_CASES[case]
    moving, fixed = ar.sums_pair(shape_f, shape_m)
    M = ar.sums_matrix(shape_f, shape_m, window)
    for model in ar.MODELS:
        for photometric in (True, False):
            S, g, rr, n = ar.sums_on_window(moving, fixed, M, window, model, photometric, ar.SUMS_GAIN, ar.SUMS_BIAS)
            S32, g32, rr32, n32 = ar.sums_on_window(moving, fixed, M, window, model, photometric, ar.SUMS_GAIN, ar.SUMS_BIAS, dtype=np.float32)
            d = np.sqrt(np.diag(S))
            assert (d > 0).all() and n > 0.5 * (shape_f[0] * shape_f[1] if window is None else (window[1] - window[0]) * (window[3] - window[2]))
            eS, eg, er = (np.abs(S32 - S) / np.outer(d, d)).max(), (np.abs(g32 - g) / (d * np.sqrt(rr))).max(), abs(rr32 / rr - 1)
            print("%s against %s, window %s, %s, photometric %s: S %.2g, g %.2g, r^2 %.2g of the gate's unit; count %d" % (
                shape_f, shape_m, window, model, photometric, eS, eg, er, n))
            assert n32 == n
            assert eS <= ar.GATE / 4 and eg <= ar.GATE / 4 and er <= ar.GATE / 4


@pytest.mark.parametrize("case", range(len(ar.SUMS_TRIP_CASES)))
def test_the_float32_sums_of_the_trip_cases_stay_within_a_quarter_of_the_gate(case):
    """the frames of up to 1190 tiles on which the device's reduction runs both loop forms: float32 sums per tile and a float64 sum over
    the tiles do not grow with the frame, so the quarter holds as on the small ones"""
    shape, model, photometric = ar.SUMS_TRIP_CASES[case]
    _, _, _, (S, g, rr, n) = ar.sums_trip_reference(case)
    _, _, _, (S32, g32, rr32, n32) = ar.sums_trip_reference(case, np.float32)
    d = np.sqrt(np.diag(S))
    assert (d > 0).all() and n > 0.5 * shape[0] * shape[1]
    eS, eg, er = (np.abs(S32 - S) / np.outer(d, d)).max(), (np.abs(g32 - g) / (d * np.sqrt(rr))).max(), abs(rr32 / rr - 1)
    print("%s, %s, photometric %s: S %.2g, g %.2g, r^2 %.2g of the gate's unit; count %d" % (shape, model, photometric, eS, eg, er, n))
    assert n32 == n
    assert eS <= ar.GATE / 4 and eg <= ar.GATE / 4 and er <= ar.GATE / 4


@pytest.mark.parametrize("shape_s,shape_o", ar.WARP_CASES)
def test_the_float32_warp_stays_within_a_quarter_of_the_gate(shape_s, shape_o):
    src = ar.warp_source(shape_s)
    for name, M in ar.warp_matrices(shape_s, shape_o).items():
        ref = ar.warp(src, M, shape_o)
        got = ar.warp(src, M, shape_o, dtype=np.float32)
        err, bound = np.abs(got - ref).max(), ar.GATE * max(1.0, np.abs(ref).max())
        print("%s -> %s, %s: float32 against float64 %.3g (gate %.3g)" % (shape_s, shape_o, name, err, bound))
        assert got.dtype == np.float32 and err <= bound / 4


@pytest.mark.parametrize("model,blur", ar.RECOVERY)
def test_the_float32_loop_stays_within_a_quarter_of_the_gate(model, blur):
    """the whole loop with the sums in float32 and in the device's order: its final matrix moves no corner more than a quarter of
    ALIGN_GATE = 0.05 px from the float64 one.  Measured, px: translation 3.5e-6 / 2.6e-6, affine 1.5e-6 / 8.1e-6, homography
    5.4e-6 / 7.7e-6 (sharp / blurred); the device gives the same figures"""
    _, fixed, _ = ar.pair(model, blur)
    ref, per = ar.recovered(model, blur)
    got, per32 = ar.recovered(model, blur, np.float32)
    gap = ar.corner_error(got.matrix, ref.matrix, fixed.shape)
    print("%s, box %d: float32 loop %.2g px from the float64 one; steps %s against %s" % (model, blur, gap, per32, per))
    assert gap <= ar.ALIGN_GATE / 4
    assert all(abs(a - b) <= 1 for a, b in zip(per, per32))


def test_align_args():
    from lib import _native
    ok = _native.align_args
    sm, sf = (160, 192, 3), (200, 180, 3)
    got = ok("affine", True, None, 30, 1e-3, None, None, sm, sf)
    assert got[:5] == (1, 1, 0, 30, 1e-3) and np.array_equal(got[5], np.eye(3)) and got[6] == (0, 200, 0, 180)
    got = ok("homography", False, 2, np.int64(5), 0.5, 2 * ar.translation(3, 4), (10, 150, 0.0, 100), sm, sf)
    assert got[:5] == (2, 0, 2, 5, 0.5) and np.array_equal(got[5], ar.translation(3, 4)) and got[6] == (10, 150, 0, 100)
    assert ok("translation", True, 1, 1, 1, None, (0, 16, 0, 16), sm, sf)[0] == 0
    bad = [dict(model="rigid"), dict(model=1), dict(photometric=1), dict(photometric=None),
           dict(levels=0), dict(levels=9), dict(levels=1.5), dict(levels="2"), dict(levels=True), dict(levels=5),      # 160 >> 4 = 10 px
           dict(iterations=0), dict(iterations=2.5), dict(iterations="3"),
           dict(tolerance=0), dict(tolerance=-1), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance="x"),
           dict(init=np.eye(2)), dict(init=np.zeros((3, 3))), dict(init=np.full((3, 3), np.nan)), dict(init="identity"),
           dict(init=[[1, 0, 0], [0, 1, 0], [0, 0, 0]]),
           dict(window=(0, 0, 0, 10)), dict(window=(0, 201, 0, 180)), dict(window=(-1, 20, 0, 180)), dict(window=(0, 20, 0)), dict(window=(0.5, 20, 0, 180)),
           dict(window=(0, 15, 0, 180)),                                                                             # below 16 px
           dict(shape_moving=(12, 192, 3))]
    for change in bad:
        kw = dict(model="affine", photometric=True, levels=None, iterations=30, tolerance=1e-3, init=None, window=None, shape_moving=sm, shape_fixed=sf)
        kw.update(change)
        with pytest.raises(ValueError):
            print("refused:", change)
            ok(**kw)


def test_plan():
    from lib import _native
    for (H, W), levels in [((160, 192), None), ((4096, 4096), None), ((1023, 1023), None), ((31, 33), None), ((127, 500), None), ((128, 500), None), ((160, 192), 3),
                           ((4096, 4096), 8), ((100000, 70000), None)]:
        plan = _native.align_plan(H, W, levels)
        want = ar.auto_levels((H, W)) if levels is None else levels
        planes = sum((H >> l) * (W >> l) for l in range(want))
        assert plan == (want, 4 * (2 * 67 + 67 * (-(-H // 32)) * (-(-W // 32)) + 2 * planes)) and plan._fields == ("levels", "workspace_bytes")
    assert _native.align_plan(4096, 4096).levels == 7 and _native.align_plan(160, 192).levels == 2 and _native.align_plan(127, 127).levels == 1
    for H, W, levels in ((0, 52, None), (15, 52, None), (160, 192, 5), (160, 192, 9), (160, 192, -1)):
        with pytest.raises(_native.NativeError) as ei:
            _native.align_plan(H, W, levels)
        assert ei.value.code == _native.ICS_EINVAL == -1


def test_entries_and_header():
    from lib import _native
    lib = _native.load()
    cd, ci, vp = C.c_double, C.c_int, C.c_void_p
    pd = C.POINTER(cd)
    assert lib.ics_img_align.argtypes == [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, cd, pd, pd, pd]
    assert lib.ics_img_align_sums.argtypes == [vp, vp, ci, ci, ci, ci, ci, ci, pd, cd, cd, pd, ci]
    assert lib.ics_img_warp.argtypes == [vp, pd, ci, ci, C.POINTER(vp)]
    assert lib.ics_img_align_plan.argtypes == [ci, ci, ci, C.POINTER(ci), C.POINTER(C.c_size_t)]
    assert all(getattr(lib, n).restype is ci for n in ("ics_img_align", "ics_img_align_sums", "ics_img_warp", "ics_img_align_plan"))
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    assert ("int ics_img_align(const ics_img *moving, const ics_img *fixed, int y0, int y1, int x0, int x1, int model, int photometric, int levels,\n"
            "                  int iterations, double tolerance, double M[9] /* in: start, out: result */, double gain_bias[2] /* in/out */,\n"
            "                  double stats[5] /* rms, coverage, steps taken, levels used, last step px */);\n") in header
    assert "int ics_img_warp(const ics_img *src, const double M[9], int oh, int ow, ics_img **out);\n" in header
    assert "int ics_img_align_plan(int H, int W, int levels, int *used, size_t *workspace_bytes);\n" in header
    assert re.search(r"#define ICS_ABI_VERSION 4\b", header) and lib.ics_abi_version() == 4
    assert re.search(r"#define ICS_IMG_ALIGN_MAX_LEVELS 8\b", header) and _native.IMG_ALIGN_MAX_LEVELS == ar.MAX_LEVELS == 8
    # the native entries refuse by themselves, before they touch a frame, what the Python layer refuses before them
    fake = vp(1)
    eye = (cd * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    mat = lambda *v: (cd * 9)(*v)
    gb, stats = (cd * 2)(1.0, 0.0), (cd * 5)()
    good = dict(moving=fake, fixed=fake, y0=0, y1=40, x0=0, x1=52, model=1, photometric=1, levels=0, iterations=30, tolerance=1e-3, M=eye, gain_bias=gb, stats=stats)
    bad = [dict(moving=None), dict(fixed=None), dict(M=None), dict(gain_bias=None), dict(stats=None),
           dict(model=3), dict(model=-1),
           dict(M=mat(1, 0, 0, 0, 1, 0, 0, 0, float("nan"))), dict(M=mat(1, 0, 0, 0, 1, 0, 0, 0, 0)), dict(M=mat(1, 2, 0, 2, 4, 0, 0, 0, 1)),
           dict(M=mat(float("inf"), 0, 0, 0, 1, 0, 0, 0, 1)),
           dict(y1=0), dict(y0=40), dict(x0=52, x1=52), dict(x0=60), dict(y0=-1), dict(x0=-1),
           dict(iterations=0), dict(iterations=-3),
           dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
           dict(levels=-1), dict(levels=9),
           dict(gain_bias=(cd * 2)(0.0, 0.0)), dict(gain_bias=(cd * 2)(float("nan"), 0.0))]
    for change in bad:
        args = dict(good, **change)
        assert lib.ics_img_align(*args.values()) == _native.ICS_EINVAL, change
    sums = (cd * 29)()
    good = dict(moving=fake, fixed=fake, y0=0, y1=40, x0=0, x1=52, model=1, photometric=0, M=eye, gain=1.0, bias=0.0, sums=sums, count=29)
    for change in [dict(moving=None), dict(fixed=None), dict(M=None), dict(sums=None), dict(count=28), dict(photometric=1), dict(model=3), dict(y1=0), dict(x0=-1),
                   dict(M=mat(0, 0, 0, 0, 0, 0, 0, 0, 1)), dict(gain=0.0), dict(bias=float("inf"))]:
        assert lib.ics_img_align_sums(*dict(good, **change).values()) == _native.ICS_EINVAL, change
    out = vp()
    for args in [(None, eye, 4, 4, C.byref(out)), (fake, None, 4, 4, C.byref(out)), (fake, eye, 4, 4, None), (fake, eye, 0, 4, C.byref(out)), (fake, eye, 4, -1, C.byref(out)),
                 (fake, mat(1, 1, 0, 1, 1, 0, 0, 0, 1), 4, 4, C.byref(out)), (fake, mat(1, 0, 0, 0, 1, 0, 0, float("nan"), 1), 4, 4, C.byref(out))]:
        assert lib.ics_img_warp(*args) == _native.ICS_EINVAL and not out.value, args
    for name in ("align_args", "align_plan", "AlignPlan", "Alignment", "ALIGN_MODELS"):
        assert hasattr(_native, name), name
    for name in ("align", "align_sums", "warp"):
        assert hasattr(_native.DeviceImage, name), name


def test_utils_align_and_warp_have_no_cpu_fallback():
    import inspect
    from lib import _native, utils
    assert utils.Alignment._fields == ("matrix", "gain", "bias", "rms", "coverage", "steps")
    assert str(inspect.signature(utils.align)) == ("(moving, fixed, model='affine', photometric=True, levels=None, iterations=30, tolerance=0.001, init=None, "
                                                   "window=None, info=False)")
    assert str(inspect.signature(utils.warp)) == "(src, matrix, shape=None)"
    assert inspect.signature(utils.estimate_psf).parameters["register"].default is None
    assert utils.PsfEstimate._fields == ("psf", "raw", "rejected") and utils.PsfEstimate(1, 2, 3).matrix is None
    z, y = np.zeros((40, 52, 3)), np.zeros((44, 50, 3))
    for args, kw in [((z, y), dict(model="rigid")), ((z, y), dict(levels=3)), ((z, y), dict(iterations=0)), ((z, y), dict(tolerance=0)), ((z, y), dict(init=np.zeros((3, 3)))),
                     ((z, y), dict(window=(0, 45, 0, 50))), ((z[..., 0], y), {}), ((z, y[..., :2]), {}), ((z[:10], y), {})]:
        with pytest.raises(ValueError):                               # refused before anything is uploaded
            utils.align(*args, **kw)
    for args in [(z, np.zeros((3, 3))), (z, np.eye(2)), (z[..., 0], np.eye(3)), (z, np.eye(3), (0, 5))]:
        with pytest.raises(ValueError):
            utils.warp(*args)
    for kw in (dict(register="rigid"), dict(register="affine", window=(0, 41, 0, 52)), dict(register="affine", size=4)):
        with pytest.raises(ValueError):
            utils.estimate_psf(**dict(dict(blurred=z, sharp=y, size=5), **kw))
    if _native.device_count() == 0:
        for call in (lambda: utils.align(z, y), lambda: utils.warp(z, np.eye(3)), lambda: utils.estimate_psf(z, y, 5, register="affine")):
            with pytest.raises(_native.NativeError) as ei:
                call()
            assert ei.value.code == _native.ICS_ENODEV
