"""GPU: DeviceImage.tv_deconvolve / lib.utils.tv_deconvolve (csrc/ics_img_tvdeconv.hip) against the float64 specification
(tests/tv_deconv_ref.py), with a box, a Gaussian and an off-centre L-shaped PSF on the three channels, so that a swapped channel or a
flipped kernel cannot pass.  Shapes (wiener_ref.GPU_SHAPES), both couplings:

  5 x 7, K 3            8 x 16 transform: a shrink tile larger than the domain, the wrap inside one tile
  60 x 60 / 61 x 61     64^2 / 128^2: the exact fit and one over; log2 even and odd, i.e. the leading radix-2 stage
  70 x 150              128 x 256: Py != Px, several shrink tiles with the wrap on both axes
  16 x 2040, 2040 x 16  long lines on either axis beside a short one
  24 x 8170, 8170 x 24  64 x 8192, 8192 x 64: the full LDS line and the raised LDS limit

Gate: max |gpu - ref| <= 1e-4 max(1, max |ref|), the project's parity gate; tests/test_tv_deconv.py shows the float32 evaluation of the
specification itself within a quarter of it at every one of these cases."""
import gc

import numpy as np
import pytest

import test_tv_deconv as tt
import tv_deconv_ref as tr
import wiener_ref as wr

pytestmark = pytest.mark.gpu

CASES = [(shape, K, coupling, tr.ITERATIONS) for shape, K, coupling in tt.GPU_CASES]
CASES += [(shape, K, coupling, n) for shape, K in (((40, 52), 5), ((70, 150), 9)) for coupling in tr.COUPLINGS for n in (1, 3)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rms(a):
    return float(np.sqrt((a.astype(np.float64) ** 2).mean()))


@pytest.mark.parametrize("shape,K,coupling,iterations", CASES)
def test_tv_deconvolve_matches_the_float64_specification(shape, K, coupling, iterations):
    from lib import utils
    f, k, ref = tt.gpu_case(shape, K, coupling, iterations)
    got = utils.tv_deconvolve(f, k, tr.FIDELITY, tr.PENALTY, iterations, coupling)
    assert got.shape == ref.shape and got.dtype == np.float32
    err, bound = np.abs(got - ref).max(), tt.gate(ref)
    print("tv_deconvolve %s K %d %s %d iterations -> transform %s: max |gpu - ref| %.3g (gate %.3g)" % (shape, K, coupling, iterations, wr.sizes(*shape, K), err, bound))
    assert err <= bound


def test_a_transform_above_8192_points_is_refused():
    from lib import _native
    img = _native.DeviceImage.from_host(np.zeros((16, 8192, 3), np.float32))
    try:
        with pytest.raises(_native.NativeError) as ei:
            img.tv_deconvolve(np.ones((3, 3)))
        assert ei.value.code == _native.ICS_ENOSUP and "8192" in str(ei.value)
    finally:
        img.close()


@pytest.mark.parametrize("coupling", tr.COUPLINGS)
def test_two_runs_give_identical_bits_and_the_source_is_untouched(coupling):
    from lib import _native
    f, k, _ = tt.gpu_case((70, 150), 9, coupling)
    img = _native.DeviceImage.from_host(f)
    a = img.tv_deconvolve(k, coupling=coupling)
    b = img.tv_deconvolve(k, coupling=coupling)
    ha, hb, src = a.to_host(), b.to_host(), img.to_host()
    for m in (a, b, img):
        m.close()
    assert np.array_equal(bits(ha), bits(hb))
    assert np.array_equal(bits(src), bits(f))


def test_an_array_and_a_device_image_agree_bit_for_bit():
    from lib import _native, utils
    f, k, _ = tt.gpu_case((40, 52), 5, "vector")
    from_array = utils.tv_deconvolve(f, k)
    img = _native.DeviceImage.from_host(f)
    res = utils.tv_deconvolve(img, k)
    assert isinstance(res, _native.DeviceImage)
    from_image = res.to_host()
    res.close(); img.close()
    assert np.array_equal(bits(from_array), bits(from_image))
    # and a PSF given as one K x K plane is the same PSF on the three channels
    assert np.array_equal(bits(utils.tv_deconvolve(f, k[..., 1])), bits(utils.tv_deconvolve(f, np.dstack([k[..., 1]] * 3))))


def test_a_constant_frame_comes_back_constant():
    from lib import utils
    for shape, K in (((40, 52), 5), ((61, 61), 5), ((16, 2040), 9)):
        out = utils.tv_deconvolve(np.full(shape + (3,), 0.37, np.float32), wr.three_psfs(K))
        assert np.abs(out - np.float32(0.37)).max() <= 1e-5, (shape, np.abs(out - np.float32(0.37)).max())


def test_on_poisoned_red_zoned_pool_blocks(debug_switch):
    """pool check mode (csrc/ics_pool.h): the workspace is filled with 0xFF (NaN) and its red zone verified when it goes back -- a
    read of an entry nobody wrote (a spectrum, a b plane, a halo) would spread NaN over the frame, a store past the end would be counted"""
    from lib import _native, utils
    from lib import deconvolution as dc
    f, k, ref = tt.gpu_case((70, 150), 9, "vector")
    clean = utils.tv_deconvolve(f, k)
    dc._drop_jobs(); gc.collect()
    _native.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned = utils.tv_deconvolve(f, k)
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    assert _native.debug_set("pool_overruns", 0) == 0
    assert np.array_equal(bits(poisoned), bits(clean))
    assert np.abs(poisoned - ref).max() <= tt.gate(ref)


def test_the_three_quality_cases_beat_the_wiener_filter_on_the_device():
    from lib import utils
    for sharp, blurred, psf in wr.quality_cases():
        f = blurred.astype(np.float32)
        w = rms(utils.wiener(f, psf, 0.01) - sharp)
        for coupling in tr.COUPLINGS:
            t = rms(utils.tv_deconvolve(f, psf, coupling=coupling) - sharp)
            print("%s %s: blurred %.4f, wiener %.4f, tv %.4f" % (f.shape[:2], coupling, rms(f - sharp), w, t))
            assert t < w


def test_driver_with_the_tv_phase_on_both_paths(capsys, monkeypatch):
    """deblur_module(nonblind="tv"): the blind phase as ever, then one TV deconvolution of the whole frame -- its two printed lines, no
    non-blind call into the solver, the phase time recorded, and the host and the resident path within the driver's own tolerance
    (tests/test_driver.py: the two differ by float32 powf of the gamma steps)"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib import deconvolution as dc
    case = orc.synth_case(97, 121, 5, seed=3)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask=[48, 60], mask_size=61, display=False, iterations=3, pyramid=False, save=False, nonblind="tv")
    calls = {"host": [], "device": []}

    def host_solver(*a, **k):
        calls["host"].append(k["blind"])
        return dc.richardson_lucy_MM(*a, **k)

    real_device = dc.richardson_lucy_MM_device

    def device_solver(*a, **k):
        calls["device"].append(k["blind"])
        return real_device(*a, **k)

    monkeypatch.setattr(dc, "richardson_lucy_MM_device", device_solver)
    out_h, psf_h = dv.deblur_module(pic, "h", ".", 5, solver=host_solver, **kw)
    log_h = capsys.readouterr().out
    dv.deblur_module.last_phase_seconds = {}
    out_d, psf_d = dv.deblur_module(pic, "d", ".", 5, device_resident=True, **kw)
    log_d = capsys.readouterr().out
    assert calls == {"host": [True], "device": [True]}                 # one pyramid level, blind; nothing non-blind
    for log in (log_h, log_d):
        assert "===== blind DECONVOLUTION =====" in log and "===== non-blind DECONVOLUTION =====" not in log
        assert "\n===== TV DECONVOLUTION =====\nTV : fidelity 2000, penalty 10, 10 iterations, vector, 128 × 128 transform\n" in log
    assert set(dv.deblur_module.last_phase_seconds) == {"blind", "non-blind"}
    assert dv.deblur_module.last_phase_seconds["blind"] > 0 and dv.deblur_module.last_phase_seconds["non-blind"] > 0
    assert out_d.shape == out_h.shape == (97, 121, 3) and np.isfinite(out_h).all() and np.isfinite(out_d).all()
    assert np.abs(psf_d - psf_h).max() < 1e-5
    print("host vs resident: %.3g of the 16-bit range" % (np.abs(out_d - out_h).max() / 65535))
    assert np.abs(out_d - out_h).max() / 65535 < 2e-5, np.abs(out_d - out_h).max()
    # the frame really went through this solver with the blind phase's PSF: the result is neither the loop's nor the Wiener filter's
    for other in ("rl", "wiener"):
        out_o, _ = dv.deblur_module(pic, "o", ".", 5, device_resident=True, **dict(kw, nonblind=other))
        assert "TV DECONVOLUTION" not in capsys.readouterr().out and np.abs(out_o - out_d).max() / 65535 > 1e-3
