"""GPU: DeviceImage.tv_deconvolve_masked / lib.utils.tv_deconvolve_masked (csrc/ics_img_tvmdeconv.hip) against the float64 specification
(tests/tvm_deconv_ref.py), with a box, a Gaussian and an off-centre L-shaped PSF on the three channels, so that a swapped channel or a
flipped kernel cannot pass.  Shapes (wiener_ref.GPU_SHAPES), both couplings, three mask forms each (none, clip 0.99, an array with a
block, a row and a column out):

  5 x 7, K 3            8 x 16 transform: a shrink tile larger than the domain, the wrap inside one tile
  40 x 52               the plain case; once more with NaN and inf pixels
  60 x 60 / 61 x 61     64^2 / 128^2: the exact fit and one over; log2 even and odd, i.e. the leading radix-2 stage; 61 x 61 with data_penalty 200
  70 x 150              128 x 256: Py != Px, several shrink tiles with the wrap on both axes
  16 x 2040, 2040 x 16  long lines on either axis beside a short one
  24 x 8170, 8170 x 24  64 x 8192, 8192 x 64: the full LDS line, eight points a lane in the column kernel, the raised LDS limit; 3 iterations

Gate: max |gpu - ref| <= 1e-4 max(1, max |ref|), the project's parity gate; tests/test_tvm_deconv.py shows the float32 evaluation of the
specification itself within a quarter of it at every one of these cases."""
import gc

import numpy as np
import pytest

import test_tvm_deconv as tt
import tvm_deconv_ref as tm
import wiener_ref as wr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape,K,coupling,mask,data_penalty,nonfinite", tt.GPU_CASES)
def test_tv_deconvolve_masked_matches_the_float64_specification(shape, K, coupling, mask, data_penalty, nonfinite):
    from lib import utils
    f, k, observed, clip, n, ref, count = tt.gpu_case(shape, K, coupling, mask, data_penalty, nonfinite)
    got, unobserved = utils.tv_deconvolve_masked(f, k, observed, clip, tm.FIDELITY, tm.PENALTY, data_penalty, n, coupling, count=True)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    err, bound = np.abs(got - ref).max(), tt.gate(ref)
    print("tv_deconvolve_masked %s K %d %s mask %s%s %d iterations -> transform %s, %d unobserved: max |gpu - ref| %.3g (gate %.3g)"
          % (shape, K, coupling, mask, " with NaN and inf" if nonfinite else "", n, wr.sizes(*shape, K), unobserved, err, bound))
    assert unobserved == count
    assert err <= bound


def test_a_transform_above_8192_points_is_refused():
    from lib import _native
    img = _native.DeviceImage.from_host(np.zeros((16, 8192, 3), np.float32))
    try:
        with pytest.raises(_native.NativeError) as ei:
            img.tv_deconvolve_masked(np.ones((3, 3)))
        assert ei.value.code == _native.ICS_ENOSUP and "8192" in str(ei.value)
    finally:
        img.close()


@pytest.mark.parametrize("coupling", tm.COUPLINGS)
def test_two_runs_give_identical_bits_and_the_source_is_untouched(coupling):
    from lib import _native
    f, k, observed, clip, n, _, count = tt.gpu_case((70, 150), 9, coupling, "array")
    img = _native.DeviceImage.from_host(f)
    a, na = img.tv_deconvolve_masked(k, observed, 0.9, coupling=coupling, count=True)
    b, nb = img.tv_deconvolve_masked(k, observed, 0.9, coupling=coupling, count=True)
    ha, hb, src = a.to_host(), b.to_host(), img.to_host()
    for m in (a, b, img):
        m.close()
    assert na == nb >= count
    assert np.array_equal(bits(ha), bits(hb))
    assert np.array_equal(bits(src), bits(f))


def test_an_array_and_a_device_image_agree_bit_for_bit():
    from lib import _native, utils
    f, k, observed, clip, n, _, count = tt.gpu_case((40, 52), 5, "vector", "array")
    from_array = utils.tv_deconvolve_masked(f, k, observed)
    img = _native.DeviceImage.from_host(f)
    res, unobserved = utils.tv_deconvolve_masked(img, k, observed, count=True)
    assert isinstance(res, _native.DeviceImage) and unobserved == count
    from_image = res.to_host()
    res.close(); img.close()
    assert np.array_equal(bits(from_array), bits(from_image))
    # a mask of any number type is the same mask, and the call without count gives the same picture
    assert np.array_equal(bits(from_array), bits(utils.tv_deconvolve_masked(f, k, observed.astype(np.float64) * 3.5)))


def test_on_poisoned_red_zoned_pool_blocks(debug_switch):
    """pool check mode (csrc/ics_pool.h): the workspace is filled with 0xFF (NaN) and its red zone verified when it goes back -- a
    read of an entry nobody wrote (a spectrum, a plane, a halo, the mask) would spread NaN over the frame, a store past the end would
    be counted; the block goes back on every path"""
    from lib import _native, utils
    from lib import deconvolution as dc
    f, k, observed, clip, n, ref, count = tt.gpu_case((70, 150), 9, "vector", "array")
    clean = utils.tv_deconvolve_masked(f, k, observed)
    dc._drop_jobs(); gc.collect()
    _native.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned, unobserved = utils.tv_deconvolve_masked(f, k, observed, count=True)
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    assert _native.debug_set("pool_overruns", 0) == 0
    assert unobserved == count
    assert np.array_equal(bits(poisoned), bits(clean))
    assert np.abs(poisoned - ref).max() <= tt.gate(ref)


def test_driver_with_the_masked_tv_phase_on_both_paths(capsys, monkeypatch):
    """deblur_module(nonblind="tv-masked"): the blind phase as ever, then one masked TV deconvolution of the whole frame -- its two
    printed lines, no non-blind call into the solver, and the host and the resident path within the bound of
    tests/test_gpu_tv_deconv.py for the two paths; nonblind="rl" beside it makes the solver calls it always made"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib import deconvolution as dc
    case = orc.synth_case(97, 121, 5, seed=3)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask=[48, 60], mask_size=61, display=False, iterations=3, pyramid=False, save=False, nonblind="tv-masked")
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
        assert "\n===== MASKED TV DECONVOLUTION =====\nTV-masked : fidelity 2000, penalties 10 / 2000, 10 iterations, vector, clip 0.99, 128 × 128 transform, " in log
        assert log.split("128 × 128 transform, ")[1].split("\n")[0].endswith(" % unobserved")
    assert set(dv.deblur_module.last_phase_seconds) == {"blind", "non-blind"}
    assert out_d.shape == out_h.shape == (97, 121, 3) and np.isfinite(out_h).all() and np.isfinite(out_d).all()
    assert np.abs(psf_d - psf_h).max() < 1e-5
    print("host vs resident: %.3g of the 16-bit range" % (np.abs(out_d - out_h).max() / 65535))
    assert np.abs(out_d - out_h).max() / 65535 < 2e-5, np.abs(out_d - out_h).max()
    # the loop beside it: its two phases, both through the solver, and another picture
    calls["device"].clear()
    out_o, _ = dv.deblur_module(pic, "o", ".", 5, device_resident=True, **dict(kw, nonblind="rl"))
    log_o = capsys.readouterr().out
    assert calls["device"] == [True, False] and "TV DECONVOLUTION" not in log_o and "===== non-blind DECONVOLUTION =====" in log_o
    assert np.abs(out_o - out_d).max() / 65535 > 1e-3
    out_t, _ = dv.deblur_module(pic, "t", ".", 5, device_resident=True, **dict(kw, nonblind="tv"))
    assert "MASKED" not in capsys.readouterr().out and np.abs(out_t - out_d).max() / 65535 > 1e-4
