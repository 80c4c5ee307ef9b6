"""GPU: DeviceImage.wiener / lib.utils.wiener (csrc/ics_img_wiener.hip) against the float64 specification (tests/wiener_ref.py), with a
box, a Gaussian and an off-centre L-shaped PSF on the three channels, so that a packed pair of channels or a flipped kernel cannot
pass.  Shapes (wiener_ref.GPU_SHAPES): the smallest sizes (8 x 16 transform), small lines, the exact fit 60 + 5 - 1 = 64 and one
over, Py != Px, lines of 2048 and lines of 8192 on either axis (the full LDS line), and the refusal above 8192.

Gate: max |gpu - ref| <= 1e-4 max(1, max |ref|), the project's parity gate; tests/test_wiener.py shows the float32 evaluation of the
specification itself within a quarter of it at every one of these shapes."""
import gc

import numpy as np
import pytest

import test_wiener as tw
import wiener_ref as wr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("balance", wr.BALANCES)
@pytest.mark.parametrize("shape,K", wr.GPU_SHAPES)
def test_wiener_matches_the_float64_specification(shape, K, balance):
    from lib import utils
    f, k, ref = tw.gpu_case(shape, K, balance)
    got = utils.wiener(f, k, balance)
    assert got.shape == ref.shape and got.dtype == np.float32
    err, bound = np.abs(got - ref).max(), wr.GATE * max(1.0, np.abs(ref).max())
    print("wiener %s K %d balance %g -> transform %s: max |gpu - ref| %.3g (gate %.3g)" % (shape, K, balance, wr.sizes(*shape, K), err, bound))
    assert err <= bound


def test_a_transform_above_8192_points_is_refused():
    from lib import _native
    img = _native.DeviceImage.from_host(np.zeros((16, 8192, 3), np.float32))
    try:
        with pytest.raises(_native.NativeError) as ei:
            img.wiener(np.ones((3, 3)), 0.01)
        assert ei.value.code == _native.ICS_ENOSUP and "8192" in str(ei.value)
    finally:
        img.close()


def test_two_runs_give_identical_bits_and_the_source_is_untouched():
    from lib import _native
    f, k, _ = tw.gpu_case((70, 150), 9, 0.01)
    img = _native.DeviceImage.from_host(f)
    a = img.wiener(k, 0.01)
    b = img.wiener(k, 0.01)
    ha, hb, src = a.to_host(), b.to_host(), img.to_host()
    for m in (a, b, img):
        m.close()
    assert np.array_equal(bits(ha), bits(hb))
    assert np.array_equal(bits(src), bits(f))


def test_an_array_and_a_device_image_agree_bit_for_bit():
    from lib import _native, utils
    f, k, _ = tw.gpu_case((40, 52), 5, 0.01)
    from_array = utils.wiener(f, k)
    img = _native.DeviceImage.from_host(f)
    res = utils.wiener(img, k)
    assert isinstance(res, _native.DeviceImage)
    from_image = res.to_host()
    res.close(); img.close()
    assert np.array_equal(bits(from_array), bits(from_image))
    # and a PSF given as one K x K plane is the same PSF on the three channels
    assert np.array_equal(bits(utils.wiener(f, k[..., 1])), bits(utils.wiener(f, np.dstack([k[..., 1]] * 3))))


def test_a_constant_frame_comes_back_constant():
    from lib import utils
    for shape, K in (((40, 52), 5), ((61, 61), 5), ((16, 2040), 9)):
        out = utils.wiener(np.full(shape + (3,), 0.37, np.float32), wr.three_psfs(K), 0.01)
        assert np.abs(out - np.float32(0.37)).max() <= 1e-5, (shape, np.abs(out - np.float32(0.37)).max())


def test_on_poisoned_red_zoned_pool_blocks(debug_switch):
    """pool check mode (csrc/ics_pool.h): every block the call takes is filled with 0xFF (NaN) and its red zone verified when it goes
    back -- a read of a spectrum entry nobody wrote would spread NaN over the frame, a store past a buffer's end would be counted"""
    from lib import _native, utils
    from lib import deconvolution as dc
    f, k, ref = tw.gpu_case((70, 150), 9, 0.01)
    clean = utils.wiener(f, k, 0.01)
    dc._drop_jobs(); gc.collect()
    _native.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned = utils.wiener(f, k, 0.01)
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    assert _native.debug_set("pool_overruns", 0) == 0
    assert np.array_equal(bits(poisoned), bits(clean))
    assert np.abs(poisoned - ref).max() <= wr.GATE * max(1.0, np.abs(ref).max())


def test_driver_with_the_wiener_phase_on_both_paths(capsys, monkeypatch):
    """deblur_module(nonblind="wiener"): the blind phase as ever, then one Wiener pass of the whole frame -- its two printed lines, no
    non-blind call into the solver, the phase time recorded, and the host and the resident path within the driver's own tolerance
    (tests/test_driver.py: the two differ by float32 powf of the gamma steps)"""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from lib import deconvolution as dc
    case = orc.synth_case(97, 121, 5, seed=3)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask=[48, 60], mask_size=61, display=False, iterations=3, pyramid=False, save=False, nonblind="wiener")
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
        assert "===== WIENER DECONVOLUTION =====\nWiener : balance 0.01, 128 × 128 transform\n" in log
    assert set(dv.deblur_module.last_phase_seconds) == {"blind", "non-blind"} and dv.deblur_module.last_phase_seconds["non-blind"] > 0
    assert out_d.shape == out_h.shape == (97, 121, 3) and np.isfinite(out_h).all() and np.isfinite(out_d).all()
    assert np.abs(psf_d - psf_h).max() < 1e-5
    print("host vs resident: %.3g of the 16-bit range" % (np.abs(out_d - out_h).max() / 65535))
    assert np.abs(out_d - out_h).max() / 65535 < 2e-5, np.abs(out_d - out_h).max()
    # the frame really was filtered with the blind phase's PSF: the result is not the loop's
    out_rl, _ = dv.deblur_module(pic, "r", ".", 5, device_resident=True, **dict(kw, nonblind="rl"))
    assert "WIENER" not in capsys.readouterr().out and np.abs(out_rl - out_d).max() / 65535 > 1e-3
