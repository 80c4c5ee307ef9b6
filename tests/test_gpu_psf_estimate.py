"""GPU: DeviceImage.psf_raw / lib.utils.estimate_psf (csrc/ics_img_psfest.hip) against the float64 specification
(tests/psf_est_ref.py), the blurred frame made from the sharp one by a box, a Gaussian and an off-centre L-shaped PSF on the three
channels, so that a packed pair of channels, a swapped pair of frames or a flipped kernel cannot pass.  Shapes (psf_est_ref.GPU_CASES):
the smallest sizes (8 x 16 transform, the taper clamped by H // 2), small lines, the exact fit 60 + 5 - 1 = 64 and one over, Py != Px,
lines of 2048 and of 8192 on either axis (the full LDS line), the largest K with the crop wrapping far, and the refusal above 8192.

Gate: max |gpu - ref| <= 1e-4 max |ref| on the raw kernel, the project's parity gate taken relative to the peak of raw because the taps
are far below 1 (tests/test_psf_estimate.py shows the float32 evaluation of the specification itself within a quarter of it at every
one of these shapes); 1e-5 relative on the energies."""
import gc

import numpy as np
import pytest

import psf_est_ref as pr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw_of(b, s, K, regularisation=pr.REGULARISATION, coupling="vector", window=None):
    """DeviceImage.psf_raw of two arrays: (raw, energy)"""
    from lib import _native
    db, ds = _native.DeviceImage.from_host(b), _native.DeviceImage.from_host(s)
    try:
        return db.psf_raw(ds, K, regularisation, coupling, window)
    finally:
        db.close(); ds.close()


@pytest.mark.parametrize("shape,K", pr.GPU_CASES)
def test_every_case_has_gradients(shape, K):
    s, _ = pr.gpu_pair(shape, K)
    assert (pr.gpu_reference(shape, K, pr.REGULARISATIONS[0], "channel")[1] > 0).all() and s.shape == shape + (3,)


@pytest.mark.parametrize("coupling", pr.COUPLINGS)
@pytest.mark.parametrize("regularisation", pr.REGULARISATIONS)
@pytest.mark.parametrize("shape,K", pr.GPU_CASES)
def test_raw_and_energy_match_the_float64_specification(shape, K, regularisation, coupling):
    s, b = pr.gpu_pair(shape, K)
    ref, S = pr.gpu_reference(shape, K, regularisation, coupling)
    raw, energy = raw_of(b, s, K, regularisation, coupling)
    assert raw.shape == ref.shape == (K, K, 3) and raw.dtype == np.float32 and energy.shape == (3,) and energy.dtype == np.float64
    err, bound = np.abs(raw - ref).max(), pr.GATE * np.abs(ref).max()
    rel = np.abs(energy / S - 1).max()
    print("psf_raw %s K %d regularisation %g %s: max |gpu - ref| %.3g (gate %.3g, ratio %.3g); energy %.3g relative" % (
        shape, K, regularisation, coupling, err, bound, err / bound, rel))
    assert err <= bound
    assert rel <= pr.ENERGY_GATE
    if coupling == "vector":
        assert np.array_equal(bits(raw[..., 0]), bits(raw[..., 1])) and np.array_equal(bits(raw[..., 0]), bits(raw[..., 2])) and energy[0] == energy[1] == energy[2]


def test_a_window_with_odd_offsets_gives_the_bits_of_the_two_crops():
    s, b = pr.gpu_pair((70, 150), 9)
    y0, y1, x0, x1 = 3, 64, 5, 86
    for coupling in pr.COUPLINGS:
        win, ew = raw_of(b, s, 9, 1e-3, coupling, (y0, y1, x0, x1))
        crop, ec = raw_of(np.ascontiguousarray(b[y0:y1, x0:x1]), np.ascontiguousarray(s[y0:y1, x0:x1]), 9, 1e-3, coupling)
        assert np.array_equal(bits(win), bits(crop)) and np.array_equal(ew, ec)
        ref = pr.raw_kernel(b[y0:y1, x0:x1], s[y0:y1, x0:x1], 9, 1e-3, coupling)[0]
        assert np.abs(win - ref).max() <= pr.GATE * np.abs(ref).max()


def test_two_runs_give_identical_bits_and_both_sources_are_untouched():
    from lib import _native
    s, b = pr.gpu_pair((70, 150), 9)
    db, ds = _native.DeviceImage.from_host(b), _native.DeviceImage.from_host(s)
    r1, e1 = db.psf_raw(ds, 9, coupling="channel")
    r2, e2 = db.psf_raw(ds, 9, coupling="channel")
    hb, hs = db.to_host(), ds.to_host()
    db.close(); ds.close()
    assert np.array_equal(bits(r1), bits(r2)) and np.array_equal(e1, e2)
    assert np.array_equal(bits(hb), bits(b)) and np.array_equal(bits(hs), bits(s))


def test_arrays_and_device_images_agree_bit_for_bit():
    from lib import _native, utils
    s, b = pr.gpu_pair((40, 52), 5)
    from_arrays = utils.estimate_psf(b, s, 5, info=True)
    db, ds = _native.DeviceImage.from_host(b), _native.DeviceImage.from_host(s)
    from_images = utils.estimate_psf(db, ds, 5, info=True)
    with pytest.raises(ValueError, match="both"):
        utils.estimate_psf(db, s, 5)
    db.close(); ds.close()
    assert np.array_equal(bits(from_arrays.raw), bits(from_images.raw)) and np.array_equal(bits(from_arrays.psf), bits(from_images.psf))
    assert from_arrays.rejected == from_images.rejected and from_arrays.psf.dtype == np.float32 and from_arrays.psf.shape == (5, 5, 3)
    assert np.abs(from_arrays.psf.sum(axis=(0, 1)) - 1).max() < 1e-6
    assert np.array_equal(bits(utils.estimate_psf(b, s, 5)), bits(from_arrays.psf))


def test_on_poisoned_red_zoned_pool_blocks(debug_switch):
    """pool check mode (csrc/ics_pool.h): every block the call takes is filled with 0xFF (NaN) and its red zone verified when it goes
    back -- a read of a spectrum entry nobody wrote would spread NaN over the kernel, a store past the workspace's end would be counted"""
    from lib import _native
    from lib import deconvolution as dc
    s, b = pr.gpu_pair((70, 150), 9)
    for coupling in pr.COUPLINGS:
        clean, e0 = raw_of(b, s, 9, 1e-3, coupling)
        dc._drop_jobs(); gc.collect()
        _native.debug_set("pool_overruns", 0)
        debug_switch("pool_check", 0xFF)
        poisoned, e1 = raw_of(b, s, 9, 1e-3, coupling)
        gc.collect()
        debug_switch("pool_check", -1)
        gc.collect()
        assert _native.debug_set("pool_overruns", 0) == 0
        assert np.array_equal(bits(poisoned), bits(clean)) and np.array_equal(e0, e1)


def test_a_transform_above_8192_points_is_refused():
    from lib import _native
    z = np.zeros((16, 8192, 3), np.float32)
    with pytest.raises(_native.NativeError) as ei:
        raw_of(z, z, 3)
    assert ei.value.code == _native.ICS_ENOSUP and "8192" in str(ei.value)


def test_frames_of_different_shapes_are_refused():
    from lib import _native, utils
    s, b = pr.gpu_pair((40, 52), 5)
    with pytest.raises(ValueError, match="different shapes"):
        raw_of(b, s[:, :50], 5)
    with pytest.raises(ValueError, match="different shapes"):
        utils.estimate_psf(b[:39], s, 5)
    # ... and by the native entry itself
    import ctypes as C
    db, ds = _native.DeviceImage.from_host(b), _native.DeviceImage.from_host(np.ascontiguousarray(s[:, :50]))
    raw, energy = (C.c_float * 75)(), (C.c_double * 3)()
    rc = _native.load().ics_img_psf_estimate(db._h, ds._h, 0, 40, 0, 50, 5, 1e-3, 1, raw, energy)
    rc_box = _native.load().ics_img_psf_estimate(db._h, db._h, 0, 41, 0, 52, 5, 1e-3, 1, raw, energy)
    db.close(); ds.close()
    assert rc == _native.ICS_EINVAL and rc_box == _native.ICS_EINVAL


def test_a_nan_in_either_frame_raises_not_finite():
    from lib import utils
    s, b = pr.gpu_pair((40, 52), 5)
    for which in (0, 1):
        pair = [b.copy(), s.copy()]
        pair[which][20, 30, 1] = np.nan
        with pytest.raises(ValueError, match="not finite"):
            utils.estimate_psf(pair[0], pair[1], 5)


def test_a_constant_sharp_frame_raises_no_gradients():
    from lib import utils
    _, b = pr.gpu_pair((40, 52), 5)
    with pytest.raises(ValueError, match="no gradients"):
        utils.estimate_psf(b, np.full(b.shape, 0.37, np.float32), 5)


def test_wiener_with_the_estimate_lowers_the_error():
    """end to end on the 70 x 150 quality case (a 9-px box, sigma 0.002): with the true PSF wiener takes the rms error to the sharp frame
    from 0.1095 to 0.0790 (README)"""
    from lib import utils
    sharp, blurred, k = pr.quality_cases()[1]
    est = utils.estimate_psf(blurred, sharp, 9)
    rms = lambda a: float(np.sqrt(np.mean((np.asarray(a, np.float64) - sharp) ** 2)))
    before, after, true = rms(blurred), rms(utils.wiener(blurred, est)), rms(utils.wiener(blurred, k))
    print("wiener with the estimated PSF: rms %.4f -> %.4f (true PSF: %.4f); L1 of the estimate to the true box %.4f" % (
        before, after, true, np.abs(est[..., 0] - k[..., 0]).sum()))
    assert after < before
