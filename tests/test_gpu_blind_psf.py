"""GPU: DeviceImage.psf_raw(mask=) (k_img_ed_rows of csrc/ics_img_edges.hip in front of the pair solve of csrc/ics_img_psfest.hip)
against the float64 specification (edges_ref.masked_raw_kernel) with a given random mask of density 0.3 and with the specification's
own mask of the sharp frame, on the smallest transform (8 x 16), a small plain case, one over the exact fit 60 + 5 - 1 = 64, Py != Px,
and lines of 2048 on either axis; both couplings.  Gate: psf_est_ref.GATE max |ref|, the gate of the unmasked solve.  An all-ones mask
gives the bits of mask=None; a window with odd offsets equals its crop.

lib.utils.blind_psf end to end on box 5 (80 x 104), box 9 and the L of 9 (160 x 192): the device's PSF meets the quality conditions of
tests/test_edges.py, and its L1 to the specification's PSF is within edges_ref.BLIND_GATE, four times the scatter rounding alone
produces (measured into edges_ref.BLIND_SCATTER).  deblur_module(blind="fast", nonblind="wiener") on a 160 x 192 picture."""
import gc

import numpy as np
import pytest

import edges_ref as er
import psf_est_ref as pr

pytestmark = pytest.mark.gpu

CASES = [((5, 7), 3), ((40, 52), 5), ((61, 61), 5), ((70, 150), 9), ((16, 2040), 9), ((2040, 16), 9)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw_of(b, s, mask, K, regularisation=pr.REGULARISATION, coupling="vector", window=None):
    from lib import _native
    db, ds = _native.DeviceImage.from_host(b), _native.DeviceImage.from_host(s)
    dm = None if mask is None else _native.DeviceMask.from_host(mask)
    try:
        return db.psf_raw(ds, K, regularisation, coupling, window, mask=dm)
    finally:
        db.close(); ds.close()
        if dm is not None:
            dm.close()


def masks_of(shape, K, coupling):
    """the random mask and the specification's own mask of the sharp frame (per_sector as blind_psf starts: keep = 2)"""
    s, _ = pr.gpu_pair(shape, K)
    H, W = shape
    rng = np.random.default_rng(H * 31 + W + K)
    random = rng.random((H, W) if coupling == "vector" else (H, W, 3)) < 0.3
    own = er.edge_mask(s, int(np.ceil(2.0 * np.sqrt(H * W) * K / 4)), coupling, np.float32)[0]
    return {"random": random, "own": own}


@pytest.mark.parametrize("coupling", pr.COUPLINGS)
@pytest.mark.parametrize("shape,K", CASES)
def test_masked_raw_matches_the_float64_specification(shape, K, coupling):
    s, b = pr.gpu_pair(shape, K)
    for name, mask in masks_of(shape, K, coupling).items():
        assert mask.any() and not mask.all()
        ref, S = er.masked_raw_kernel(b, s, mask, K, pr.REGULARISATION, coupling)
        raw, energy = raw_of(b, s, mask, K, pr.REGULARISATION, coupling)
        assert raw.shape == ref.shape == (K, K, 3) and raw.dtype == np.float32
        err, bound = np.abs(raw - ref).max(), pr.GATE * np.abs(ref).max()
        rel = np.abs(energy / S - 1).max()
        print("masked psf_raw %s K %d %s, %s mask (%.2f kept): max |gpu - ref| %.3g (gate %.3g, ratio %.3g); energy %.3g relative" % (
            shape, K, coupling, name, mask.mean(), err, bound, err / bound, rel))
        assert err <= bound
        assert rel <= pr.ENERGY_GATE
        if name == "random":                                            # (dead leaves are piecewise constant: their own mask can keep every gradient there is)
            plain = pr.raw_kernel(b, s, K, pr.REGULARISATION, coupling)[0]
            assert np.abs(ref - plain).max() > 10 * bound               # the mask matters: the unmasked kernel would not pass


@pytest.mark.parametrize("coupling", pr.COUPLINGS)
def test_an_all_ones_mask_gives_the_bits_of_no_mask(coupling):
    for shape, K in (((40, 52), 5), ((70, 150), 9)):
        s, b = pr.gpu_pair(shape, K)
        ones = np.ones(shape if coupling == "vector" else shape + (3,), bool)
        masked, em = raw_of(b, s, ones, K, 1e-3, coupling)
        plain, ep = raw_of(b, s, None, K, 1e-3, coupling)
        assert np.array_equal(bits(masked), bits(plain)) and np.array_equal(em, ep)


def test_a_window_with_odd_offsets_gives_the_bits_of_the_crops():
    s, b = pr.gpu_pair((70, 150), 9)
    y0, y1, x0, x1 = 3, 64, 5, 86
    for coupling in pr.COUPLINGS:
        mask = masks_of((70, 150), 9, coupling)["random"]
        win, ew = raw_of(b, s, mask, 9, 1e-3, coupling, (y0, y1, x0, x1))
        crop, ec = raw_of(np.ascontiguousarray(b[y0:y1, x0:x1]), np.ascontiguousarray(s[y0:y1, x0:x1]), np.ascontiguousarray(mask[y0:y1, x0:x1]), 9, 1e-3, coupling)
        assert np.array_equal(bits(win), bits(crop)) and np.array_equal(ew, ec)
        ref = er.masked_raw_kernel(b[y0:y1, x0:x1], s[y0:y1, x0:x1], mask[y0:y1, x0:x1], 9, 1e-3, coupling)[0]
        assert np.abs(win - ref).max() <= pr.GATE * np.abs(ref).max()


def test_the_devices_own_prediction_feeds_the_solve_without_leaving_it(debug_switch):
    """shock -> edge_mask -> psf_raw(mask=) on device handles only, twice, the second time on poisoned red-zoned pool blocks: identical
    bits, no overrun; and the raw kernel is the float64 specification's for the device's shock frame and mask"""
    from lib import _native
    from lib import deconvolution as dc
    s, b = pr.gpu_pair((70, 150), 9)

    def run(coupling):
        db = _native.DeviceImage.from_host(b)
        p = db.shock(4, coupling=coupling)
        m = p.edge_mask(600, coupling)
        try:
            raw, energy = db.psf_raw(p, 9, 1e-3, coupling, mask=m.mask)
            return raw, energy, p.to_host(), m.mask.to_host()
        finally:
            for o in (db, p, m.mask):
                o.close()

    for coupling in pr.COUPLINGS:
        raw, energy, p, mask = run(coupling)
        ref, S = er.masked_raw_kernel(b, p, mask, 9, 1e-3, coupling)
        assert np.abs(raw - ref).max() <= pr.GATE * np.abs(ref).max() and np.abs(energy / S - 1).max() <= pr.ENERGY_GATE
        dc._drop_jobs(); gc.collect()
        _native.debug_set("pool_overruns", 0)
        debug_switch("pool_check", 0xFF)
        raw2, energy2, p2, mask2 = run(coupling)
        gc.collect()
        debug_switch("pool_check", -1)
        gc.collect()
        assert _native.debug_set("pool_overruns", 0) == 0
        assert np.array_equal(bits(raw), bits(raw2)) and np.array_equal(energy, energy2) and np.array_equal(bits(p), bits(p2)) and np.array_equal(mask, mask2)


def test_refusals_of_the_mask():
    from lib import _native
    s, b = pr.gpu_pair((40, 52), 5)
    db, ds = _native.DeviceImage.from_host(b), _native.DeviceImage.from_host(s)
    m1, m3 = _native.DeviceMask.from_host(np.ones((40, 52), bool)), _native.DeviceMask.from_host(np.ones((40, 52, 3), bool))
    small = _native.DeviceMask.from_host(np.ones((40, 50), bool))
    try:
        for mask, coupling in ((m3, "vector"), (m1, "channel"), (small, "vector"), (np.ones((40, 52), bool), "vector")):
            with pytest.raises(ValueError, match="mask"):
                db.psf_raw(ds, 5, 1e-3, coupling, mask=mask)
        import ctypes as C
        raw, energy = (C.c_float * 75)(), (C.c_double * 3)()
        lib = _native.load()
        assert lib.ics_img_psf_estimate_masked(db._h, ds._h, None, 0, 40, 0, 52, 5, 1e-3, 1, raw, energy) == _native.ICS_EINVAL
        assert lib.ics_img_psf_estimate_masked(db._h, ds._h, m3._h, 0, 40, 0, 52, 5, 1e-3, 1, raw, energy) == _native.ICS_EINVAL
        assert lib.ics_img_psf_estimate_masked(db._h, ds._h, small._h, 0, 40, 0, 50, 5, 1e-3, 1, raw, energy) == _native.ICS_EINVAL
        with pytest.raises(ValueError):
            _native.DeviceMask.from_host(np.ones((4, 5, 2), bool))
        assert m3.shape == (40, 52, 3) and np.array_equal(m3.to_host(), np.ones((40, 52, 3), bool))
    finally:
        for o in (db, ds, m1, m3, small):
            o.close()


@pytest.mark.parametrize("name", er.BLIND_GPU_CASES)
def test_blind_psf_meets_the_quality_conditions_and_the_specifications_psf(name):
    from lib import _native, utils
    sharp, blurred, k, spec = er.blind_reference(name)
    K = k.shape[0]
    got = utils.blind_psf(blurred, K, info=True)
    psf = got.psf
    assert psf.shape == (K, K, 3) and psf.dtype == np.float32 and np.abs(psf.sum(axis=(0, 1)) - 1).max() < 1e-6 and (psf >= 0).all()
    assert got.levels == er.blind_levels(blurred.shape[0], blurred.shape[1], K) == _native.blind_psf_plan(blurred.shape[0], blurred.shape[1], K).levels
    assert len(got.kept) == len(got.rejected) == len(got.levels)
    q = er.quality(name, psf, lambda f, p: utils.wiener(f, p, er.BLIND["balance"]))
    dist = float(np.abs(psf[..., 0].astype(np.float64) - spec[..., 0]).sum())
    print("blind_psf %s on the device: L1 to truth %.3f, guesses %s, own flip %.3f; rms %.4f -> %.4f; L1 to the specification's PSF %.6f (gate %.6f)" % (
        name, q["l1"], {n: round(v, 3) for n, v in q["guesses"].items()}, q["flip"], q["rms_blurred"], q["rms_wiener"], dist, er.BLIND_GATE))
    er.assert_quality(name, q)
    assert dist <= er.BLIND_GATE
    # a DeviceImage is read where it lies, a window of it equals the crop, and two runs give identical bits
    pad = np.pad(blurred, ((3, 2), (5, 4), (0, 0)), mode="edge")
    d = _native.DeviceImage.from_host(pad)
    try:
        win = utils.blind_psf(d, K, window=(3, 3 + blurred.shape[0], 5, 5 + blurred.shape[1]))
        back = d.to_host()
    finally:
        d.close()
    assert np.array_equal(bits(win), bits(psf)) and np.array_equal(bits(back), bits(pad))


def test_blind_psf_refusals_and_the_pool(debug_switch):
    from lib import _native, utils
    from lib import deconvolution as dc
    _, blurred, k, _ = er.blind_reference("box5")
    for kw in (dict(size=4), dict(size=1), dict(size=257), dict(size=21), dict(size=5, iterations=0), dict(size=5, keep=0), dict(size=5, balance=-1),
               dict(size=5, shock=(4, 0.4)), dict(size=5, coupling="rgb"), dict(size=5, window=(0, 19, 0, 104))):
        with pytest.raises(ValueError):
            utils.blind_psf(blurred, **kw)
    with pytest.raises(ValueError, match="smaller than 4 x size"):
        utils.blind_psf(blurred, 21)
    with pytest.raises(ValueError, match="smaller than 4 x size"):
        _native.blind_psf_plan(80, 104, 21)
    bad = blurred.copy()
    bad[40, 50, 1] = np.nan
    with pytest.raises(ValueError, match="not finite: despeckle first"):
        utils.blind_psf(bad, 5)
    d = _native.DeviceImage.from_host(bad)
    try:
        with pytest.raises(ValueError, match="not finite: despeckle first"):
            utils.blind_psf(d, 5)
    finally:
        d.close()
    with pytest.raises(ValueError, match="no gradients to select"):
        utils.blind_psf(np.full((80, 104, 3), 0.5, np.float32), 5)
    plan = _native.blind_psf_plan(80, 104, 5)
    assert plan.levels == [(3, 40, 52), (5, 80, 104)] and plan.peak_bytes > 4 * 12 * 80 * 104
    # on poisoned, red-zoned pool blocks: the same bits, no overrun, and nothing left in use after a refusal
    clean = utils.blind_psf(blurred, 5)
    dc._drop_jobs(); gc.collect()
    _native.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned = utils.blind_psf(blurred, 5)
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    assert _native.debug_set("pool_overruns", 0) == 0
    assert np.array_equal(bits(clean), bits(poisoned))


def picture():
    """the box-9 case as an 8-bit picture in linear light: deblur_module encodes it with gamma 1 / 2.2 before anything else"""
    _, blurred, _, _ = er.blind_reference("box9")
    return np.round(np.clip(blurred.astype(np.float64), 0, 1) ** 2.2 * 255).astype(np.float32)


def run_driver(**kw):
    import contextlib
    import io
    import deconvolve
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out, psf = deconvolve.deblur_module(picture(), "blind-fast", "/nonexistent", 9, mask_size=121, display=False, save=False, iterations=5, **kw)
    return out, psf, buf.getvalue(), dict(deconvolve.deblur_module.last_phase_seconds)


def test_the_driver_with_a_fast_blind_phase():
    host, psf_h, text_h, _ = run_driver(blind="fast", nonblind="wiener", device_resident=False)
    dev, psf_d, text_d, phases = run_driver(blind="fast", nonblind="wiener", device_resident=True)
    for text in (text_h, text_d):
        assert "===== FAST BLIND PSF =====" in text and text.count("Level : PSF") == 3 and "===== blind DECONVOLUTION =====" not in text
        assert "===== WIENER DECONVOLUTION =====" in text
    for psf in (psf_h, psf_d):
        assert psf.shape == (9, 9, 3) and psf.dtype == np.float32 and np.abs(psf.sum(axis=(0, 1)) - 1).max() < 1e-6
    assert phases["blind"] > 0 and phases["non-blind"] > 0
    # The two paths encode the gamma on different processors (numpy's and the device's powf differ in the last bit of some pixels), so
    # the frames the alternation sees differ by rounding: the PSFs may differ by what rounding alone scatters, edges_ref.BLIND_GATE; the
    # Wiener filter at balance 0.01 amplifies no frequency by more than 1 / (2 sqrt(balance)) = 5 per unit of the Laplacian's transfer,
    # so the 16-bit outputs stay within 5 x the gate x full scale
    dist = float(np.abs(psf_h.astype(np.float64) - psf_d).sum(axis=(0, 1)).max())
    out_diff = float(np.abs(host.astype(np.float64) - dev).max())
    print("driver, host frames against resident frames: L1 of the PSFs %.6f (gate %.6f), max |out| difference %.2f of 65535" % (dist, er.BLIND_GATE, out_diff))
    assert host.shape == dev.shape == (160, 192, 3)
    assert dist <= er.BLIND_GATE
    assert out_diff <= 5 * er.BLIND_GATE * 65535
    n3 = run_driver(blind=("fast", 3), nonblind="wiener")
    assert n3[2].count("Level : PSF") == 3 and not np.array_equal(n3[1], psf_d)
    import deconvolve
    for kw in (dict(blind="slow"), dict(blind=("fast", 0)), dict(blind=("fast", 2.5)), dict(blind="fast", blur="motion")):
        with pytest.raises(ValueError):
            run_driver(nonblind="wiener", **kw)


def test_blind_rl_is_the_call_without_the_argument():
    for resident in (True, False):
        a = run_driver(nonblind="wiener", device_resident=resident)
        b = run_driver(blind="rl", nonblind="wiener", device_resident=resident)
        import re
        untimed = lambda text: re.sub(r"[0-9.]+ sec", "sec", text)           # (the solver prints its wall time)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and untimed(a[2]) == untimed(b[2])
        assert "===== blind DECONVOLUTION =====" in a[2] and "FAST BLIND" not in a[2]
