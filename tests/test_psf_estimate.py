"""CPU: the specification of DeviceImage.psf_raw / lib.utils.estimate_psf (tests/psf_est_ref.py) does what it is for -- it recovers box
PSFs from a sharp / blurred pair and keeps their orientation --, its float32 evaluation stays within a quarter of the GPU gate at every
GPU shape, and the layers above the kernels (argument checks, the projection, the plan, the C entries and the header) hold what
include/ics_hip.h and lib/_native.py state.  tests/test_gpu_psf_estimate.py gates the kernels against the specification."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import psf_est_ref as pr
import wiener_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_projected_estimate_is_close_to_the_true_box():
    """with the true sharp frame and noise of sigma 0.002, at the defaults: within L1 0.1 of the box, about twice the worst value
    measured when the method was chosen (0.045)"""
    for sharp, blurred, k in pr.quality_cases():
        K = k.shape[0]
        est = pr.estimate(blurred, sharp, K)
        assert est.shape == (K, K, 3) and np.abs(est.sum(axis=(0, 1)) - 1).max() < 1e-12
        d = max(np.abs(est[..., c] - k[..., c]).sum() for c in range(3))
        print("box of %d px on %s: L1 to the true PSF %.4f" % (K, sharp.shape[:2], d))
        assert d <= 0.1


def test_the_orientation_is_that_of_a_true_convolution():
    """a 160 x 192 dead-leaves frame cut from a larger one, blurred by three_psfs(15) as true convolutions: every channel's estimate is
    at least five times closer to its own PSF than to that PSF flipped in both axes, for the off-centre L-shaped channel"""
    K = 15
    rng = np.random.default_rng(7)
    big = pr.dead_leaves(rng, 160 + 2 * K, 192 + 2 * K)
    k = pr.three_psfs(K)
    blurred = pr.blurred_by(big, k, K, rng)
    est = pr.estimate(blurred, big[K:-K, K:-K], K, coupling="channel")
    own = [np.abs(est[..., c] - k[..., c]).sum() for c in range(3)]
    flipped = np.abs(est[..., 2] - k[::-1, ::-1, 2]).sum()
    print("L1 to the own PSF (box, Gaussian, L): %.3f %.3f %.3f; the L to its flipped copy: %.3f" % (*own, flipped))
    assert 5 * own[2] <= flipped
    for c in range(3):                                               # no channel took another one's kernel
        assert own[c] == min(np.abs(est[..., c] - k[..., o]).sum() for o in range(3))


@pytest.mark.parametrize("shape,K", pr.GPU_CASES)
def test_the_float32_evaluation_stays_within_a_quarter_of_the_gate(shape, K):
    s, b = pr.gpu_pair(shape, K)
    worst = 0.0
    for regularisation in pr.REGULARISATIONS:
        for coupling in pr.COUPLINGS:
            ref, S = pr.gpu_reference(shape, K, regularisation, coupling)
            raw, _ = pr.raw_kernel(b, s, K, regularisation, coupling, dtype=np.float32)
            assert raw.dtype == np.float32 and (S > 0).all()
            worst = max(worst, np.abs(raw - ref).max() / np.abs(ref).max())
    print("%s K %d: float32 against float64, %.3g of the peak" % (shape, K, worst))
    assert worst <= pr.GATE / 4


def test_psf_estimate_args():
    from lib import _native
    ok = _native.psf_estimate_args
    shape = (70, 150, 3)
    assert ok(9, 1e-3, 0.05, "vector", None, shape, shape) == (9, 1e-3, 0.05, "vector", (0, 70, 0, 150))
    assert ok(np.int64(255), 1, 0, "channel", (3, 260, 5, 300), (300, 300, 3), (300, 300)) == (255, 1.0, 0.0, "channel", (3, 260, 5, 300))
    assert ok(3, 1e-3, 0.999, "vector", (0.0, 3.0, 0, 3), shape, shape)[4] == (0, 3, 0, 3)
    bad = [dict(shape_sharp=(70, 149, 3)), dict(shape_blurred=(69, 150, 3)),                                  # frames of different shapes
           dict(size=8), dict(size=1), dict(size=257), dict(size=9.5), dict(size="9"), dict(size=True),      # K even, outside 3 .. 255, no integer
           dict(size=71), dict(size=11, window=(0, 10, 0, 150)),                                             # K above the frame, above the window
           dict(window=(0, 0, 0, 150)), dict(window=(10, 5, 0, 150)), dict(window=(-1, 70, 0, 150)),         # an empty window, a negative corner
           dict(window=(0, 71, 0, 150)), dict(window=(0, 70, 0, 151)),                                       # a window not inside the frames
           dict(window=(0, 70, 0)), dict(window=(0.5, 70, 0, 150)), dict(window="all"),
           dict(regularisation=0), dict(regularisation=-1e-3), dict(regularisation=float("nan")), dict(regularisation=float("inf")),
           dict(regularisation="x"), dict(regularisation=1e-60),                                             # (0 as float32)
           dict(threshold=1), dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold="x"), dict(threshold=None),
           dict(coupling="both"), dict(coupling=1)]
    for change in bad:
        kw = dict(size=9, regularisation=1e-3, threshold=0.05, coupling="vector", window=None, shape_blurred=shape, shape_sharp=shape)
        kw.update(change)
        with pytest.raises(ValueError):
            print("refused:", change)
            ok(**kw)
    # a window inside the blurred frame only: the frames differ, refused
    with pytest.raises(ValueError):
        ok(9, 1e-3, 0.05, "vector", (0, 70, 0, 150), (70, 150, 3), (60, 150, 3))


def test_psf_project():
    from lib import _native
    rng = np.random.default_rng(3)
    raw = rng.normal(0.0, 0.02, (7, 7, 3))
    raw[3, 3] += 1.0
    raw[2, 4] += 0.5
    psf, rejected = _native.psf_project(raw, 0.05)
    ref, rej = pr.project(raw, 0.05)
    assert psf.dtype == np.float32 and psf.shape == (7, 7, 3) and len(rejected) == 3 and all(isinstance(v, float) for v in rejected)
    assert np.array_equal(psf, ref.astype(np.float32)) and np.allclose(rejected, rej, rtol=1e-12, atol=0)
    assert np.abs(psf.astype(np.float64).sum(axis=(0, 1)) - 1).max() < 1e-6 and (psf >= 0).all()
    for c in range(3):
        m = raw[..., c].max()
        kept = raw[..., c] >= 0.05 * m
        assert np.array_equal(psf[..., c] > 0, kept)                                       # exactly the taps at or above the threshold stay
        assert abs(rejected[c] - np.abs(raw[..., c][~kept]).sum() / np.abs(raw[..., c]).sum()) < 1e-15
    # threshold 0 cuts the negative taps and nothing else
    p0, r0 = _native.psf_project(raw, 0.0)
    assert np.array_equal(p0 > 0, raw > 0) and all(v > 0 for v in r0)
    # a plane with a single positive tap comes back as that tap = 1
    one = np.full((5, 5, 3), -0.25)
    one[1, 3] = 0.125
    p1, r1 = _native.psf_project(one, 0.5)
    assert np.array_equal(p1[1, 3], [1, 1, 1]) and p1.sum() == 3 and np.allclose(r1, 6.0 / 6.125)
    for poison in (np.nan, np.inf, -np.inf):
        broken = raw.copy()
        broken[0, 0, 1] = poison
        with pytest.raises(ValueError, match="not finite") as ei:
            _native.psf_project(broken, 0.05)
        assert "despeckle first" in str(ei.value)
    for flat in (np.zeros((3, 3, 3)), -np.ones((3, 3, 3))):
        with pytest.raises(ValueError, match="no positive tap"):
            _native.psf_project(flat, 0.05)
    with pytest.raises(ValueError):
        _native.psf_project(np.ones((3, 5, 3)), 0.05)
    with pytest.raises(ValueError):
        _native.psf_project(np.ones((3, 3, 3)), 1.0)


def test_plan():
    from lib import _native
    for (H, W), K in pr.GPU_CASES + [((4096, 4096), 15), ((1023, 1023), 31)]:
        plan = _native.psf_estimate_plan(H, W, K)
        assert (plan.Py, plan.Px) == wr.sizes(H, W, K) and plan._fields == ("Py", "Px", "workspace_bytes")
        # twelve complex planes, the K rows that leave the solve, the twiddles, the energies, the tapers, the row slots, the raw kernel
        assert plan.workspace_bytes == 8 * (12 * plan.Py * plan.Px + 3 * K * plan.Px + plan.Py + plan.Px) + 32 + 4 * (H + W + 6 * H + 3 * K * K)
    for H, W, K in ((16, 8192, 3), (8192, 16, 3), (8171, 24, 23)):
        with pytest.raises(_native.NativeError) as ei:
            _native.psf_estimate_plan(H, W, K)
        assert ei.value.code == _native.ICS_ENOSUP == -6 and "8192" in str(ei.value)
    for H, W, K in ((40, 52, 4), (40, 52, 1), (300, 300, 257), (40, 52, 41), (52, 40, 41), (0, 52, 3)):
        with pytest.raises(_native.NativeError) as ei:
            _native.psf_estimate_plan(H, W, K)
        assert ei.value.code == _native.ICS_EINVAL == -1


def test_entries_and_header():
    from lib import _native
    lib = _native.load()
    cf, cd, ci, vp = C.c_float, C.c_double, C.c_int, C.c_void_p
    assert lib.ics_img_psf_estimate.argtypes == [vp, vp, ci, ci, ci, ci, ci, cf, ci, C.POINTER(cf), C.POINTER(cd)]
    assert lib.ics_img_psf_estimate_plan.argtypes == [ci, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_size_t)]
    assert lib.ics_img_psf_estimate.restype is ci and lib.ics_img_psf_estimate_plan.restype is ci
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    assert ("int ics_img_psf_estimate(const ics_img *blurred, const ics_img *sharp, int y0, int y1, int x0, int x1, int K,\n"
            "                         float regularisation, int coupling, float *raw /* K*K*3 */, double energy[3]);\n"
            "int ics_img_psf_estimate_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);\n") in header
    assert re.search(r"#define ICS_ABI_VERSION 4\b", header) and lib.ics_abi_version() == 4
    # the native entry refuses by itself, before it touches a frame, what the Python layer refuses before it
    fake = vp(1)
    raw, energy = (cf * 27)(), (cd * 3)()
    good = dict(blurred=fake, sharp=fake, y0=0, y1=40, x0=0, x1=52, K=3, regularisation=1e-3, coupling=1, raw=raw, energy=energy)
    bad = [dict(blurred=None), dict(sharp=None), dict(raw=None), dict(energy=None),
           dict(y1=0), dict(y0=40), dict(x0=52, x1=52), dict(x0=60), dict(y0=-1), dict(x0=-1),
           dict(K=4), dict(K=1), dict(K=257, y1=300, x1=300), dict(K=41), dict(K=5, y0=36),
           dict(regularisation=0.0), dict(regularisation=-1.0), dict(regularisation=float("nan")), dict(regularisation=float("inf")),
           dict(coupling=2), dict(coupling=-1)]
    for change in bad:
        args = dict(good, **change)
        assert lib.ics_img_psf_estimate(*args.values()) == _native.ICS_EINVAL, change
    assert lib.ics_img_psf_estimate(*dict(good, y1=16, x1=8192).values()) == _native.ICS_ENOSUP and b"8192" in lib.ics_last_error()
    for name in ("psf_estimate_args", "psf_estimate_plan", "psf_project", "PsfEstimatePlan"):
        assert hasattr(_native, name), name
    assert hasattr(_native.DeviceImage, "psf_raw")


def test_utils_estimate_psf_has_no_cpu_fallback():
    from lib import _native, utils
    assert utils.PsfEstimate._fields == ("psf", "raw", "rejected")
    z = np.zeros((10, 12, 3))
    for args, kw in [((z, z, 4), {}), ((z, z, 11), {}), ((z, z[:9], 3), {}), ((z, z, 3), dict(regularisation=0)), ((z, z, 3), dict(threshold=1)),
                     ((z, z, 3), dict(coupling="rgb")), ((z, z, 3), dict(window=(0, 11, 0, 12))), ((z[..., 0], z[..., 0], 3), {}), ((z, z[..., :2], 3), {})]:
        with pytest.raises(ValueError):                               # refused before anything is uploaded
            utils.estimate_psf(*args, **kw)
    if _native.device_count() == 0:
        with pytest.raises(_native.NativeError) as ei:
            utils.estimate_psf(z, z, 3)
        assert ei.value.code == _native.ICS_ENODEV
