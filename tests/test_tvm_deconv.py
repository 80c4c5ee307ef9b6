"""CPU: the specification of the TV deconvolution with a masked data term (tests/tvm_deconv_ref.py) keeps a constant frame, follows a
permutation of the channels, ignores what stands at non-finite pixels, is not tests/tv_deconv_ref.py under another name, beats it by
the unknown edges alone in the three quality cases and near clipped lights from 30 iterations; its float32 evaluation stays within a
quarter of the GPU gate at every GPU case; and the host layers above the kernels (lib._native.tv_deconvolve_masked_args /
tv_deconvolve_masked_plan, deconvolve._nonblind_args, lib.utils.tv_deconvolve_masked) accept and refuse what they state.  The GPU side:
tests/test_gpu_tvm_deconv.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import tv_deconv_ref as tr
import tvm_deconv_ref as tm
import wiener_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = ("none", "clip", "array")
BIG = ((24, 8170), (8170, 24))                               # the full LDS line: 3 iterations
# shape, K, coupling, mask form, data_penalty, non-finite pixels
GPU_CASES = [(shape, K, coupling, mask, 200.0 if shape == (61, 61) else None, False)
             for shape, K in wr.GPU_SHAPES for coupling in tm.COUPLINGS for mask in MASKS]
GPU_CASES += [((40, 52), 5, "vector", "array", None, True)]


def rms(a):
    return float(np.sqrt((a ** 2).mean()))


def gate(ref):
    return wr.GATE * max(1.0, float(np.abs(ref).max()))


def normalised(k):
    """what tv_deconvolve_masked_args hands to the library"""
    k64 = k.astype(np.float64)
    return (k64 / k64.sum(axis=(0, 1))).astype(np.float32)


def iterations_of(shape):
    return 3 if shape in BIG else tm.ITERATIONS


def mask_of(form, H, W):
    """(observed, clip) of a mask form: nothing, the clip alone, or an array with nine in ten pixels kept and, where the frame holds
    them, one 9 x 9 block, one whole row and one whole column out"""
    if form == "none":
        return None, None
    if form == "clip":
        return None, 0.99
    m = np.random.default_rng(1).random((H, W)) > 0.1
    if H >= 12 and W >= 12:
        m[2:11, 3:12] = False
    if H >= 3:
        m[H // 2, :] = False
    if W >= 3:
        m[:, W // 3] = False
    return m.astype(np.uint8), None


@functools.lru_cache(maxsize=None)
def gpu_case(shape, K, coupling, mask, data_penalty=None, nonfinite=False):
    """frame, PSF, observed, clip, iterations and the float64 reference (out, unobserved) of one GPU case (shared with
    tests/test_gpu_tvm_deconv.py)"""
    H, W = shape
    f = wr.frame(H, W, seed=H * 10007 + W).astype(np.float32)
    if nonfinite:
        f[3, 4, 0] = f[20, 30, 1] = f[39, 51, 2] = np.nan
        f[10, 10, 1] = np.inf
        f[0, 0, 2] = -np.inf
    k = wr.three_psfs(K).astype(np.float32)
    observed, clip = mask_of(mask, H, W)
    n = iterations_of(shape)
    ref, count = tm.tv_deconvolve_masked(f.astype(np.float64), normalised(k).astype(np.float64), observed, clip, tm.FIDELITY, tm.PENALTY, data_penalty, n, coupling)
    for a in (f, k, ref) + (() if observed is None else (observed,)):
        a.setflags(write=False)
    return f, k, observed, clip, n, ref, count


# ---- the specification ------------------------------------------------------------------------------------------------------------------
def test_a_constant_frame_comes_back_constant_with_a_random_mask_too():
    f = np.full((33, 47, 3), 0.37)
    m = np.random.default_rng(3).random((33, 47)) > 0.3
    for coupling in tm.COUPLINGS:
        for observed in (None, m):
            out, n = tm.tv_deconvolve_masked(f, wr.three_psfs(7), observed, coupling=coupling)
            assert np.abs(out - 0.37).max() <= 1e-12
            assert n == (0 if observed is None else int((~m).sum()))


def test_permuting_the_channels_permutes_the_output():
    f, k = wr.frame(40, 52, 7), wr.three_psfs(5)
    m = np.random.default_rng(4).random((40, 52)) > 0.2
    perm = [2, 0, 1]
    for coupling in tm.COUPLINGS:
        a, na = tm.tv_deconvolve_masked(f, k, m, 0.9, coupling=coupling)
        b, nb = tm.tv_deconvolve_masked(f[..., perm], k[..., perm], m, 0.9, coupling=coupling)
        assert na == nb and np.abs(a[..., perm] - b).max() <= 1e-12


def test_what_stands_at_a_non_finite_pixel_does_not_matter():
    f, k = wr.frame(40, 52, 7), wr.three_psfs(5)
    a, b = f.copy(), f.copy()
    a[5, 6, 0], a[20, 30, 1], a[0, 0, 2], a[39, 51, 0] = np.nan, np.inf, -np.inf, np.nan
    b[5, 6, 0], b[20, 30, 1], b[0, 0, 2], b[39, 51, 0] = np.inf, np.nan, np.nan, -np.inf
    ra, na = tm.tv_deconvolve_masked(a, k)
    rb, nb = tm.tv_deconvolve_masked(b, k)
    assert na == nb == 4 and np.isfinite(ra).all() and np.array_equal(ra, rb)


def test_it_is_not_the_unmasked_method_under_another_name():
    f, k = wr.frame(40, 52, 7), wr.three_psfs(5)
    for coupling in tm.COUPLINGS:
        assert np.abs(tm.tv_deconvolve_masked(f, k, None, None, coupling=coupling)[0] - tr.tv_deconvolve(f, k, coupling=coupling)).max() > 1e-3


PINNED = {"vector": (0.0333, 0.0501, 0.0740), "channel": (0.0342, 0.0516, 0.0774)}      # recomputed by this test, four digits


def test_the_unknown_edges_alone_lower_the_error_in_the_three_quality_cases():
    for i, (sharp, blurred, psf) in enumerate(wr.quality_cases()):
        for coupling in tm.COUPLINGS:
            plain = rms(tr.tv_deconvolve(blurred, psf, coupling=coupling) - sharp)
            out, n = tm.tv_deconvolve_masked(blurred, psf, coupling=coupling)
            masked = rms(out - sharp)
            print("%s %s: blurred %.4f, tv %.4f, tv-masked %.4f (%.1f %% lower)" % (blurred.shape[:2], coupling, rms(blurred - sharp), plain, masked,
                                                                                   100 * (1 - masked / plain)))
            assert n == 0 and masked <= 0.95 * plain
            assert "%.4f" % masked == "%.4f" % PINNED[coupling][i]


def test_twenty_missing_pixels_are_simply_not_data():
    sharp, blurred, psf = wr.quality_cases()[1]
    rng = np.random.default_rng(11)
    holed = blurred.copy()
    holed[rng.integers(0, 70, 20), rng.integers(0, 150, 20), rng.integers(0, 3, 20)] = np.nan
    out, n = tm.tv_deconvolve_masked(holed, psf)
    whole, _ = tm.tv_deconvolve_masked(blurred, psf)
    print("70 x 150: rms %.4f whole, %.4f with %d pixels missing" % (rms(whole - sharp), rms(out - sharp), n))
    assert 1 <= n <= 20 and np.isfinite(out).all() and rms(out - sharp) <= rms(whole - sharp) + 5e-4


def clipped_lights():
    """six 3 x 3 lights of value 8 under the 15-px box of the third quality case, clipped at 1: truth, frame, PSF, the ring where the
    error is read (within 12 px of a clipped pixel, the clipped pixels and their neighbours left out)"""
    from scipy.ndimage import binary_dilation, convolve
    sharp, _, psf = wr.quality_cases()[2]
    rng = np.random.default_rng(5)
    big = np.pad(sharp, ((15, 15), (15, 15), (0, 0)), mode="edge")
    for _ in range(6):
        cy = rng.integers(30, 160)
        cx = rng.integers(30, 190)
        big[cy:cy + 3, cx:cx + 3] = 8
    blurred = np.dstack([convolve(big[..., c], psf[..., c], mode="nearest") for c in range(3)])[15:-15, 15:-15]
    frame = np.minimum(blurred + rng.normal(0, 0.002, blurred.shape), 1)
    sat = (frame >= 0.99).any(axis=2)
    ring = binary_dilation(sat, iterations=12) & ~binary_dilation(sat, iterations=1)
    return big[15:-15, 15:-15], frame, psf, ring


def test_near_clipped_lights_the_mask_pays_at_30_iterations():
    truth, frame, psf, ring = clipped_lights()

    def near(u):
        return rms((np.clip(u, 0, 1) - np.clip(truth, 0, 1))[ring])

    with_clip, n = tm.tv_deconvolve_masked(frame, psf, clip=0.99, iterations=30)
    without, _ = tm.tv_deconvolve_masked(frame, psf, clip=None, iterations=30)
    print("rms near the lights: blurred %.4f, 30 iterations without clip %.4f, with clip 0.99 %.4f (%d pixels out)" % (near(frame), near(without), near(with_clip), n))
    assert n > 0 and near(with_clip) <= 0.95 * near(without)


# ---- float32 against float64 at the GPU cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,coupling,mask,data_penalty,nonfinite", GPU_CASES)
def test_float32_evaluation_is_within_a_quarter_of_the_gate(shape, K, coupling, mask, data_penalty, nonfinite):
    f, k, observed, clip, n, ref, count = gpu_case(shape, K, coupling, mask, data_penalty, nonfinite)
    got, count32 = tm.tv_deconvolve_masked(f, normalised(k), observed, clip, tm.FIDELITY, tm.PENALTY, data_penalty, n, coupling, np.float32)
    assert got.dtype == np.float32 and count32 == count
    err, bound = float(np.abs(got - ref).max()), 0.25 * gate(ref)
    print("float32 - float64: %.3g (bound %.3g, max |ref| %.3g, %d unobserved)" % (err, bound, np.abs(ref).max(), count))
    assert err <= bound


# ---- the host layers ------------------------------------------------------------------------------------------------------------------------------
def test_tv_deconvolve_masked_args_accepts_and_refuses_what_it_states():
    from lib import _native
    ok = np.ones((40, 52))
    ok[3, 4] = 0
    k, m, clip, mu, beta, gamma, n, coupling = _native.tv_deconvolve_masked_args(2.0 * np.ones((5, 5)), 7 * ok, 0.99, 2000, 10, None, 10, "vector", (40, 52, 3))
    assert np.array_equal(k, _native.tv_deconvolve_args(2.0 * np.ones((5, 5)), 2000, 10, 10, "vector", (40, 52, 3))[0])
    assert m.dtype == np.uint8 and m.flags.c_contiguous and np.array_equal(m, ok.astype(np.uint8))
    assert (clip, mu, beta, gamma, n, coupling) == (0.99, 2000.0, 10.0, 2000.0, 10, "vector") and isinstance(clip, float) and isinstance(gamma, float)
    got = _native.tv_deconvolve_masked_args(np.ones((3, 3)), None, None, 1, 1, 3, 500, "channel", (3, 3))
    assert got[1] is None and got[2:] == (float("inf"), 1.0, 1.0, 3.0, 500, "channel")
    assert _native.tv_deconvolve_masked_args(np.ones((3, 3)), None, np.inf, 1, 1, None, 1, "channel", (3, 3))[2] == float("inf")
    assert _native.tv_deconvolve_masked_args(np.ones((3, 3)), ok > 0, 2, 1, 1, None, 1, "channel", (40, 52))[1].sum() == 40 * 52 - 1

    def refused(psf=np.ones((3, 3)), observed=None, clip=None, fidelity=2000, penalty=10, data_penalty=None, iterations=10, coupling="vector", shape=(6, 300, 3)):
        with pytest.raises(ValueError):
            _native.tv_deconvolve_masked_args(psf, observed, clip, fidelity, penalty, data_penalty, iterations, coupling, shape)

    for observed in (np.ones((6, 299)), np.ones((300, 6)), np.ones((6, 300, 3)), np.ones(6 * 300), np.zeros((6, 300)), 1):
        refused(observed=observed)
    for clip in (0, -1, np.nan, -np.inf, "x", "0.99"):
        refused(clip=clip)
    for data_penalty in (0, -1, np.nan, np.inf, "x"):
        refused(data_penalty=data_penalty)
    # every refusal of tv_deconvolve_args
    for psf in [np.ones((4, 4)), np.ones((1, 1)), np.ones((257, 257)), np.ones((3, 5)), np.ones((3, 3, 2)), np.ones(3), np.ones((7, 7)), np.full((3, 3), np.nan),
                np.full((3, 3), np.inf), np.zeros((3, 3)), -np.ones((3, 3)), np.dstack([np.ones((3, 3)), np.ones((3, 3)), np.zeros((3, 3))]), "box"]:
        refused(psf=psf)
    for v in (0, -1, np.nan, np.inf, "x"):
        refused(fidelity=v)
        refused(penalty=v)
    for n in (0, -1, 2.5, 501, "x"):
        refused(iterations=n)
    for coupling in ("luma", None, 1):
        refused(coupling=coupling)


def test_tv_deconvolve_masked_plan_returns_the_sizes_and_the_documented_bytes():
    from lib import _native
    for H, W, K in [(5, 7, 3), (40, 52, 5), (60, 60, 5), (61, 61, 5), (70, 150, 9), (16, 2040, 9), (8170, 24, 23), (4096, 4096, 15), (4000, 6000, 45), (8190, 8190, 3)]:
        plan = _native.tv_deconvolve_masked_plan(H, W, K)
        wplan = _native.wiener_plan(H, W, K)
        assert (plan.Py, plan.Px) == wr.sizes(H, W, K) == tuple(wplan[:2])
        points = plan.Py * plan.Px
        tables = wplan.workspace_bytes - 2 * 3 * 8 * points           # the Wiener filter's block is two spectrum frames and the tables
        assert tables > 0
        # 14 1/3 floats per transform point and channel, the row counts and the total, a byte per point for the mask, the tables
        assert plan.workspace_bytes == 4 * (43 * points + plan.Py + 4) + points + tables
        assert plan.workspace_bytes <= 16 * 4 * 3 * points + tables
    for H, W, K in [(16, 8192, 3), (8192, 16, 3), (8171, 24, 23)]:
        with pytest.raises(_native.NativeError) as ei:
            _native.tv_deconvolve_masked_plan(H, W, K)
        assert ei.value.code == -6 and "8192" in str(ei.value)        # ICS_ENOSUP, the message names the limit
    for H, W, K in [(40, 52, 4), (40, 52, 1), (40, 52, 257), (4, 52, 5), (40, 4, 5), (0, 5, 3)]:
        with pytest.raises(_native.NativeError) as ei:
            _native.tv_deconvolve_masked_plan(H, W, K)
        assert ei.value.code == -1


def test_the_two_entries_exist_with_their_signatures():
    from lib import _native
    lib = _native.load()
    assert len(lib.ics_img_tv_deconvolve_masked.argtypes) == 12 and len(lib.ics_img_tv_deconvolve_masked_plan.argtypes) == 6
    assert lib.ics_img_tv_deconvolve_masked.restype is C.c_int and lib.ics_img_tv_deconvolve_masked_plan.restype is C.c_int
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    assert ("int ics_img_tv_deconvolve_masked(const ics_img *src, const float *psf, int K, const unsigned char *observed, float clip, float fidelity, "
            "float penalty, float data_penalty, int iterations, int coupling, long long *unobserved, ics_img **out);") in header
    assert "int ics_img_tv_deconvolve_masked_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);" in header
    assert "#define ICS_IMG_TVD_MAX_ITERATIONS 500" in header and _native.IMG_TVD_MAX_ITERATIONS == 500
    assert lib.ics_abi_version() == 4
    # the native entry refuses by itself what the Python layer refuses before it
    out = C.c_void_p()
    fake = C.c_void_p(1)
    psf = (C.c_float * 27)(*([1 / 9] * 27))
    inf = float("inf")
    for args in [(0.0, 2000.0, 10.0, 2000.0, 10, 1), (float("nan"), 2000.0, 10.0, 2000.0, 10, 1), (-1.0, 2000.0, 10.0, 2000.0, 10, 1), (inf, 0.0, 10.0, 2000.0, 10, 1),
                 (inf, 2000.0, inf, 2000.0, 10, 1), (inf, 2000.0, 10.0, 0.0, 10, 1), (inf, 2000.0, 10.0, float("nan"), 10, 1), (inf, 2000.0, 10.0, 2000.0, 0, 1),
                 (inf, 2000.0, 10.0, 2000.0, 501, 1), (inf, 2000.0, 10.0, 2000.0, 10, 2)]:
        assert lib.ics_img_tv_deconvolve_masked(fake, psf, 3, None, *args, None, C.byref(out)) == _native.ICS_EINVAL, args
    assert lib.ics_img_tv_deconvolve_masked(None, psf, 3, None, inf, 2000.0, 10.0, 2000.0, 10, 1, None, C.byref(out)) == _native.ICS_EINVAL


def test_nonblind_args_takes_the_masked_forms_and_keeps_every_old_answer():
    import deconvolve as dv
    assert dv._nonblind_args("rl") is None
    assert dv._nonblind_args("wiener") == 0.01
    assert dv._nonblind_args(("wiener", 0.1)) == 0.1
    assert dv._nonblind_args("tv") == ("tv", 2000.0, 10, "vector")
    assert dv._nonblind_args(("tv", 500)) == ("tv", 500.0, 10, "vector")
    assert dv._nonblind_args(["tv", 500, 20]) == ("tv", 500.0, 20, "vector")
    assert dv._nonblind_args(("tv", 1e4, 3, "channel")) == ("tv", 1e4, 3, "channel")
    assert dv._nonblind_args("tv-masked") == ("tv-masked", 2000.0, 10, "vector", 0.99)
    assert dv._nonblind_args(("tv-masked", 500)) == ("tv-masked", 500.0, 10, "vector", 0.99)
    assert dv._nonblind_args(["tv-masked", 500, 30]) == ("tv-masked", 500.0, 30, "vector", 0.99)
    assert dv._nonblind_args(("tv-masked", 1e4, 3, "channel")) == ("tv-masked", 1e4, 3, "channel", 0.99)
    assert dv._nonblind_args(("tv-masked", 1e4, 3, "channel", 0.9)) == ("tv-masked", 1e4, 3, "channel", 0.9)
    assert dv._nonblind_args(("tv-masked", 1e4, 3, "channel", None)) == ("tv-masked", 1e4, 3, "channel", float("inf"))
    for bad in (("tv", 0), ("tv", 2000, 0), ("tv", 2000, 10, "x"), ("tv", 2000, 10, "vector", 1), "TV", ("tv",), ("tv", np.nan), ("tv", 2000, 2.5), ("tv", 2000, 501),
                ("wiener", 0), ("wiener", 0.1, 1), "tv_masked", ("tv-masked",), ("tv-masked", 0), ("tv-masked", 2000, 0), ("tv-masked", 2000, 10, "x"),
                ("tv-masked", 2000, 10, "vector", 0), ("tv-masked", 2000, 10, "vector", 0.99, 1), ("tv-masked", np.nan), None, 3):
        with pytest.raises(ValueError):
            dv._nonblind_args(bad)
    with pytest.raises(ValueError):                                   # refused before the picture is touched
        dv.deblur_module(None, "x", ".", 5, nonblind=("tv-masked", -1))


def test_utils_tv_deconvolve_masked_has_no_cpu_fallback():
    from lib import _native, utils
    with pytest.raises(ValueError):                                   # refused before anything is uploaded
        utils.tv_deconvolve_masked(np.zeros((10, 10, 3)), np.ones((4, 4)))
    with pytest.raises(ValueError):
        utils.tv_deconvolve_masked(np.zeros((10, 10, 3)), np.ones((3, 3)), observed=np.zeros((10, 10)))
    with pytest.raises(ValueError):
        utils.tv_deconvolve_masked(np.zeros((10, 10, 3)), np.ones((3, 3)), clip=0)
    with pytest.raises(ValueError):
        utils.tv_deconvolve_masked(np.zeros((10, 10)), np.ones((3, 3)))
    if _native.device_count() == 0:
        with pytest.raises(_native.NativeError) as ei:
            utils.tv_deconvolve_masked(np.zeros((10, 10, 3)), np.ones((3, 3)), clip=0.99)
        assert ei.value.code == _native.ICS_ENODEV
