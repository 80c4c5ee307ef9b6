"""CPU: the specification of the Wiener filter (tests/wiener_ref.py) has the properties that fix its conventions, its float32
evaluation stays within a quarter of the GPU gate at every GPU shape, it improves on the blurred frame in the three quality cases,
and the host layers above the kernels (lib._native.wiener_args / wiener_plan, deconvolve._nonblind_args, lib.utils.wiener) accept and
refuse what they state.  The GPU side: tests/test_gpu_wiener.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import wiener_ref as wr


# ---- the specification ------------------------------------------------------------------------------------------------------------------
def test_a_constant_frame_comes_back_constant():
    f = np.full((33, 47, 3), 0.37)
    out = wr.wiener(f, wr.three_psfs(7), 0.01)
    assert np.abs(out - 0.37).max() <= 1e-12


def test_linear_in_the_frame():
    a, b, k = wr.frame(31, 45, 1), wr.frame(31, 45, 2), wr.three_psfs(5)
    lhs = wr.wiener(2.0 * a - 3.0 * b, k, 0.01)
    rhs = 2.0 * wr.wiener(a, k, 0.01) - 3.0 * wr.wiener(b, k, 0.01)
    assert np.abs(lhs - rhs).max() <= 1e-12 * max(1.0, np.abs(rhs).max())


def test_permuting_the_channels_of_frame_and_psf_permutes_the_output():
    f, k, perm = wr.frame(31, 45, 3), wr.three_psfs(5), [2, 0, 1]
    assert np.array_equal(wr.wiener(f[..., perm], k[..., perm], 0.01), wr.wiener(f, k, 0.01)[..., perm])


def test_a_psf_shifted_by_one_tap_shifts_the_result_the_other_way():
    """the signs of the roll and of the conjugate: with a PSF whose weight sits one tap further down (right), the restored picture sits
    one pixel further up (left) -- exactly so on the whole transform, where the shift is circular, and on the cropped result away
    from the last row; and a point that a true convolution with that PSF has moved down comes back to where it was"""
    K = 5
    core = np.zeros((K, K))
    core[1:4, 1:4] = [[1, 2, 1], [2, 4, 2], [1, 2, 1]]
    down = np.roll(core, 1, axis=0)                         # the same kernel, its weight one tap down (nothing wraps: row 4 was empty)
    right = np.roll(core, 1, axis=1)
    f = wr.frame(60, 60, 4)
    Py, Px = wr.sizes(60, 60, K)
    ext = wr.extend(wr.extend(f, Py, 0), Px, 1)
    lam = wr.laplacian(Py, Px)

    def full(k):                                            # step 5 on the whole transform, before the crop
        Hc = wr.psf_spectrum(k / k.sum(), Py, Px)
        return np.fft.ifft2(np.conj(Hc) / (np.abs(Hc) ** 2 + 0.01 * lam ** 2) * np.fft.fft2(ext[..., 0])).real

    base = full(core)
    assert np.abs(full(down) - np.roll(base, -1, axis=0)).max() <= 1e-12
    assert np.abs(full(right) - np.roll(base, -1, axis=1)).max() <= 1e-12
    # and through the public function, away from the rows the crop cuts
    k3 = lambda k: np.dstack([k / k.sum()] * 3)             # noqa: E731
    a, b = wr.wiener(f, k3(core), 0.01), wr.wiener(f, k3(down), 0.01)
    assert np.abs(b[:-1] - a[1:]).max() <= 1e-12
    # a true convolution with `down` moves a point down; the filter moves it back
    from scipy.ndimage import convolve
    point = np.zeros((41, 41))
    point[20, 20] = 1.0
    moved = convolve(point, down / down.sum(), mode="constant")
    assert np.unravel_index(moved.argmax(), moved.shape) == (21, 20)
    back = wr.wiener(np.dstack([moved] * 3), k3(down), 1e-4)[..., 0]
    assert np.unravel_index(back.argmax(), back.shape) == (20, 20)


def test_a_delta_psf_is_a_low_pass_not_the_identity():
    f = wr.frame(33, 47, 5)
    d = np.zeros((3, 3, 3))
    d[1, 1] = 1
    out = wr.wiener(f, d, 0.01)
    assert 1e-3 < np.abs(out - f).max() < 0.5


def test_the_extension_is_a_ramp_back_to_the_first_entry():
    f = np.arange(5.0).reshape(5, 1, 1) * np.ones((1, 2, 3))
    e = wr.extend(f, 8, 0)                                  # g = 4: 4 -> 3, 2, 1 -> (0)
    assert e.shape == (8, 2, 3) and np.allclose(e[:, 0, 0], [0, 1, 2, 3, 4, 3, 2, 1])


# ---- float32 against float64 at the GPU shapes ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_case(shape, K, balance):
    """frame, PSF and the float64 reference of one GPU case (shared with tests/test_gpu_wiener.py)"""
    f = wr.frame(shape[0], shape[1], seed=shape[0] * 10007 + shape[1]).astype(np.float32)
    k = wr.three_psfs(K).astype(np.float32)
    k64 = k.astype(np.float64)
    k64 = k64 / k64.sum(axis=(0, 1))                        # what wiener_args hands to the library, before its rounding
    ref = wr.wiener(f.astype(np.float64), k64.astype(np.float32).astype(np.float64), balance)
    ref.setflags(write=False)
    f.setflags(write=False)
    k.setflags(write=False)
    return f, k, ref


@pytest.mark.parametrize("balance", wr.BALANCES)
@pytest.mark.parametrize("shape,K", wr.GPU_SHAPES)
def test_float32_evaluation_is_within_a_quarter_of_the_gate(shape, K, balance):
    f, k, ref = gpu_case(shape, K, balance)
    k64 = k.astype(np.float64)
    k32 = (k64 / k64.sum(axis=(0, 1))).astype(np.float32)
    got = wr.wiener(f, k32, balance, np.float32)
    err, bound = np.abs(got - ref).max(), 0.25 * wr.GATE * max(1.0, np.abs(ref).max())
    print("float32 - float64: %.3g (bound %.3g, max |ref| %.3g)" % (err, bound, np.abs(ref).max()))
    assert err <= bound


# ---- the quality cases --------------------------------------------------------------------------------------------------------------------------
def test_the_three_quality_cases_improve_on_the_blurred_frame():
    rms = lambda a: float(np.sqrt((a ** 2).mean()))          # noqa: E731
    seen = []
    for sharp, blurred, psf in wr.quality_cases():
        seen.append((round(rms(blurred - sharp), 4), round(rms(wr.wiener(blurred, psf, 0.01) - sharp), 4)))
    print(seen)
    assert seen == [(0.0868, 0.0678), (0.1095, 0.0790), (0.1455, 0.1087)]


# ---- the host layers ------------------------------------------------------------------------------------------------------------------------------
def test_wiener_args_accepts_and_refuses_what_it_states():
    from lib import _native
    k, b = _native.wiener_args(2.0 * np.ones((5, 5)), 0.01, (40, 52, 3))
    assert k.shape == (5, 5, 3) and k.dtype == np.float32 and k.flags.c_contiguous and b == 0.01
    assert np.array_equal(k, np.full((5, 5, 3), np.float32(1 / 25)))
    k3 = np.dstack([np.ones((3, 3)), 2 * np.eye(3), np.arange(9.0).reshape(3, 3)])
    k, _ = _native.wiener_args(k3, 1, (3, 3))
    assert np.allclose(k.astype(np.float64).sum(axis=(0, 1)), 1, atol=1e-6) and np.array_equal(k[..., 1], (np.eye(3) / 3).astype(np.float32))
    bad_psf = [np.ones((4, 4)), np.ones((1, 1)), np.ones((257, 257)), np.ones((3, 5)), np.ones((3, 3, 2)), np.ones(3), np.ones((7, 7)),
               np.full((3, 3), np.nan), np.full((3, 3), np.inf), np.zeros((3, 3)), -np.ones((3, 3)),
               np.dstack([np.ones((3, 3)), np.ones((3, 3)), np.zeros((3, 3))]), "box"]
    for psf in bad_psf:
        with pytest.raises(ValueError):
            _native.wiener_args(psf, 0.01, (6, 300, 3))
    for balance in (0, -1, np.nan, np.inf, 1e-60, "x", None):
        with pytest.raises(ValueError):
            _native.wiener_args(np.ones((3, 3)), balance, (6, 300, 3))


def test_nonblind_args_accepts_and_refuses_what_it_states():
    import deconvolve as dv
    assert dv._nonblind_args("rl") is None
    assert dv._nonblind_args("wiener") == 0.01
    assert dv._nonblind_args(("wiener", 0.1)) == 0.1 and dv._nonblind_args(["wiener", 1]) == 1.0
    for bad in ("RL", "wiener2", None, 1, ("wiener",), ("wiener", 0), ("wiener", -1), ("wiener", np.nan), ("wiener", np.inf), ("wiener", "x"),
                ("rl", 0.01), ("wiener", 0.01, 1)):
        with pytest.raises(ValueError):
            dv._nonblind_args(bad)
    # refused before the picture is touched
    with pytest.raises(ValueError):
        dv.deblur_module(None, "x", ".", 5, nonblind="tikhonov")


def test_wiener_plan_returns_the_sizes_of_the_specification():
    from lib import _native
    for H, W, K in [(5, 7, 3), (40, 52, 5), (60, 60, 5), (61, 61, 5), (70, 150, 9), (16, 2040, 9), (8170, 24, 23), (4096, 4096, 15), (4000, 6000, 45),
                    (8190, 8190, 3)]:
        plan = _native.wiener_plan(H, W, K)
        assert (plan.Py, plan.Px) == wr.sizes(H, W, K)
        # two spectrum frames of three float2 planes and the tables: less than a third frame's worth
        assert 2 * 3 * 8 * plan.Py * plan.Px < plan.workspace_bytes < 3 * 3 * 8 * plan.Py * plan.Px
    assert _native.wiener_plan(60, 60, 5)[:2] == (64, 64)             # the exact fit H + K - 1 = P
    assert _native.wiener_plan(61, 61, 5)[:2] == (128, 128)           # and one more
    assert _native.wiener_plan(8192 - 22, 24, 23)[:2] == (8192, 64)
    for H, W, K in [(16, 8192, 3), (8192, 16, 3), (8171, 24, 23)]:
        with pytest.raises(_native.NativeError) as ei:
            _native.wiener_plan(H, W, K)
        assert ei.value.code == -6 and "8192" in str(ei.value)        # ICS_ENOSUP, the message names the limit
    for H, W, K in [(40, 52, 4), (40, 52, 1), (40, 52, 257), (4, 52, 5), (40, 4, 5), (0, 5, 3)]:
        with pytest.raises(_native.NativeError) as ei:
            _native.wiener_plan(H, W, K)
        assert ei.value.code == -1


def test_the_two_entries_exist_with_their_argument_counts():
    import os
    import re
    from lib import _native
    lib = _native.load()
    assert len(lib.ics_img_wiener.argtypes) == 5 and len(lib.ics_img_wiener_plan.argtypes) == 6
    assert lib.ics_img_wiener.restype is C.c_int and lib.ics_img_wiener_plan.restype is C.c_int
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ics_hip.h")).read()
    assert re.search(r"int ics_img_wiener\(const ics_img \*src, const float \*psf, int K, float balance, ics_img \*\*out\);", header)
    assert re.search(r"int ics_img_wiener_plan\(int H, int W, int K, int \*Py, int \*Px, size_t \*workspace_bytes\);", header)
    assert int(re.search(r"#define ICS_IMG_WIENER_MAX (\d+)", header).group(1)) == _native.IMG_WIENER_MAX == wr.MAX_SIDE
    assert lib.ics_abi_version() == 4


def test_utils_wiener_has_no_cpu_fallback():
    from lib import _native, utils
    with pytest.raises(ValueError):                                   # refused before anything is uploaded
        utils.wiener(np.zeros((10, 10, 3)), np.ones((4, 4)))
    with pytest.raises(ValueError):
        utils.wiener(np.zeros((10, 10)), np.ones((3, 3)))
    if _native.device_count() > 0:
        pytest.skip("a GPU is present: tests/test_gpu_wiener.py runs the filter")
    with pytest.raises(_native.NativeError):
        utils.wiener(np.zeros((10, 10, 3)), np.ones((3, 3)))
