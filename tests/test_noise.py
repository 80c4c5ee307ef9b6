"""CPU: the specification of the noise estimate (tests/noise_ref.py: the lower median of the finest starlet detail scale, the level and
sigma derived from it, the automatic thresholds) checked against its definitions and against pictures of known noise, and the surface
of lib._native.noise_args / auto_thresholds / wavelet_args(thresholds="auto") / deblur_module(local_contrast=(gains, "auto")) as far
as it can be checked without a GPU."""
import math
import os
import re
import statistics

import numpy as np
import pytest

import noise_ref as nr
import wavelet_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ics_hip.h")


def ramp(H, W):
    """a smooth picture far from 0 and 1: a plane per channel, which the B3 spline reproduces (w_0 = 0 away from the border)"""
    y, x = np.mgrid[0:H, 0:W]
    base = 0.35 + 0.3 * (x / max(W - 1, 1) + y / max(H - 1, 1)) / 2
    return np.stack([base, base[::-1], base[:, ::-1]], axis=2)


def noisy_ramp(H, W, sigma, seed=7):
    """ramp + white Gaussian noise of standard deviation sigma, float32, unclipped"""
    return (ramp(H, W) + np.random.default_rng(seed).normal(0.0, sigma, (H, W, 3))).astype(np.float32)


# ---- the constants --------------------------------------------------------------------------------------------------------------------
def test_impulse_norm_table_matches_the_oracle_and_the_header():
    from lib import _native
    e = nr.impulse_norms()
    assert len(e) == len(_native.IMG_NOISE_E) == wr.MAX_SCALES == _native.IMG_WAVELET_MAX_SCALES
    for j, (a, b) in enumerate(zip(_native.IMG_NOISE_E, e)):
        assert abs(a - b) <= 1e-9 * b, (j, a, b)
    assert abs(e[0] - nr.E0) <= 1e-12 and abs(_native.IMG_NOISE_E[0] - nr.E0) <= 1e-15
    assert nr.E0 == math.sqrt(1 - 2 * (6 / 16) ** 2 + (70 / 256) ** 2) and abs(nr.E0 - 0.8907963102787584) < 1e-15
    src = open(HEADER).read()
    table = re.search(r"#define ICS_IMG_NOISE_E \{([^}]*)\}", src).group(1).replace("\\", " ")
    assert tuple(float(v) for v in table.split(",")) == tuple(_native.IMG_NOISE_E)
    assert float(re.search(r"#define ICS_IMG_NOISE_STRENGTH ([0-9.]+)f", src).group(1)) == _native.IMG_NOISE_STRENGTH == nr.STRENGTH == 3.0


def chi3_cdf(x):
    return math.erf(x / math.sqrt(2.0)) - math.sqrt(2.0 / math.pi) * x * math.exp(-x * x / 2.0)


def test_kappa_against_its_definitions():
    from lib import _native
    assert abs(statistics.NormalDist().inv_cdf(0.75) - nr.KAPPA["channel"]) <= 1e-12
    try:
        from scipy.stats import chi
        med = float(chi(3).median())
    except ImportError:
        lo, hi = 1.0, 2.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if chi3_cdf(mid) < 0.5 else (lo, mid)
        med = 0.5 * (lo + hi)
    assert abs(chi3_cdf(1.5381722544550522) - 0.5) <= 1e-14
    assert abs(med - 1.5381722544550522) <= 1e-10
    assert abs(med / math.sqrt(3.0) - nr.KAPPA["vector"]) <= 1e-10 and abs(nr.KAPPA["vector"] - 0.888064165169638) <= 1e-14     # rms of chi_3: sqrt(3)
    assert _native.IMG_NOISE_KAPPA == nr.KAPPA


# ---- the oracle on pictures of known noise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", nr.COUPLINGS)
@pytest.mark.parametrize("sigma", [0.01, 0.05])
def test_oracle_recovers_the_noise_of_a_smooth_picture(sigma, coupling):
    """Gate 2 %: the median of n = 86 387 samples of |N(0, s)| scatters by 1 / (2 f(med) sqrt(n)) = 0.4 % of itself (f the density at
    the median; neighbouring w_0 are correlated, which widens it somewhat), and the folded border rows differ from the interior.
    Measured with this picture (default_rng(7), 301 x 287), |sigma_est / sigma - 1|: channel 0.639 % (sigma 0.01) and 0.640 % (0.05)
    at the worst channel (R; G 0.10 / 0.12 %, B 0.05 / 0.00 %), vector 0.112 % and 0.124 %."""
    pic = noisy_ramp(301, 287, sigma)
    assert pic.min() > 0 and pic.max() < 1
    _, _, est = nr.noise_estimate(pic, coupling)
    for s in est:
        print("noise oracle %s sigma %.2f: estimate %.6f, off by %.3f %%" % (coupling, sigma, s, 100 * abs(s / sigma - 1)))
        assert abs(s / sigma - 1) <= 0.02, (coupling, sigma, s)
    _, _, est32 = nr.noise_estimate(pic, coupling, np.float32)         # the float32 restatement estimates the same
    assert all(abs(float(a) / b - 1) <= 1e-4 for a, b in zip(est32, est))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coupling", nr.COUPLINGS)
def test_oracle_properties(coupling, dtype):
    const = np.full((23, 31, 3), 0.375, np.float32) * np.array([1.0, 0.5, 2.0], np.float32)
    assert all(m == 0 for m in nr.medians(const, coupling, dtype))       # every product and sum of the passes is exact: w_0 = 0
    pic = noisy_ramp(61, 47, 0.03, seed=11)
    med = nr.medians(pic, coupling, dtype)
    assert len(med) == (3 if coupling == "channel" else 1) and all(m > 0 and m.dtype == dtype for m in med)
    q = nr.populations(pic, coupling, dtype)
    for m, pop in zip(med, q):                                           # an element of the population, of rank (n - 1) // 2
        assert m in pop and int(np.sum(pop < m)) <= (pop.size - 1) // 2 < int(np.sum(pop <= m))
    for k in (-1, -7, 3):                                                # a power of two scales every rounding with it: exact
        scaled = nr.medians(pic * np.float32(2.0 ** k), coupling, dtype)
        assert [m * dtype(2.0 ** k) for m in med] == scaled, k
    for order in ([2, 0, 1], [1, 0, 2]):
        perm = nr.medians(np.ascontiguousarray(pic[..., order]), coupling, dtype)
        assert perm == ([med[i] for i in order] if coupling == "channel" else med)
    even = nr.populations(pic[:6, :7], coupling, dtype)[0]               # n = 42: the lower of the two middle values
    assert nr.lower_median(even) == np.sort(even)[20]


# ---- auto_thresholds, noise_args, the "auto" forms ----------------------------------------------------------------------------------
def test_auto_thresholds_formula_and_rounding():
    from lib import _native
    E = _native.IMG_NOISE_E
    level = float(np.float32(0.0123456789))
    t = _native.auto_thresholds(level, 5)
    assert t.dtype == np.float32 and t.shape == (5,) and t.flags.c_contiguous
    for j in range(5):
        assert t[j] == np.float32(3.0 * level * E[j] / E[0])
    assert t[0] == np.float32(3.0 * level)
    assert np.array_equal(t, nr.auto_thresholds(level, 5, E))
    assert np.array_equal(_native.auto_thresholds(level, 8, 2.5), nr.auto_thresholds(level, 8, E, 2.5))
    assert np.array_equal(_native.auto_thresholds((0.001, level, 0.002), 5), t)              # "channel": the largest level counts
    assert np.array_equal(_native.auto_thresholds(level, 3, 0.0), np.zeros(3, np.float32))
    assert np.array_equal(_native.auto_thresholds(0.0, 3), np.zeros(3, np.float32))
    assert np.all(np.diff(t) < 0)
    for bad in (float("nan"), float("inf"), -1.0, "strong"):
        with pytest.raises(ValueError, match="strength"):
            _native.auto_thresholds(level, 5, bad)
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match="scales"):
            _native.auto_thresholds(level, bad)
    for bad in (float("nan"), -0.1, (0.1, 0.2)):
        with pytest.raises(ValueError, match="level"):
            _native.auto_thresholds(bad, 5)


def test_noise_args_and_the_auto_forms_of_wavelet_args():
    from lib import _native
    assert _native.noise_args() == ("vector", 0) and _native.noise_args("channel", 2) == ("channel", 2)
    with pytest.raises(ValueError, match="coupling"):
        _native.noise_args("colour")
    for bad in (3, -1, "1", 1.5):
        with pytest.raises(ValueError, match="route"):
            _native.noise_args("vector", bad)
    gains = (1.0, 1.6, 1.8)
    g, t, residual, coupling, route = _native.wavelet_args(gains, "auto")
    assert t == ("auto", 3.0) and g.dtype == np.float32 and (residual, coupling, route) == (1.0, "vector", 0)
    assert _native.wavelet_args(gains, ("auto", 2), 1.0, "channel", 2)[1:] == (("auto", 2.0), 1.0, "channel", 2)
    assert _native.wavelet_args(gains, ["auto", 0.0])[1] == ("auto", 0.0)
    for bad in ("automatic", "", ("auto",), ("auto", 1.0, 2.0), ("manual", 1.0)):
        with pytest.raises(ValueError, match="thresholds"):
            _native.wavelet_args(gains, bad)
    for bad in (float("nan"), -1.0, float("inf"), None):
        with pytest.raises(ValueError, match="strength"):
            _native.wavelet_args(gains, ("auto", bad))
    # today's inputs: unchanged
    g, t, *_ = _native.wavelet_args(gains, (0.03, 0.015, 0.0))
    assert t.dtype == np.float32 and np.array_equal(t, np.array([0.03, 0.015, 0.0], np.float32)) and _native.wavelet_args(gains)[1] is None
    with pytest.raises(ValueError, match="thresholds"):
        _native.wavelet_args(gains, (0.03, 0.015))


def test_local_contrast_args_accept_the_auto_forms():
    import deconvolve as dv
    gains = (1.0, 1.6, 1.8, 1.4, 1.0)
    assert dv._local_contrast_args((gains, "auto")) == (gains, ("auto", 3.0), "vector")
    assert dv._local_contrast_args((gains, "auto", "channel")) == (gains, ("auto", 3.0), "channel")
    assert dv._local_contrast_args((gains, ("auto", 2), "channel")) == (gains, ("auto", 2.0), "channel")
    assert dv._local_contrast_args([list(gains), ["auto", 0]]) == (gains, ("auto", 0.0), "vector")
    for bad, word in (((gains, "automatic"), "thresholds"), ((gains, ("auto", -1.0)), "strength"), ((gains, ("auto", float("nan"))), "strength"),
                      ((gains, "auto", "colour"), "coupling")):
        with pytest.raises(ValueError, match="local_contrast: .*" + word):
            dv._local_contrast_args(bad)
    # today's inputs give today's tuples
    assert dv._local_contrast_args(None) is None
    assert dv._local_contrast_args((gains,)) == (gains, None, "vector")
    assert dv._local_contrast_args((gains, (0.02, 0.01, 0.0, 0.0, 0.0))) == (gains, (0.02, 0.01, 0.0, 0.0, 0.0), "vector")
    assert dv._local_contrast_args((gains, None, "channel")) == (gains, None, "channel")
    assert dv._local_contrast_args((2.0,)) == ((2.0,), None, "vector")
    with pytest.raises(ValueError, match="local_contrast"):
        dv._local_contrast_args((gains, (0.02,)))


def test_the_entry_is_declared_and_exported():
    from lib import _native
    src = open(HEADER).read()
    assert re.search(r"int ics_img_noise_estimate\(const ics_img \*src, int coupling, int route,\s*float median\[3\], float level\[3\], float sigma\[3\]\);", src)
    assert re.search(r"#define ICS_ABI_VERSION 4\b", src)
    lib = _native.load()
    assert lib.ics_img_noise_estimate.restype is not None and lib.ics_abi_version() == 4
