"""Noise estimate from the finest starlet scale in numpy, the specification of ics_img_noise_estimate / DeviceImage.noise_estimate
(csrc/ics_img_noise.hip) with the dtype as a parameter, built on tests/wavelet_ref.py: float64 is the oracle of the tests, float32 the
restatement the device must equal bit for bit.

    w_0   = c_0 - c_1, c_1 = V_0(H_0(c_0)) as in wavelet_ref (taps [1 4 6 4 1] / 16 along x, then y, symmetric fold, no FMA)
    q     = |w_0| per channel, three populations of n = H W values                         "channel"
            sqrt((s0 + s1) + s2), the squares of the three channels added smallest first    "vector": one population
    med   = the lower median: the value of rank k = (n - 1) // 2 (zero-based) of the sorted population, an element of it
    level = med / kappa       kappa = median of |N(0, 1)| ("channel"), median of chi_3 / sqrt(3) ("vector"): the rms of q under Gaussian noise
    sigma = level / e_0 ("channel"), level / (sqrt(3) e_0) ("vector"): the per-channel standard deviation of white noise in the picture;
            e_j = the L2 norm of the response of w_j to a unit impulse
    t_j   = strength * level * e_j / e_0: the thresholds of scale j that cut `strength` standard deviations of such noise

level, sigma and t_j are computed in double from the float32 median and rounded to float32."""
import math

import numpy as np

import wavelet_ref as wr

COUPLINGS = wr.COUPLINGS
KAPPA = {"channel": 0.6744897501960817, "vector": 1.5381722544550522 / math.sqrt(3.0)}
E0 = math.sqrt(1.0 - 2.0 * (6.0 / 16.0) ** 2 + (70.0 / 256.0) ** 2)
STRENGTH = 3.0


def detail0(f, dtype=np.float64):
    """w_0 of an H x W x 3 picture"""
    c = np.asarray(f, dtype=dtype)
    w = c - wr.smooth(c, 0, dtype)
    assert w.dtype == dtype
    return w


def populations(f, coupling, dtype=np.float64):
    """the populations whose medians are taken: 3 x n ("channel") or 1 x n ("vector")"""
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    w = detail0(f, dtype)
    if coupling == "channel":
        return np.abs(w).reshape(-1, 3).T.copy()
    s = np.sort(w * w, axis=2)
    return np.sqrt((s[..., 0] + s[..., 1]) + s[..., 2]).reshape(1, -1)


def lower_median(q):
    q = np.asarray(q).ravel()
    k = (q.size - 1) // 2
    return np.partition(q, k)[k]


def medians(f, coupling, dtype=np.float64):
    return [lower_median(q) for q in populations(f, coupling, dtype)]


def derived(median, coupling):
    """(level, sigma) as float32 from one median, in double"""
    level = float(median) / KAPPA[coupling]
    sigma = level / E0 if coupling == "channel" else level / (math.sqrt(3.0) * E0)
    return np.float32(level), np.float32(sigma)


def noise_estimate(f, coupling="vector", dtype=np.float64):
    """(medians, levels, sigmas): three values each for "channel", one for "vector"; float32 medians give float32 derived numbers,
    float64 medians are left in double (the oracle)"""
    med = medians(f, coupling, dtype)
    if dtype == np.float32:
        lv, sg = zip(*(derived(m, coupling) for m in med))
        return list(med), list(lv), list(sg)
    lv = [float(m) / KAPPA[coupling] for m in med]
    return list(med), lv, [v / (E0 if coupling == "channel" else math.sqrt(3.0) * E0) for v in lv]


def impulse_norms(scales=wr.MAX_SCALES, size=1025):
    """e_0 .. e_{scales-1}: the L2 norms of the detail scales of a unit impulse in the middle of a size x size picture"""
    f = np.zeros((size, size, 1))
    f[size // 2, size // 2, 0] = 1.0
    return [float(np.sqrt(np.sum(w * w))) for w in wr.decompose(f, scales)[0]]


def auto_thresholds(level, scales, e, strength=STRENGTH):
    """t_j = strength * level * e_j / e_0 as float32; level: one value or several (the largest counts)"""
    level = float(np.max(np.atleast_1d(np.asarray(level, dtype=np.float64))))
    return np.array([strength * level * e[j] / e[0] for j in range(scales)], dtype=np.float64).astype(np.float32)
