"""Wavelet equaliser (undecimated B3-spline / "a trous" / starlet decomposition, soft-thresholded and weighted scale by scale) in
numpy, the specification of ics_img_wavelet_equalize / DeviceImage.wavelet_equalize (csrc/ics_img_wavelet.hip) with the dtype as a
parameter: float64 is the oracle of the tests, float32 the restatement whose distance from the oracle sets their gates.

    c_0 = f,  c_{j+1} = V_j(H_j(c_j)):  taps [1 4 6 4 1] / 16 at offsets {-2 .. 2} * 2^j along x (H_j), then along y (V_j)
    an index outside the picture folds as numpy.pad(mode="symmetric"): i mod 2n, then 2n - 1 - i if >= n
    one axis pass: ((a[-2] + a[+2]) / 16 + (a[-1] + a[+1]) * 4 / 16) + a[0] * 6 / 16
    w_j = c_j - c_{j+1}
    s_j = sign(w) max(|w| - t_j, 0)                 "channel"
          w * (max(m - t_j, 0) / m), 0 where m = 0   "vector": m = sqrt(w_r^2 + w_g^2 + w_b^2), the squares added smallest first
    out = residual * c_J + (((g_0 s_0) + g_1 s_1) + ... )    accumulated in that order from zero"""
import numpy as np

COUPLINGS = ("channel", "vector")
MAX_SCALES = 8


def fold(i, n):
    """index of numpy.pad(mode="symmetric") for any integer i"""
    i = np.mod(np.asarray(i), 2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def axis_pass(c, d, axis, dtype):
    n = c.shape[axis]
    a = [np.take(c, fold(np.arange(n) + k * d, n), axis=axis) for k in (-2, -1, 0, 1, 2)]
    return ((a[0] + a[4]) * dtype(1 / 16) + (a[1] + a[3]) * dtype(4 / 16)) + a[2] * dtype(6 / 16)


def smooth(c, j, dtype=np.float64):
    """c_{j+1} from c_j"""
    return axis_pass(axis_pass(c, 2 ** j, 1, dtype), 2 ** j, 0, dtype)


def shrink(w, t, coupling, dtype):
    t = dtype(t)
    if coupling == "channel":
        return np.sign(w) * np.maximum(np.abs(w) - t, dtype(0))
    q = np.sort(w * w, axis=2)                  # smallest first: the sum does not depend on the order of the channels
    m = np.sqrt((q[..., 0] + q[..., 1]) + q[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(m > 0, np.maximum(m - t, dtype(0)) / m, dtype(0)).astype(dtype)
    return w * k[..., None]


def decompose(f, scales, dtype=np.float64):
    """([w_0 .. w_{J-1}], c_J)"""
    c = np.asarray(f, dtype=dtype)
    details = []
    for j in range(scales):
        nxt = smooth(c, j, dtype)
        details.append(c - nxt)
        c = nxt
    return details, c


def wavelet_equalize(f, gains, thresholds=None, residual=1.0, coupling="vector", dtype=np.float64):
    """f: H x W x 3.  Every operation is carried out in `dtype`."""
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    gains = [float(g) for g in gains]
    if not 1 <= len(gains) <= MAX_SCALES:
        raise ValueError("1 .. %d scales" % MAX_SCALES)
    thresholds = [0.0] * len(gains) if thresholds is None else [float(t) for t in thresholds]
    if len(thresholds) != len(gains):
        raise ValueError("one threshold per gain")
    details, c = decompose(f, len(gains), dtype)
    acc = np.zeros_like(c)
    for w, g, t in zip(details, gains, thresholds):
        acc = acc + dtype(np.float32(g)) * shrink(w, np.float32(t), coupling, dtype)      # the device takes float32 parameters
    out = dtype(np.float32(residual)) * c + acc
    assert out.dtype == dtype
    return out
