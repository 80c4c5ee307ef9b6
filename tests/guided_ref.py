"""Guided filter (He, Sun, Tang) with the picture as its own guide, in numpy: the specification of ics_img_guided /
DeviceImage.guided_filter (csrc/ics_img_guided.hip) with the dtype as a parameter: float64 is the oracle of the tests, float32 the
restatement whose distance from the oracle sets their gates.  The restatement performs the kernel's operations in the kernel's order
(gf_channel / gf_vector / gf_out there), every product and sum rounded on its own: no FMA.

    I' = I - 0.5                                     (centring: E[I'^2] - E[I']^2 cancels far less than E[I^2] - E[I]^2)
    window of pixel k: the (2 r + 1)^2 square clipped to the picture; mean_k(x) = (sum over it) / (its pixel count)
    a sum: along x first, then along y, the taps added from zero in ascending offset order -r .. r; a tap outside the picture is +0
    "channel", per channel c:  mu = mean(I'_c), v = mean(I'_c^2) - mu mu, a = v / (v + eps), b = mu - a mu
    "vector":  mu_i = mean(I'_i), S_ij = mean(I'_i I'_j) - mu_i mu_j (i <= j), M = S + eps E,
               c_ij the six cofactors of M, det = (M00 c00 + M01 c01) + M02 c02, A_ij = [i = j] - eps (c_ij / det)   (= M^-1 S),
               b_i = mu_i - ((A_i0 mu_0 + A_i1 mu_1) + A_i2 mu_2)
    q = (mean(a) I' + mean(b)) + 0.5   or   q_i = (((mean(A_i0) I'_0 + mean(A_i1) I'_1) + mean(A_i2) I'_2) + mean(b_i)) + 0.5
    out = q if detail == 0 else q + detail (I - q)"""
import numpy as np

COUPLINGS = ("channel", "vector")
MAX_RADIUS = 32
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # the distinct entries of a symmetric 3 x 3, in the kernel's order


def box_sum(x, r):
    """sum over the clipped (2 r + 1)^2 window of every pixel of x (H x W or H x W x C), in x.dtype: rows first, then columns, taps
    in ascending order from zero"""
    for axis in (1, 0):
        n = x.shape[axis]
        pad = [(0, 0)] * x.ndim
        pad[axis] = (r, r)
        p = np.pad(x, pad)
        s = np.zeros_like(x)
        for k in range(2 * r + 1):
            s = s + np.take(p, np.arange(k, k + n), axis=axis)
        x = s
    return x


def window_count(H, W, r, dtype):
    ny = np.minimum(np.arange(H) + r, H - 1) - np.maximum(np.arange(H) - r, 0) + 1
    nx = np.minimum(np.arange(W) + r, W - 1) - np.maximum(np.arange(W) - r, 0) + 1
    return (ny[:, None] * nx[None, :]).astype(dtype)


def box_mean(x, r):
    cnt = window_count(x.shape[0], x.shape[1], r, x.dtype)
    return box_sum(x, r) / (cnt if x.ndim == 2 else cnt[..., None])


def coefficients(Ic, r, eps, coupling):
    """(a, b) of every window from the centred picture: a is H x W x 3 ("channel") or H x W x 6 (PAIRS order, "vector")"""
    dtype = Ic.dtype.type
    one = dtype(1)
    mu = box_mean(Ic, r)
    if coupling == "channel":
        v = box_mean(Ic * Ic, r) - mu * mu
        a = v / (v + eps)
        return a, mu - a * mu
    S = {(i, j): box_mean(Ic[..., i] * Ic[..., j], r) - mu[..., i] * mu[..., j] for i, j in PAIRS}
    M = {ij: S[ij] + eps if ij[0] == ij[1] else S[ij] for ij in PAIRS}
    c = {(0, 0): M[1, 1] * M[2, 2] - M[1, 2] * M[1, 2], (0, 1): M[0, 2] * M[1, 2] - M[0, 1] * M[2, 2], (0, 2): M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1],
         (1, 1): M[0, 0] * M[2, 2] - M[0, 2] * M[0, 2], (1, 2): M[0, 1] * M[0, 2] - M[0, 0] * M[1, 2], (2, 2): M[0, 0] * M[1, 1] - M[0, 1] * M[0, 1]}
    det = (M[0, 0] * c[0, 0] + M[0, 1] * c[0, 1]) + M[0, 2] * c[0, 2]
    A = {ij: (one if ij[0] == ij[1] else dtype(0)) - eps * (c[ij] / det) for ij in PAIRS}
    at = lambda i, j: A[min(i, j), max(i, j)]     # noqa: E731
    b = np.stack([mu[..., i] - ((at(i, 0) * mu[..., 0] + at(i, 1) * mu[..., 1]) + at(i, 2) * mu[..., 2]) for i in range(3)], axis=2)
    return np.stack([A[ij] for ij in PAIRS], axis=2), b


def base_layer(I, radius, eps, coupling="vector", dtype=np.float64):
    """q: the edge-preserving base layer.  I: H x W x 3.  Every operation is carried out in `dtype`."""
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    if not 1 <= int(radius) <= MAX_RADIUS or int(radius) != radius:
        raise ValueError("radius %r (1 .. %d)" % (radius, MAX_RADIUS))
    if not eps > 0:
        raise ValueError("eps %r" % (eps,))
    r, half = int(radius), dtype(0.5)
    Ic = np.asarray(I, dtype=dtype) - half
    a, b = coefficients(Ic, r, dtype(np.float32(eps)), coupling)         # the device takes float32 parameters
    ma, mb = box_mean(a, r), box_mean(b, r)
    if coupling == "channel":
        q = (ma * Ic + mb) + half
    else:
        k = {ij: n for n, ij in enumerate(PAIRS)}
        at = lambda i, j: ma[..., k[min(i, j), max(i, j)]]     # noqa: E731
        q = np.stack([(((at(i, 0) * Ic[..., 0] + at(i, 1) * Ic[..., 1]) + at(i, 2) * Ic[..., 2]) + mb[..., i]) + half for i in range(3)], axis=2)
    assert q.dtype == dtype
    return q


def guided_filter(I, radius, eps, detail=0.0, coupling="vector", dtype=np.float64):
    q = base_layer(I, radius, eps, coupling, dtype)
    if detail == 0:
        return q
    out = q + dtype(np.float32(detail)) * (np.asarray(I, dtype=dtype) - q)
    assert out.dtype == dtype
    return out
