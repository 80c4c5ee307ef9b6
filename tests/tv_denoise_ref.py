"""TV (Rudin-Osher-Fatemi) denoising by Chambolle's dual projection iteration in numpy, the specification of
ics_img_tv_denoise / DeviceImage.tv_denoise (csrc/ics_img_tvdenoise.hip) with the dtype as a parameter: float64 is the oracle of
the tests, float32 the restatement whose distance from the oracle sets their gates.

    min_u 1/2 |u - f|^2 + weight * TV(u),    tau = 1/8, a fixed number of iterations, q = (qx, qy) = 0 at the start

    u  = f + div q          (div q)[y,x] = qx[y,x] - qx[y,x-1] + qy[y,x] - qy[y-1,x], terms with index -1 are 0
    gx = u[y,x+1] - u[y,x]  (0 in the last column),   gy = u[y+1,x] - u[y,x]  (0 in the last row)
    s  = gx^2 + gy^2        "channel": per channel;  "vector": summed over the three channels (smallest term first), one s per pixel
    q  = (q + tau g) / (1 + (tau / weight) sqrt(s))

The result is f + div q of the last q; iterations = 0 returns a copy of f."""
import numpy as np

TAU = 0.125
COUPLINGS = ("channel", "vector")


def div(qx, qy):
    d = qx + qy
    d[:, 1:] -= qx[:, :-1]
    d[1:, :] -= qy[:-1, :]
    return d


def grad(u):
    gx, gy = np.zeros_like(u), np.zeros_like(u)
    gx[:, :-1] = u[:, 1:] - u[:, :-1]
    gy[:-1, :] = u[1:, :] - u[:-1, :]
    return gx, gy


def tv_denoise(f, weight=0.1, iterations=50, coupling="vector", dtype=np.float64):
    """f: H x W x 3.  Every operation is carried out in `dtype`."""
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    f = np.asarray(f, dtype=dtype)
    tau = dtype(TAU)
    k = tau / dtype(weight)
    qx, qy = np.zeros_like(f), np.zeros_like(f)
    for _ in range(iterations):
        gx, gy = grad(f + div(qx, qy))
        s = gx * gx + gy * gy
        if coupling == "vector":
            s = np.sort(s, axis=2)              # smallest first: the sum does not depend on the order of the channels
            s = ((s[..., 0] + s[..., 1]) + s[..., 2])[..., None]
        den = dtype(1) + k * np.sqrt(s)
        qx = (qx + tau * gx) / den
        qy = (qy + tau * gy) / den
    out = f + div(qx, qy)
    assert out.dtype == dtype
    return out


def rof_energy(u, f, weight, coupling):
    """1/2 |u - f|^2 + weight * TV(u) in float64, TV with the forward differences above"""
    u, f = np.asarray(u, np.float64), np.asarray(f, np.float64)
    gx, gy = grad(u)
    s = gx * gx + gy * gy
    if coupling == "vector":
        s = s.sum(axis=2)
    return 0.5 * float(((u - f) ** 2).sum()) + weight * float(np.sqrt(s).sum())
