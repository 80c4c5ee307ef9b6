"""The specification of DeviceImage.tv_deconvolve / lib.utils.tv_deconvolve (csrc/ics_img_tvdeconv.hip, include/ics_hip.h) in numpy /
scipy: deconvolution of an H x W x 3 frame f by a K x K x 3 PSF, every channel of which sums to 1, under a total-variation prior --
minimise sum |Du| + (mu / 2) |h * u - f|^2 by variable splitting (FTVd, Wang, Yang, Yin, Zhang 2008, in its split-Bregman / ADMM form,
Goldstein and Osher 2009).  mu = fidelity, beta = penalty, n = iterations.

  1. Py, Px, the ramp-extended frame ext and Hc are the Wiener filter's (tests/wiener_ref.py, steps 1 to 3); L is its step 4 itself,
     not squared: 4 sin^2(pi ky / Py) + 4 sin^2(pi kx / Px) is the transfer of D^T D for periodic forward differences, exactly.
     Everything below runs on the periodic Py x Px domain, the data term included.
  2. N0c = mu conj(Hc) fft2(ext_c),  Gc = 1 / (mu |Hc|^2 + beta L),  u = ext, bx = by = 0.
  3. n times, indices mod Px, Py:
       vx = u[y, x+1] - u[y, x] + bx,  vy = u[y+1, x] - u[y, x] + by
       m  = sqrt(vx^2 + vy^2) -- "channel": per value; "vector": summed over the three channels too (six terms)
       s  = (m - 1 / beta) / m where m > 1 / beta, else 0
       wx = s vx, wy = s vy;  bx = vx - wx, by = vy - wy;  px = wx - bx, py = wy - by
       z  = (px[y, x-1] - px[y, x]) + (py[y-1, x] - py[y, x])                                   (= D^T p)
       u_c = real(ifft2((N0c + beta fft2(z_c)) Gc))
  4. out = u[:H, :W].  Nothing is clipped.

dtype float64 is the reference the GPU is gated against; dtype float32 evaluates the same formulas with float32 arrays and
complex64 transforms and shows how far rounding alone moves the result."""
import numpy as np
import scipy.fft as sfft

from wiener_ref import GATE, GPU_SHAPES, extend, frame, laplacian, psf_spectrum, quality_cases, sizes, three_psfs  # noqa: F401

FIDELITY, PENALTY, ITERATIONS = 2000.0, 10.0, 10           # the defaults of DeviceImage.tv_deconvolve
MAX_ITERATIONS = 500                                        # include/ics_hip.h ICS_IMG_TVD_MAX_ITERATIONS
COUPLINGS = ("vector", "channel")


def tv_deconvolve(f, psf, fidelity=FIDELITY, penalty=PENALTY, iterations=ITERATIONS, coupling="vector", dtype=np.float64):
    f = np.asarray(f)
    psf = np.asarray(psf)
    H, W, _ = f.shape
    K = psf.shape[0]
    assert psf.shape == (K, K, 3) and K % 2 == 1 and fidelity > 0 and penalty > 0 and iterations >= 1 and coupling in COUPLINGS
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    Py, Px = sizes(H, W, K)
    mu, beta = dtype(fidelity), dtype(penalty)
    thr = dtype(1) / beta
    ext = extend(extend(f.astype(dtype), Py, 0), Px, 1)
    lam = laplacian(Py, Px).astype(dtype)
    N0, G = [], []
    for c in range(3):
        Hc = psf_spectrum(psf[..., c].astype(dtype), Py, Px, dtype).astype(cdtype)
        N0.append((mu * np.conj(Hc) * sfft.fft2(ext[..., c])).astype(cdtype))
        G.append(dtype(1) / (mu * (Hc.real * Hc.real + Hc.imag * Hc.imag) + beta * lam))
    u = ext.copy()
    bx = np.zeros_like(u)
    by = np.zeros_like(u)
    for _ in range(iterations):
        vx = np.roll(u, -1, axis=1) - u + bx
        vy = np.roll(u, -1, axis=0) - u + by
        sq = vx * vx + vy * vy
        m = np.sqrt(sq.sum(axis=2, keepdims=True) if coupling == "vector" else sq)
        s = np.where(m > thr, (m - thr) / np.where(m > thr, m, dtype(1)), dtype(0)).astype(dtype)
        wx, wy = s * vx, s * vy
        bx, by = vx - wx, vy - wy
        px, py = wx - bx, wy - by
        z = (np.roll(px, 1, axis=1) - px) + (np.roll(py, 1, axis=0) - py)
        for c in range(3):
            u[..., c] = sfft.ifft2((N0[c] + beta * sfft.fft2(z[..., c])) * G[c]).real
        assert u.dtype == dtype and bx.dtype == dtype and z.dtype == dtype
    return u[:H, :W].copy()
