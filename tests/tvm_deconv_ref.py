"""The specification of DeviceImage.tv_deconvolve_masked / lib.utils.tv_deconvolve_masked (csrc/ics_img_tvmdeconv.hip,
include/ics_hip.h) in numpy / scipy: TV deconvolution of an H x W x 3 frame f by a K x K x 3 PSF, every channel of which sums to 1,
with a masked data term -- minimise sum |Du| + (mu / 2) |M (h * u - f)|^2, M a 0/1 plane: the extension of the frame to the transform
size, clipped pixels, non-finite pixels and whatever the caller marks are unobserved, not fitted.  The mask breaks the diagonal solve of
tests/tv_deconv_ref.py and one more splitting variable (v = h * u, multiplier d, penalty gamma) restores it: Almeida and Figueiredo,
"Deconvolving images with unknown boundaries using the alternating direction method of multipliers", IEEE TIP 2013.
mu = fidelity, beta = penalty, gamma = data_penalty (None: mu), n = iterations.

  1. Py, Px, the ramp extension, Hc and L are those of tests/tv_deconv_ref.py (imported from tests/wiener_ref.py).
  2. m[y, x] = observed[y, x] != 0 (all true for None) and the three channels finite and the three channels < clip;
     f0 = f with non-finite values replaced by 0;  ext = the ramp extension of f0;  M = m on the frame, 0 on every extension pixel,
     one plane for the three channels.
  3. Gc = 1 / (gamma |Hc|^2 + beta L) (its DC term is 1 / gamma);  u = ext, bx = by = d = 0, r_c = real(ifft2(Hc fft2(ext_c))).
  4. n times, indices mod Px, Py:
       the shrink step of tests/tv_deconv_ref.py unchanged: u, bx, by -> bx, by, z (threshold 1 / beta, "vector" / "channel")
       t = r + d;  v = (mu M ext + gamma t) / (mu M + gamma);  d = t - v;  q = v - d     (M = 0: v = t, d = 0, q = r)
       U_c = (gamma conj(Hc) fft2(q_c) + beta fft2(z_c)) Gc;  u_c = real(ifft2(U_c));  r_c = real(ifft2(Hc U_c))
  5. out = u[:H, :W], nothing clipped; and the number of frame pixels with m false.

dtype float64 is the reference the GPU is gated against; dtype float32 evaluates the same formulas with float32 arrays and
complex64 transforms and shows how far rounding alone moves the result."""
import numpy as np
import scipy.fft as sfft

from wiener_ref import GATE, GPU_SHAPES, extend, frame, laplacian, psf_spectrum, quality_cases, sizes, three_psfs  # noqa: F401

FIDELITY, PENALTY, ITERATIONS = 2000.0, 10.0, 10           # the defaults of DeviceImage.tv_deconvolve_masked (data_penalty: fidelity)
COUPLINGS = ("vector", "channel")


def observed_plane(f, observed=None, clip=None):
    """m of step 2: H x W booleans"""
    f = np.asarray(f)
    m = np.isfinite(f).all(axis=2)
    if clip is not None and np.isfinite(clip):
        with np.errstate(invalid="ignore"):
            m &= (f < f.dtype.type(clip)).all(axis=2)
    if observed is not None:
        m &= np.asarray(observed) != 0
    return m


def tv_deconvolve_masked(f, psf, observed=None, clip=None, fidelity=FIDELITY, penalty=PENALTY, data_penalty=None, iterations=ITERATIONS,
                         coupling="vector", dtype=np.float64):
    """-> (out, unobserved)"""
    f = np.asarray(f)
    psf = np.asarray(psf)
    H, W, _ = f.shape
    K = psf.shape[0]
    assert psf.shape == (K, K, 3) and K % 2 == 1 and fidelity > 0 and penalty > 0 and iterations >= 1 and coupling in COUPLINGS
    assert observed is None or np.shape(observed) == (H, W)
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    Py, Px = sizes(H, W, K)
    mu, beta = dtype(fidelity), dtype(penalty)
    gamma = mu if data_penalty is None else dtype(data_penalty)
    thr = dtype(1) / beta
    f = f.astype(dtype)
    m = observed_plane(f, observed, clip)
    ext = extend(extend(np.where(np.isfinite(f), f, dtype(0)), Py, 0), Px, 1)
    M = np.zeros((Py, Px, 1), dtype)
    M[:H, :W, 0] = m
    lam = laplacian(Py, Px).astype(dtype)
    Hs, G = [], []
    for c in range(3):
        Hc = psf_spectrum(psf[..., c].astype(dtype), Py, Px, dtype).astype(cdtype)
        Hs.append(Hc)
        G.append(dtype(1) / (gamma * (Hc.real * Hc.real + Hc.imag * Hc.imag) + beta * lam))
    u = ext.copy()
    bx = np.zeros_like(u)
    by = np.zeros_like(u)
    d = np.zeros_like(u)
    r = np.empty_like(u)
    for c in range(3):
        r[..., c] = sfft.ifft2(Hs[c] * sfft.fft2(ext[..., c])).real
    num, den = mu * M * ext, mu * M + gamma
    for _ in range(iterations):
        vx = np.roll(u, -1, axis=1) - u + bx
        vy = np.roll(u, -1, axis=0) - u + by
        sq = vx * vx + vy * vy
        mag = np.sqrt(sq.sum(axis=2, keepdims=True) if coupling == "vector" else sq)
        s = np.where(mag > thr, (mag - thr) / np.where(mag > thr, mag, dtype(1)), dtype(0)).astype(dtype)
        wx, wy = s * vx, s * vy
        bx, by = vx - wx, vy - wy
        px, py = wx - bx, wy - by
        z = (np.roll(px, 1, axis=1) - px) + (np.roll(py, 1, axis=0) - py)
        t = r + d
        v = (num + gamma * t) / den
        d = t - v
        q = v - d
        for c in range(3):
            U = ((gamma * np.conj(Hs[c]) * sfft.fft2(q[..., c]) + beta * sfft.fft2(z[..., c])) * G[c]).astype(cdtype)
            u[..., c] = sfft.ifft2(U).real
            r[..., c] = sfft.ifft2(Hs[c] * U).real
        assert u.dtype == dtype and r.dtype == dtype and d.dtype == dtype and z.dtype == dtype
    return u[:H, :W].copy(), int(H * W - m.sum())
