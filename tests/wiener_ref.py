"""The specification of DeviceImage.wiener / lib.utils.wiener (csrc/ics_img_wiener.hip, include/ics_hip.h) in numpy / scipy: Wiener
deconvolution of an H x W x 3 frame by a K x K x 3 PSF, every channel of which sums to 1, regularised by the Laplacian as
skimage.restoration.wiener does by default.

  1. Py, Px: the smallest powers of two >= H + K - 1, W + K - 1.
  2. The frame is extended to Py x Px so that the wrap-around edge carries no step, separably: along y, for every column, rows
     H .. Py - 1 are (1 - t / g) f[H - 1] + (t / g) f[0], g = Py - H + 1, t = 1 .. g - 1; then the same along x on all Py rows.
  3. Hc = fft2 of channel c of the PSF, zero padded to Py x Px, its centre tap (K // 2, K // 2) rolled to (0, 0).
  4. L(ky, kx) = 4 - 2 cos(2 pi ky / Py) - 2 cos(2 pi kx / Px), a closed form.
  5. G = conj(Hc) / (|Hc|^2 + balance L^2); out[..., c] = real(ifft2(G fft2(ext[..., c])))[:H, :W].  Nothing is clipped.

dtype float64 is the reference the GPU is gated against; dtype float32 evaluates the same formulas with float32 arrays and
complex64 transforms and shows how far rounding alone moves the result.  A delta PSF does not return the input: G is then
1 / (1 + balance L^2), a low-pass."""
import numpy as np
import scipy.fft as sfft

MAX_SIDE = 8192          # include/ics_hip.h ICS_IMG_WIENER_MAX


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def sizes(H, W, K):
    return next_pow2(H + K - 1), next_pow2(W + K - 1)


def extend(f, P, axis):
    """`f` with its `axis` grown to P entries by the ramp from the last entry back to the first"""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    g = P - n + 1
    t = (np.arange(1, g, dtype=f.dtype) / f.dtype.type(g)).reshape((-1,) + (1,) * (f.ndim - 1))
    ramp = (1 - t) * f[n - 1] + t * f[0]
    return np.moveaxis(np.concatenate([f, ramp], axis=0), 0, axis)


def laplacian(Py, Px):
    ky = np.arange(Py, dtype=np.float64).reshape(-1, 1)
    kx = np.arange(Px, dtype=np.float64).reshape(1, -1)
    return 4.0 - 2.0 * np.cos(2.0 * np.pi * ky / Py) - 2.0 * np.cos(2.0 * np.pi * kx / Px)


def psf_spectrum(k, Py, Px, dtype=np.float64):
    K = k.shape[0]
    h = np.zeros((Py, Px), dtype)
    h[:K, :K] = k
    return sfft.fft2(np.roll(h, (-(K // 2), -(K // 2)), axis=(0, 1)))


def wiener(f, psf, balance, dtype=np.float64):
    f = np.asarray(f)
    psf = np.asarray(psf)
    H, W, _ = f.shape
    K = psf.shape[0]
    assert psf.shape == (K, K, 3) and K % 2 == 1 and balance > 0
    Py, Px = sizes(H, W, K)
    ext = extend(extend(f.astype(dtype), Py, 0), Px, 1)
    lam = laplacian(Py, Px).astype(dtype)
    reg = dtype(balance) * lam * lam
    out = np.empty((H, W, 3), dtype)
    for c in range(3):
        Hc = psf_spectrum(psf[..., c].astype(dtype), Py, Px, dtype)
        G = np.conj(Hc) / ((Hc.real * Hc.real + Hc.imag * Hc.imag) + reg)
        out[..., c] = sfft.ifft2(G * sfft.fft2(ext[..., c])).real[:H, :W]
    assert out.dtype == dtype
    return out


# ---- the pictures and PSFs of the tests -------------------------------------------------------------------------------------------------
def dead_leaves(rng, H, W, n=400):
    img = np.full((H, W, 3), 0.5)
    yy, xx = np.mgrid[:H, :W]
    for _ in range(n):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(3, 20)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.uniform(0.05, 0.95, 3)
    return img


def quality_cases(seed=109, sigma=0.002):
    """(sharp, blurred + noise, psf) for a uniform box of 5 px on 40 x 52, of 9 px on 70 x 150 and of 15 px on 160 x 192, drawn in this
    order from one generator"""
    from scipy.ndimage import convolve
    rng = np.random.default_rng(seed)
    cases = []
    for H, W, K in [(40, 52, 5), (70, 150, 9), (160, 192, 15)]:
        big = dead_leaves(rng, H + 2 * K, W + 2 * K)
        k = np.ones((K, K)) / K ** 2
        blurred = np.dstack([convolve(big[..., c], k, mode="nearest") for c in range(3)])[K:-K, K:-K]
        blurred = blurred + rng.normal(0, sigma, blurred.shape)
        cases.append((big[K:-K, K:-K], blurred, np.dstack([k] * 3)))
    return cases


def three_psfs(K):
    """a box, a Gaussian and an L-shaped PSF with its weight off centre on the three channels, each of sum 1: a transform that packs two
    channels, swaps them or flips a kernel cannot pass"""
    box = np.ones((K, K))
    r = np.arange(K) - K // 2
    gauss = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * (K / 4.0) ** 2))
    ell = np.full((K, K), 0.02)
    ell[0, :] = 1.0
    ell[:, 0] = 2.0
    ell[K - 1, K - 1] = 0.5
    k = np.dstack([box, gauss, ell])
    return k / k.sum(axis=(0, 1))


def frame(H, W, seed):
    """a smooth picture with a few edges and some noise, values in about [0, 1]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    f = np.empty((H, W, 3))
    for c in range(3):
        f[..., c] = 0.5 + 0.3 * np.sin(0.11 * (c + 1) * yy + 0.07 * xx + c) + 0.15 * ((xx * (c + 2) // 7 + yy // 5) % 2)
    return np.clip(f + rng.normal(0, 0.01, f.shape), 0.0, 1.0)


# frame, K of the GPU cases (tests/test_gpu_wiener.py), and the gate: max |gpu - ref| <= GATE max(1, max |ref|)
GPU_SHAPES = [((5, 7), 3), ((40, 52), 5), ((60, 60), 5), ((61, 61), 5), ((70, 150), 9), ((16, 2040), 9), ((2040, 16), 9), ((24, 8170), 23), ((8170, 24), 23)]
GATE = 1e-4
BALANCES = (0.01, 0.001)
