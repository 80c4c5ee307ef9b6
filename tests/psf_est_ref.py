"""The specification of DeviceImage.psf_raw / lib.utils.estimate_psf (csrc/ics_img_psfest.hip, include/ics_hip.h) in numpy / scipy: the
PSF that takes a sharp H x W x 3 frame s to a blurred one b of the same scene, the linear solve of the fast blind methods (Cho and Lee
2009; Xu and Jia 2010) on the derivatives of the pair, k = argmin sum |d s * k - d b|^2 + gamma |k|^2.

  1. Py, Px = wiener_ref.sizes(H, W, K), each at most 8192.
  2. The taper w = wy (x) wx: Ty = min(K, H // 2), j = min(y, H - 1 - y), wy[y] = 0.5 - 0.5 cos(pi (j + 0.5) / Ty) for j < Ty, else 1;
     wx the same along x (the pair obeys b = s * k only away from the border).
  3. For f = s and f = b and every channel: dx[y, x] = w[y, x] (f[y, x+1] - f[y, x]) for x < W - 1, 0 at x = W - 1; dy the same along
     y; everything zero beyond H x W up to Py x Px (no ramp extension).
  4. A = fft2(d s), B = fft2(d b); per channel N_c = sum_d conj(A) B, D_c = sum_d |A|^2, S_c = sum_d sum_pixels (d s_c)^2 over the two
     directions d.  "vector" sums N, D and S over the three channels (one PSF, its plane and its energy three times); "channel" keeps
     three.
  5. full = real(ifft2(N / (D + regularisation S))); raw[i, j] = full[(i - K // 2) mod Py, (j - K // 2) mod Px], K x K x 3: the
     orientation of wiener_ref.psf_spectrum, b ~ s * raw as a true convolution with the centre tap at (K // 2, K // 2).
  6. The projection (project), per plane, in float64: m = max(raw); taps below threshold m are 0 (every negative tap too); the rest is
     divided by its sum; rejected = sum |raw - kept| / sum |raw|, kept the plane before the division.

dtype float64 is the reference the GPU is gated against; dtype float32 evaluates the same formulas with float32 arrays and complex64
transforms and shows how far rounding alone moves the result."""
import functools

import numpy as np
import scipy.fft as sfft

import wiener_ref as wr
from wiener_ref import dead_leaves, frame, quality_cases, three_psfs   # noqa: F401  (the pictures of the tests)

REGULARISATION = 1e-3
THRESHOLD = 0.05


def taper(n, K, dtype=np.float64):
    T = min(K, n // 2)
    j = np.minimum(np.arange(n), n - 1 - np.arange(n))
    w = np.ones(n)
    w[j < T] = 0.5 - 0.5 * np.cos(np.pi * (j[j < T] + 0.5) / T)
    return w.astype(dtype)


def derivatives(f, K, Py, Px, dtype=np.float64):
    """the tapered forward differences of an H x W x 3 frame, zero padded: (2, Py, Px, 3), direction x first"""
    f = np.asarray(f).astype(dtype)
    H, W, _ = f.shape
    w = (taper(H, K, dtype)[:, None] * taper(W, K, dtype)[None, :])[..., None]
    d = np.zeros((2, Py, Px, 3), dtype)
    d[0, :H, :W - 1] = w[:, :W - 1] * (f[:, 1:] - f[:, :-1])
    d[1, :H - 1, :W] = w[:H - 1] * (f[1:] - f[:-1])
    return d


def raw_kernel(b, s, K, regularisation=REGULARISATION, coupling="vector", dtype=np.float64):
    """steps 1 to 5: (raw K x K x 3, energy of 3 entries)"""
    b, s = np.asarray(b), np.asarray(s)
    H, W, _ = s.shape
    assert b.shape == s.shape and K % 2 == 1 and 3 <= K <= min(H, W, 255) and regularisation > 0 and coupling in ("vector", "channel")
    Py, Px = wr.sizes(H, W, K)
    assert max(Py, Px) <= wr.MAX_SIDE
    ds, db = derivatives(s, K, Py, Px, dtype), derivatives(b, K, Py, Px, dtype)
    A, B = sfft.fft2(ds, axes=(1, 2)), sfft.fft2(db, axes=(1, 2))
    N = (np.conj(A) * B).sum(axis=0)                               # Py x Px x 3
    D = (A.real * A.real + A.imag * A.imag).sum(axis=0)
    S = (ds * ds).sum(axis=(0, 1, 2))                              # 3
    if coupling == "vector":
        N, D, S = (np.repeat(v.sum(axis=-1, keepdims=True), 3, axis=-1) for v in (N, D, S))
    full = sfft.ifft2(N / (D + dtype(regularisation) * S), axes=(0, 1)).real
    idx_y, idx_x = (np.arange(K) - K // 2) % Py, (np.arange(K) - K // 2) % Px
    raw = full[idx_y][:, idx_x]
    assert raw.dtype == dtype and raw.shape == (K, K, 3)
    return raw, S.astype(np.float64)


def project(raw, threshold=THRESHOLD):
    """step 6: (psf K x K x 3 float64, every plane of sum 1; rejected, 3 floats)"""
    raw = np.asarray(raw, dtype=np.float64)
    psf, rejected = np.empty_like(raw), np.empty(3)
    for c in range(3):
        p = raw[..., c]
        kept = np.where(p < threshold * p.max(), 0.0, p)
        rejected[c] = np.abs(p - kept).sum() / np.abs(p).sum()
        psf[..., c] = kept / kept.sum()
    return psf, rejected


def estimate(b, s, K, regularisation=REGULARISATION, threshold=THRESHOLD, coupling="vector"):
    return project(raw_kernel(b, s, K, regularisation, coupling)[0], threshold)[0]


# ---- the pictures of the tests -----------------------------------------------------------------------------------------------------------
def blurred_by(sharp_big, k, K, rng, sigma=0.002):
    """the K-wider frame convolved by the K x K x 3 PSF k (a true convolution, the frame repeating its edge; through the transform, so
    that K = 255 takes no longer than K = 3), its rim of K cut off, plus noise"""
    from scipy.signal import fftconvolve
    pad = np.pad(sharp_big, ((K // 2, K // 2), (K // 2, K // 2), (0, 0)), mode="edge")
    b = np.dstack([fftconvolve(pad[..., c], k[..., c], mode="valid") for c in range(3)])[K:-K, K:-K]
    return b + rng.normal(0, sigma, b.shape)


# frame, K of the GPU cases (tests/test_gpu_psf_estimate.py): an 8 x 16 transform with the taper clamped by H // 2, a small plain case,
# the exact fit 60 + 5 - 1 = 64 and one over, Py != Px, lines of 2048 and the full LDS line of 8192 on either axis, the largest K
GPU_CASES = [((5, 7), 3), ((40, 52), 5), ((60, 60), 5), ((61, 61), 5), ((70, 150), 9), ((16, 2040), 9), ((2040, 16), 9), ((24, 8170), 23), ((8170, 24), 23),
             ((260, 300), 255)]
GATE = 1e-4                       # max |x - ref| <= GATE max |ref|: the project's parity gate relative to the peak of raw (the taps are far below 1)
ENERGY_GATE = 1e-5                # relative, on the energies
REGULARISATIONS = (1e-2, 1e-4)
COUPLINGS = ("vector", "channel")


@functools.lru_cache(maxsize=None)
def gpu_pair(shape, K):
    """(sharp, blurred) float32, H x W x 3: wiener_ref.frame where both sides are below 40 px (it has gradients everywhere), dead leaves
    above; blurred by three_psfs(K) on a frame K larger all round, cropped, plus noise of sigma 0.002.  Shared by the tests: do not
    write to it.  (wiener_ref.frame is no picture for the long thin cases: its stripes repeat over thousands of pixels, the spectrum
    of their derivative is a few peaks 10^3 times above the rest, and float32 transforms, whose error is relative to the peaks, lose
    the rest -- the float32 evaluation of this specification is then itself 1e-4 of the peak off the float64 one, the whole gate.)"""
    H, W = shape
    rng = np.random.default_rng(1000 + H + 7 * W + K)
    if max(H, W) < 40:
        big = frame(H + 2 * K, W + 2 * K, seed=H + W)
    else:
        big = dead_leaves(rng, H + 2 * K, W + 2 * K)
    s = np.ascontiguousarray(big[K:-K, K:-K], dtype=np.float32)
    b = np.ascontiguousarray(blurred_by(big, three_psfs(K), K, rng), dtype=np.float32)
    s.setflags(write=False); b.setflags(write=False)
    return s, b


@functools.lru_cache(maxsize=None)
def gpu_reference(shape, K, regularisation, coupling):
    s, b = gpu_pair(shape, K)
    raw, S = raw_kernel(b, s, K, regularisation, coupling)
    raw.setflags(write=False); S.setflags(write=False)
    return raw, S
