"""Drop-in for the parts of the reference's `lib/utils.py` that sit on the deconvolution path.

Same names and argument meaning as the reference (file:line in /root/reference/lib/utils.py):

    timeit                                   :30-42
    disc_blur, lens_blur                     :134-143
    uniform_kernel / gaussian_kernel /
    kaiser_kernel / poisson_kernel           :146-170   (host side: tiny separable windows)
    bilateral_filter(source, radius, std_i, std_s, parallel=1)      :194-234   -> HIP (ics_bilateral)
    bessel_blur(src, radius, amount)         :237-249   -> HIP (ics_conv2d_symm)
    gaussian_blur(src, radius, amount)       :252-264   -> HIP (ics_conv2d_symm)
    USM(src, radius, strength, amount, method="bessel")             :267-277   -> HIP (ics_usm)
    save(pic, name, dest_path)               :303-312   (16-bit RGB TIFF)
    convolve(a, b, domain)                   :420-447   (FFT convolution; unused by the reference)

The filters run on the GPU through libics_hip.so in float64 like the reference (scipy's
convolve2d(mode="same", boundary="symm")); there is no CPU fallback for them.  Given a `lib._native.DeviceImage`
(H x W x 3 float32 in HBM) instead of a 2-D array, the four filters work on it there, every channel on its own
in float32, and return a new DeviceImage (csrc/ics_img_filters.hip): no transfer, no synchronisation; `tv_denoise`,
`wavelet_equalizer`, `noise_estimate`, `despeckle`, `median_filter`, `guided_filter` and `local_laplacian` (not in the reference; csrc/ics_img_tvdenoise.hip, csrc/ics_img_wavelet.hip,
csrc/ics_img_despeckle.hip,
csrc/ics_img_guided.hip, csrc/ics_img_llf.hip) work on such an image or on an
H x W x 3 array.  The colour tools of
the reference (Lagrange_interpolation, grey_point, auto_vibrance, overlay, blending) and its dead
code (divTV, gradTVEM) are outside the deconvolution path and are not provided.

Notes on reference quirks that are kept:
  * `gaussian_kernel(radius, std)`: `radius` is the window SIZE (scipy.signal.gaussian(radius, std)).
  * `bilateral_filter` as shipped raises NameError (`gaussian` is undefined, :186-187); the intended
    gaussian(x, s) = exp(-x^2 / (2 s^2)) is used (any normalisation cancels in filtered / W).
"""
from __future__ import annotations

import collections
import math
import os
import struct
import time
from os.path import join

import numpy as np

from . import _native


def timeit(method):
    """lib/utils.py:30-42"""
    def timed(*args, **kw):
        ts = time.time()
        result = method(*args, **kw)
        te = time.time()
        print('%r %2.2f sec' % (method.__name__, te - ts))
        return result
    return timed


# ---- PSF window builders (host) ------------------------------------------------------------------
def disc_blur(x):
    half = [1 / (np.pi * x ** 2) for x in range(1, int(x / 2) + 1)]
    return half


def lens_blur(size):
    window = disc_blur(size)
    kern = np.outer(window, window)
    kern = kern / kern.sum()
    return kern


def uniform_kernel(size):
    kern = np.ones((size, size))
    kern /= np.sum(kern)
    return kern


def _gaussian_window(M, std):
    """scipy.signal.windows.gaussian(M, std, sym=True)"""
    if M < 1:
        return np.array([])
    if M == 1:
        return np.ones(1)
    n = np.arange(0, M) - (M - 1.0) / 2.0
    return np.exp(-n ** 2 / (2 * std * std))


def _exponential_window(M, tau):
    """scipy.signal.windows.exponential(M, center=None, tau=tau, sym=True)"""
    if M < 1:
        return np.array([])
    if M == 1:
        return np.ones(1)
    center = (M - 1) / 2
    n = np.arange(0, M)
    return np.exp(-np.abs(n - center) / tau)


def gaussian_kernel(radius, std):
    window = _gaussian_window(radius, std)
    kern = np.outer(window, window)
    kern = kern / kern.sum()
    return kern


def kaiser_kernel(radius, beta):
    window = np.kaiser(radius, beta)
    kern = np.outer(window, window)
    kern = kern / kern.sum()
    return kern


def poisson_kernel(radius, tau):
    window = _exponential_window(radius, tau)
    kern = np.outer(window, window)
    kern = kern / kern.sum()
    return kern


# ---- filters (GPU) -------------------------------------------------------------------------------
def _as2d(src):
    src = np.asarray(src)
    if src.ndim != 2:
        raise ValueError("expected a 2-D channel, got shape %s" % (src.shape,))
    return np.ascontiguousarray(src, dtype=np.float64)


def bilateral_filter(source, radius, std_i, std_s, parallel=1):
    """lib/utils.py:194-234: symmetric padding by `radius`, all (2r+1)^2 offsets,
    w = gaussian(neighbour - source, std_i) * gaussian(distance, std_s), result = sum(neighbour*w)/sum(w)."""
    if isinstance(source, _native.DeviceImage):
        return source.bilateral(radius, std_i, std_s)
    return _native.Context.get().bilateral(_as2d(source), int(radius), float(std_i), float(std_s))


def tv_denoise(src, weight=0.1, iterations=50, coupling="vector"):
    """Not in the reference's lib/utils.py (its README lists "TV denoise" among what may come): Rudin-Osher-Fatemi denoising
    min_u 1/2 |u - src|^2 + weight * TV(u) by `iterations` steps of Chambolle's dual projection (tau = 1/8, no early stop) on the
    device, float32.  coupling "vector" ties the three channels to one edge set, "channel" treats each on its own.  A
    `lib._native.DeviceImage` gives a new DeviceImage (nothing crosses PCIe); an H x W x 3 array is uploaded once and the float32
    result downloaded once.  Parity with skimage.restoration.denoise_tv_chambolle (tau = 1/4, energy stop) is unpinned."""
    if isinstance(src, _native.DeviceImage):
        return src.tv_denoise(weight, iterations, coupling)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.tv_denoise(weight, iterations, coupling)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


def wavelet_equalizer(src, gains, thresholds=None, residual=1.0, coupling="vector"):
    """Not in the reference's lib/utils.py (its README advises to add local contrast "through wavelets high-pass filter" after the
    deconvolution, and lists wavelet denoising among what may come): the picture is split into len(gains) <= 8 detail scales by the
    undecimated B3-spline ("a trous") transform, scale j holding the detail of about 2^j pixels; every scale is soft-thresholded by
    thresholds[j] (None: 0) and multiplied by gains[j], and the scales are summed back onto residual * the coarsest approximation.
    gains=[1, 1.6, 1.8, 1.4, 1] lifts the 2 - 8 px contrast and leaves the 1 px noise alone; gains=[1] * 5 with
    thresholds=[0.03, 0.015, 0, 0, 0] removes noise from the two finest scales only.  coupling "vector" shrinks the three channels
    of a pixel together (no hue shift), "channel" each on its own.  A `lib._native.DeviceImage` gives a new DeviceImage (nothing
    crosses PCIe); an H x W x 3 array is uploaded once and the float32 result downloaded once (`DeviceImage.wavelet_equalize`,
    csrc/ics_img_wavelet.hip).  thresholds="auto" or ("auto", strength) takes them from `noise_estimate` of this picture with the same
    coupling: strength (3 unless given) standard deviations of its noise at every scale, estimated on the device from the resident
    frame (only a few floats come back)."""
    if isinstance(src, _native.DeviceImage):
        return src.wavelet_equalize(gains, thresholds, residual, coupling)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.wavelet_args(gains, thresholds, residual, coupling)        # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.wavelet_equalize(gains, thresholds, residual, coupling)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


def noise_estimate(src, coupling="vector"):
    """Not in the reference's lib/utils.py (its README calls its algorithms "auto-adaptative, meaning that all the regularization
    parameters are estimated by the algorithm based on statistical assumptions"; this does it for the filters that follow the
    deconvolution): the noise of a picture from the finest scale of the B3-spline wavelet transform, by the median of its absolute
    value (Donoho and Johnstone) -- robust against the edges and texture that a standard deviation would count as noise.  Returns
    `lib._native.NoiseEstimate(median, level, sigma)`: tuples of three floats (R, G, B) for coupling "channel", of one for "vector"
    (the magnitude over the three channels).  sigma is the standard deviation per channel of white noise that would give this
    median; level is the rms of the quantity `wavelet_equalizer` thresholds at its finest scale, so that thresholds="auto" there is
    `lib._native.auto_thresholds(level, scales)`.  A `lib._native.DeviceImage` is read where it lies; an H x W x 3 array is uploaded
    once and nothing but the result floats comes back (`DeviceImage.noise_estimate`, csrc/ics_img_noise.hip)."""
    if isinstance(src, _native.DeviceImage):
        return src.noise_estimate(coupling)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.noise_args(coupling)                                         # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        return img.noise_estimate(coupling)
    finally:
        img.close()


BlurWidth = collections.namedtuple("BlurWidth", "width extent_x extent_y")


def blur_width_args(max_width=63):
    """`max_width` of estimate_blur_width checked (ValueError): an odd integer, 3 to IMG_BLURWIDTH_MAX_LAG - 1"""
    top = _native.IMG_BLURWIDTH_MAX_LAG - 1
    try:
        whole = int(max_width) == max_width and not isinstance(max_width, bool)
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or not 3 <= int(max_width) <= top or int(max_width) % 2 == 0:
        raise ValueError("max_width %r (an odd integer, 3 to %d)" % (max_width, top))
    return int(max_width)


def estimate_blur_width(src, max_width=63, window=None):
    """Not in the reference, whose driver leaves it open (deconvolve.py:122, "TODO : automatically evaluate blur size") while its README
    names an ill-chosen blur size as what keeps a pyramid step from converging: the `blur_width` of `deblur_module` from the picture.
    The derivative of a sharp picture is close to white along its axis, so the derivative of a blurred one correlates with itself
    over as many pixels as the PSF is wide (Yitzhaky and Kopeika).  The autocorrelation of the luma's differences along x and along
    y is taken on the device, lags 0 .. max_width + 1 (`DeviceImage.blur_profile`, csrc/ics_img_blurwidth.hip); the host reads the
    base of each profile's triangle (`lib._native.blur_extent`: half-maximum line fit, lags 0 and 1 left to the picture's noise).
    Returns BlurWidth(width, extent_x, extent_y): the extents in pixels and width = the smallest odd integer at or above the larger
    one, 3 at least.  window (y0, y1, x0, x1), half-open: the region to look at (None: the whole frame).  A `lib._native.DeviceImage`
    is read where it lies; an H x W x 3 array is uploaded once and only the profiles come back.  It cannot see a blur thinner than its
    projection on the axes (a diagonal line reads as its extents along x and y), a defocus that varies over the frame (it reads an average), or a
    picture that was never sharp (its own softness adds to the width).  ValueError: max_width not an odd integer in 3 .. 127, a bad
    window, a frame with NaN or inf (despeckle first), and "blur wider than max_width" where a profile does not end within the lags."""
    max_width = blur_width_args(max_width)
    if isinstance(src, _native.DeviceImage):
        img, own = src, False
        _native.blur_profile_args(max_width + 1, window, img.shape)
    else:
        arr = np.asarray(src)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
        _native.blur_profile_args(max_width + 1, window, arr.shape)         # refused before anything is uploaded
        img, own = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32)), True
    try:
        prof = img.blur_profile(max_width + 1, window)
    finally:
        if own:
            img.close()
    ex, ey = _native.blur_extent(prof.ax), _native.blur_extent(prof.ay)
    if max(ex, ey) == _native.BLUR_SATURATED:
        raise ValueError("blur wider than max_width = %d (a profile does not end within %d lags): raise max_width" % (max_width, max_width + 1))
    width = _native.blur_width_from(prof.ax, prof.ay)
    if width > max_width:
        raise ValueError("blur wider than max_width = %d (x %.2f, y %.2f)" % (max_width, ex, ey))
    return BlurWidth(width, ex, ey)


BlurMap = _native.BlurMap


def _blur_map_edge_form(edge):
    """`edge` of blur_map -> (None, the number) or (strength, None) for "auto" / ("auto", strength), checked (ValueError)"""
    if isinstance(edge, str):
        if edge != "auto":
            raise ValueError("edge %r (a number above 0, \"auto\" or (\"auto\", strength))" % (edge,))
        return 5.0, None
    if isinstance(edge, (tuple, list)):
        if len(edge) != 2 or edge[0] != "auto":
            raise ValueError("edge %r (a number above 0, \"auto\" or (\"auto\", strength))" % (edge,))
        return _native._strength(edge[1]), None
    return None, edge


def blur_map(src, sigmas=(1.0, 2.0), edge=0.02, max_sigma=8.0, window=None, sparse=False, fill=False):
    """Not in the reference, whose README lists local blur estimation first under what may come one day and motivates its mask with
    "cases where the PSF varies spatially": a map of the local blur width of the picture, to see where the defocus lies before a
    box is chosen for the PSF (`best_mask(blur=...)`).  Zhuo and Sim's gradient-ratio defocus map: the luma is smoothed by two
    Gaussians sigmas = (sigma_a, sigma_b); at an edge pixel of a step blurred by a Gaussian of s the two gradient magnitudes stand in
    the ratio R = sqrt((s^2 + sigma_b^2) / (s^2 + sigma_a^2)), which is solved for s.  Edge pixels are the local maxima of the
    gradient along its direction at or above `edge`, readings above `max_sigma` are dropped, and the readings are averaged, weighted
    by the gradient, over cells of 16 x 16 pixels from the window's origin (`DeviceImage.blur_map`, csrc/ics_img_blurmap.hip: one
    launch, local, no PSF, a fixed cost).  Returns `lib._native.BlurMap(sigma, weight, count, pixels)`: sigma float64 per cell, NaN
    where the cell holds no edge (fill=True: filled from the nearest cells that hold one, `lib._native.blur_map_fill`); weight the sum
    of the gradient magnitudes; count the edge pixels; pixels the h x w plane of the readings (-1 where none) with sparse=True, else
    None.  edge="auto" or ("auto", strength) (strength 5 unless given): `strength` standard deviations of the gradient under the
    frame's noise (`noise_estimate(src, "vector")` on the same frame, `lib._native.blur_map_edge`).  window (y0, y1, x0, x1),
    half-open: the region to map (None: the whole frame).  A `lib._native.DeviceImage` is read where it lies; an H x W x 3 array is
    uploaded once and only the grid (and the plane) comes back.  It reports a sigma of Gaussian equivalence, not a PSF; it reads a
    sharp edge as about 0.5 to 0.8, underestimates above about 2 sigma_b, assumes isolated step edges (texture finer than sigma_b
    reads low) and is blind where no edge passes `edge`.  ValueError: sigmas outside 0.5 <= sigma_a < sigma_b with ceil(3 sigma_b) <=
    8, edge or max_sigma not above 0, a bad window, a window with NaN or inf ("not finite: despeckle first")."""
    strength, number = _blur_map_edge_form(edge)
    if isinstance(src, _native.DeviceImage):
        img, own = src, False
        _native.blur_map_args(sigmas, 1.0 if number is None else number, max_sigma, window, img.shape)
    else:
        arr = np.asarray(src)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
        _native.blur_map_args(sigmas, 1.0 if number is None else number, max_sigma, window, arr.shape)   # refused before anything is uploaded
        img, own = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32)), True
    try:
        if number is None:
            number = _native.blur_map_edge(noise_estimate(img, "vector").sigma[0], sigmas[0], strength)
        got = img.blur_map(sigmas, number, max_sigma, window, sparse)
    finally:
        if own:
            img.close()
    return got._replace(sigma=_native.blur_map_fill(got)) if fill else got


MaskChoice = collections.namedtuple("MaskChoice", "center_y center_x score trace clipped")
MaskChoiceBlur = collections.namedtuple("MaskChoiceBlur", "center_y center_x score trace clipped sigma")


def mask_blur_args(blur):
    """`blur` of best_mask checked (ValueError) and as (lo, hi): two finite numbers, 0 <= lo <= hi"""
    try:
        lo, hi = (float(v) for v in blur)
        ok = not any(isinstance(v, (bool, str)) for v in blur) and 0 <= lo <= hi < math.inf
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("blur %r ((lo, hi), two finite numbers, 0 <= lo <= hi: the range of the box's blur width)" % (blur,))
    return lo, hi


def best_mask_args(mask_size, clip, region, shape):
    """the arguments of best_mask checked (ValueError, without a device) and as (box side, region, clip): the box deblur_module cuts
    for `mask_size` is 2 (mask_size // 2) + 1 pixels a side"""
    try:
        whole = int(mask_size) == mask_size and not isinstance(mask_size, bool)
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or 2 * (int(mask_size) // 2) + 1 < _native.IMG_MASK_CELL:
        raise ValueError("mask_size %r (an integer, at least %d)" % (mask_size, _native.IMG_MASK_CELL))
    return _native.window_scores_args(2 * (int(mask_size) // 2) + 1, region, clip, shape)


def best_mask(src, mask_size=255, clip=0.99, region=None, blur=None):
    """Not in the reference, whose README has the user select "a specific zone to refine the PSF": the `mask` of `deblur_module` from
    the picture.  The blind phase estimates the PSF on one box of the frame; a box of sky or bokeh gives it nothing to estimate from,
    a box with one dominant edge direction leaves the PSF free along that direction, and clipped pixels break the linear blur model
    Richardson-Lucy assumes.  The box chosen is the one whose structure tensor of luma differences has the largest SMALLER eigenvalue
    (Shi and Tomasi's criterion on a whole window), pixels with a channel at or above `clip` left out (`DeviceImage.window_scores`,
    csrc/ics_img_mask.hip).  Returns MaskChoice(center_y, center_x, score, trace, clipped): the centre to pass as `mask=` with this
    `mask_size` (box origin + mask_size // 2, the box being 2 (mask_size // 2) + 1 pixels a side), the box's score and mean squared
    gradient, and the fraction of the scored pixels that are clipped.  region (y0, y1, x0, x1), half-open: where the box may lie
    (None: the whole frame).  A `lib._native.DeviceImage` is read where it lies; an H x W x 3 array is uploaded once and a few numbers
    come back.  It ranks boxes on a 16-px grid from the region's origin, scores the inner 16 (side // 16) pixels of a box, and
    prefers the sharpest textured zone: under a blur that varies over the frame that is the zone in focus, not necessarily the
    subject.  blur=(lo, hi) tells it which blur to look for: the candidates' scores (`window_scores(..., scores=True)`) and the
    blur map of the same region (`blur_map` at its defaults, `lib._native.blur_map_box_sigma`: the weighted mean reading of the
    box's cells) are taken, and the best-scoring box whose blur width lies in [lo, hi] is returned, ties as before, as
    MaskChoiceBlur(center_y, center_x, score, trace, clipped, sigma), sigma being the box's blur width.  ValueError: mask_size
    below 16, a bad region or one smaller than the box, clip not above 0, a bad blur range, "no box with a blur in ..." where none
    qualifies."""
    if blur is not None:
        blur = mask_blur_args(blur)
    if isinstance(src, _native.DeviceImage):
        img, own = src, False
        size, region, clip = best_mask_args(mask_size, clip, region, img.shape)
    else:
        arr = np.asarray(src)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
        size, region, clip = best_mask_args(mask_size, clip, region, arr.shape)   # refused before anything is uploaded
        img, own = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32)), True
    try:
        got = img.window_scores(size, region, clip, scores=blur is not None)
        if blur is not None:
            sig = _native.blur_map_box_sigma(img.blur_map(window=region), size, (region[1] - region[0], region[3] - region[2]))
            ok = (sig >= blur[0]) & (sig <= blur[1])                        # (NaN: a box without an edge never qualifies)
            if not ok.any():
                raise ValueError("no box with a blur in [%g, %g] (the boxes read %s)" % (
                    blur[0], blur[1], "nothing" if np.isnan(sig).all() else "%.2f to %.2f" % (np.nanmin(sig), np.nanmax(sig))))
            i, j = divmod(int(np.argmax(np.where(ok, got.map, -1.0))), sig.shape[1])   # the largest score, ties to the lowest row, then column
            by, bx, sigma = region[0] + _native.IMG_MASK_CELL * i, region[2] + _native.IMG_MASK_CELL * j, float(sig[i, j])
            got = img.window_scores(size, (by, by + size, bx, bx + size), clip)        # the box alone: its score again, its trace and clipped count
    finally:
        if own:
            img.close()
    scored = float(_native.IMG_MASK_CELL * (size // _native.IMG_MASK_CELL)) ** 2
    if blur is not None:
        return MaskChoiceBlur(got.box_y + size // 2, got.box_x + size // 2, got.score, got.trace, got.clipped / scored, sigma)
    return MaskChoice(got.box_y + size // 2, got.box_x + size // 2, got.score, got.trace, got.clipped / scored)


def despeckle(src, threshold, radius=1, coupling="vector", count=False):
    """Not in the reference's lib/utils.py, which has no rank filter: a thresholded median for the frame BEFORE the deconvolution.
    Richardson-Lucy treats a hot pixel as signal and turns it into a PSF-sized ring; a NaN spreads over the frame.  A value is
    replaced by the median of its (2 radius + 1)^2 window (radius 1 or 2) where it is further than `threshold` from it (or the
    difference is NaN) and is otherwise returned bit for bit; a frame blurred by a PSF of 3 px or more holds no real one-pixel
    detail, so nothing else is flagged.  threshold: one value (pixel values in [0, 1]), three for coupling "channel", or "auto" /
    ("auto", strength): strength (6 unless given) times the sigma of `noise_estimate` of this picture.  coupling "vector" replaces
    all three channels of a pixel flagged in one, "channel" treats every channel by itself.  count=True returns (result, counts):
    what was replaced.  A `lib._native.DeviceImage` gives a new DeviceImage (nothing crosses PCIe); an H x W x 3 array is uploaded
    once and the float32 result downloaded once (`DeviceImage.despeckle`, csrc/ics_img_despeckle.hip)."""
    if isinstance(src, _native.DeviceImage):
        return src.despeckle(threshold, radius, coupling, count=count)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.despeckle_args(threshold, radius, coupling)                  # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res, counts = img.despeckle(threshold, radius, coupling, count=True)
    finally:
        img.close()
    try:
        return (res.to_host(), counts) if count else res.to_host()
    finally:
        res.close()


def median_filter(src, radius=1):
    """Not in the reference's lib/utils.py: the median of the (2 radius + 1)^2 window (radius 1 or 2, coordinates clamped at the
    border) of every channel, `despeckle` with threshold 0.  The median is selected by the integer order of the float bits, so it is
    defined for every input (NaN sorts at the ends) and is one of the window's values.  DeviceImage in, DeviceImage out; an
    H x W x 3 array is uploaded once and the float32 result downloaded once."""
    return despeckle(src, 0.0, radius, "channel")


def guided_filter(src, radius, eps, detail=0.0, coupling="vector"):
    """Not in the reference's lib/utils.py (its bilateral_filter serves img/bilateral-unsharp-mask/ as the edge-aware base of a
    sharpening, at (2 radius + 1)^2 exponentials per pixel): He, Sun and Tang's guided filter with the picture as its own guide.
    q is the edge-preserving base layer of the (2 radius + 1)^2 box windows, radius 1 .. 32; the result is q + detail * (src - q):
    detail 0 the base layer itself, detail 1.5 with radius 16 and eps 1e-3 a halo-free sharpening of a deblurred frame, detail 0.5
    with radius 8 and eps 1e-2 a smoothing that leaves edges alone.  eps is the variance below which a window counts as flat.
    coupling "vector" guides with the RGB pixel (one set of edges for all channels), "channel" every channel by itself.  A
    `lib._native.DeviceImage` gives a new DeviceImage (nothing crosses PCIe); an H x W x 3 array is uploaded once and the float32
    result downloaded once (`DeviceImage.guided_filter`, csrc/ics_img_guided.hip)."""
    if isinstance(src, _native.DeviceImage):
        return src.guided_filter(radius, eps, detail, coupling)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.guided_args(radius, eps, detail, coupling)                  # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.guided_filter(radius, eps, detail, coupling)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


def wiener(src, psf, balance=0.01):
    """Not in the reference's lib/utils.py (its only deconvolution is the iterative loop; `skimage.restoration`, where it takes its
    other tools from, ships this one beside Richardson-Lucy): Wiener deconvolution of a picture by a known PSF in one pass over the
    frequency domain, regularised by `balance` times the squared transfer of the Laplacian as `skimage.restoration.wiener` does by
    default.  psf: K x K or K x K x 3, K odd, 3 .. 255 -- the `psf` that `deblur_module` returns, or one you already hold; every
    channel is normalised to sum 1.  Milliseconds where the loop takes tenths of a second, at the price of ringing the loop's prior
    would have damped: no positivity (negative lobes beside edges), exact spectral zeros of box and line PSFs carried by `balance`
    alone, and a NaN spread over the whole frame (despeckle first).  A `lib._native.DeviceImage` gives a new DeviceImage (nothing
    crosses PCIe); an H x W x 3 array is uploaded once and the float32 result downloaded once (`DeviceImage.wiener`,
    csrc/ics_img_wiener.hip)."""
    if isinstance(src, _native.DeviceImage):
        return src.wiener(psf, balance)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.wiener_args(psf, balance, arr.shape)                        # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.wiener(psf, balance)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


class PsfEstimate(collections.namedtuple("PsfEstimate", "psf raw rejected")):
    """what estimate_psf(info=True) returns; `matrix`: with register=, the 3 x 3 matrix that takes a pixel of `blurred` to its position in `sharp` (else None).  It is an attribute
    of the instance, not a field: the three fields stay what they were, and `_replace`, `_make`, slicing and `==` do not carry or compare it"""
    matrix = None


Alignment = _native.Alignment


def _pair_on_device(a, b, names):
    """two DeviceImages read where they lie, or two H x W x 3 arrays: (a, b, arrays or None) -- nothing is uploaded here"""
    dev = [isinstance(v, _native.DeviceImage) for v in (a, b)]
    if dev[0] != dev[1]:
        raise ValueError("%s and %s must both be DeviceImages or both H x W x 3 arrays" % names)
    if all(dev):
        return a, b, None
    arrays = (np.asarray(a), np.asarray(b))
    for arr in arrays:
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("expected two DeviceImages or two H x W x 3 arrays, got shape %s" % (arr.shape,))
    return arrays[0], arrays[1], arrays


def _upload_pair(arrays):
    a = _native.DeviceImage.from_host(np.ascontiguousarray(arrays[0], dtype=np.float32))
    try:
        b = _native.DeviceImage.from_host(np.ascontiguousarray(arrays[1], dtype=np.float32))
    except Exception:
        a.close()
        raise
    return a, b


def align(moving, fixed, model="affine", photometric=True, levels=None, iterations=30, tolerance=1e-3, init=None, window=None, info=False):
    """Not in the reference's lib/utils.py (its README lists "Lens PSF calibration" under what may come one day; `estimate_psf` is one half
    of it, this the other): registers `moving` to `fixed` and returns the 3 x 3 float64 matrix that takes a pixel (x, y, 1) of `fixed`
    to its position in `moving` -- `warp(moving, matrix, fixed.shape)` then lies on `fixed`.  Coarse-to-fine Gauss-Newton on the luma
    (forward-additive Lucas-Kanade, Levenberg's damping; `DeviceImage.align`, csrc/ics_img_align.hip): model "translation", "affine"
    or "homography"; photometric: a gain and a bias between the frames are estimated with it (two exposures); levels None: halve
    while the smaller side stays >= 64 px; init: a start (None: the identity); window (y0, y1, x0, x1): the region of `fixed` to
    look at.  info=True: Alignment(matrix, gain, bias, rms, coverage, steps).  Two `lib._native.DeviceImage`s are read where they
    lie; two H x W x 3 arrays, which may differ in shape, are uploaded once each.  It cannot align through a blur so strong that no
    level holds texture, a motion beyond about a tenth of the frame without `init`, periodic patterns (a local minimum), parallax,
    rolling shutter or lens distortion; a strongly asymmetric PSF shifts the registration by its centroid.  ValueError: a DeviceImage
    with an array, bad arguments (before anything is uploaded), frames that are not finite, do not overlap enough or hold no
    texture.  There is no CPU fallback."""
    m, f, arrays = _pair_on_device(moving, fixed, ("moving", "fixed"))
    _native.align_args(model, photometric, levels, iterations, tolerance, init, window, m.shape, f.shape)      # refused before anything is uploaded
    if arrays is not None:
        m, f = _upload_pair(arrays)
    try:
        got = m.align(f, model, photometric, levels, iterations, tolerance, init, window)
    finally:
        if arrays is not None:
            m.close(); f.close()
    return got if info else got.matrix


def warp(src, matrix, shape=None):
    """Not in the reference's lib/utils.py: `src` seen through the 3 x 3 matrix, out[y][x] = src sampled at matrix (x, y, 1), by Keys'
    cubic convolution over 4 x 4 taps, the edge repeated beyond the frame (`DeviceImage.warp`, csrc/ics_img_align.hip); shape (H, W):
    that of the result (None: that of `src`).  A `lib._native.DeviceImage` gives a new DeviceImage, an H x W x 3 array is uploaded
    once and gives a float32 array.  ValueError: a matrix that is not 3 x 3, not finite or singular.  There is no CPU fallback."""
    if isinstance(src, _native.DeviceImage):
        return src.warp(matrix, shape)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native._matrix(matrix)                                           # refused before anything is uploaded
    if shape is not None and (len(shape) < 2 or int(shape[0]) < 1 or int(shape[1]) < 1):
        raise ValueError("shape %r (H, W at least 1)" % (shape,))
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.warp(matrix, shape)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


def estimate_psf(blurred, sharp, size, regularisation=1e-3, threshold=0.05, coupling="vector", window=None, info=False, register=None):
    """Not in the reference's lib/utils.py, whose only way to a PSF is the blind loop: the PSF from a picture and a sharper rendering of
    the same scene -- a test chart and its photograph, a frame stopped down and the same frame wide open, a synthetic target -- or the
    check of a PSF the blind phase returned against the frame it produced.  The linear solve every fast blind method repeats (Cho and
    Lee 2009; Xu and Jia 2010): k = argmin sum |d sharp * k - d blurred|^2 + regularisation S |k|^2 on the derivatives of the pair,
    tapered at the border, diagonal under the transform of `wiener` (`DeviceImage.psf_raw`, csrc/ics_img_psfest.hip); the taps below
    threshold times the largest are then cut and the rest normalised to sum 1 (`lib._native.psf_project`).  Returns the size x size x 3
    float32 PSF, ready for `wiener` / `tv_deconvolve` / `tv_deconvolve_masked`; info=True: PsfEstimate(psf, raw, rejected), the raw
    kernel and the share of its weight that the threshold cut, per channel.  size odd, 3 .. 255; coupling "vector": one PSF from the
    three channels, "channel": one each; window (y0, y1, x0, x1), half-open: the region to look at (None: the whole frame).  Two
    `lib._native.DeviceImage`s are read where they lie; two H x W x 3 arrays are uploaded once each; only the raw kernel and the energy
    come back.  Without `register=` (below) it cannot register the pair (`sharp` must lie on `blurred` to the pixel); it gives the relative PSF where `sharp` is
    itself blurred, leaves the PSF free along a direction in which `sharp` has no gradients, and a NaN spreads (despeckle first).
    ValueError: a DeviceImage with an array, frames of different shapes, bad arguments (before anything is uploaded), a raw kernel or
    energy that is not finite, a sharp frame with no gradients.  There is no CPU fallback.
    register "translation", "affine" or "homography": `sharp`, of any shape, is first registered to `blurred` (`align`, on the window,
    with a gain and a bias) and warped onto it, one line is printed, and the estimate proceeds on the warped frame; info=True then
    carries the matrix as `PsfEstimate.matrix`.  None: the frames are taken as registered."""
    if register is not None:
        return _estimate_psf_registered(blurred, sharp, size, regularisation, threshold, coupling, window, info, register)
    dev = [isinstance(v, _native.DeviceImage) for v in (blurred, sharp)]
    if dev[0] != dev[1]:
        raise ValueError("blurred and sharp must both be DeviceImages or both H x W x 3 arrays")
    if all(dev):
        b, s, own = blurred, sharp, False
        size, regularisation, threshold, coupling, window = _native.psf_estimate_args(size, regularisation, threshold, coupling, window, b.shape, s.shape)
    else:
        ab, asharp = np.asarray(blurred), np.asarray(sharp)
        for arr in (ab, asharp):
            if arr.ndim != 3 or arr.shape[2] != 3:
                raise ValueError("expected two DeviceImages or two H x W x 3 arrays, got shape %s" % (arr.shape,))
        size, regularisation, threshold, coupling, window = _native.psf_estimate_args(size, regularisation, threshold, coupling, window, ab.shape, asharp.shape)   # refused before anything is uploaded
        b = _native.DeviceImage.from_host(np.ascontiguousarray(ab, dtype=np.float32))
        try:
            s = _native.DeviceImage.from_host(np.ascontiguousarray(asharp, dtype=np.float32))
        except Exception:
            b.close()
            raise
        own = True
    try:
        raw, _ = b.psf_raw(s, size, regularisation, coupling, window)
    finally:
        if own:
            b.close(); s.close()
    psf, rejected = _native.psf_project(raw, threshold)
    return PsfEstimate(psf, raw, rejected) if info else psf


BlindPsf = collections.namedtuple("BlindPsf", "psf levels kept rejected")


def blind_psf(src, size, iterations=5, shock=(4, 0.4, 0.01), keep=2.0, regularisation=1e-3, threshold=0.05, balance=0.01, coupling="vector", window=None,
              info=False):
    """Not in the reference's lib/utils.py, whose only way to a PSF is the blind Richardson-Lucy loop: the PSF of one blurred picture by
    the fast alternation of Cho and Lee (2009), milliseconds where the loop takes tenths of a second.  Coarse to fine -- K_0 = size,
    K_{l+1} = max(3, (K_l // 2) | 1), level l on the window resized to ceil(H / 2^l) x ceil(W / 2^l), levels whose smaller side is below
    4 K_l dropped -- and on every level `iterations` times: latent = `wiener`(frame, psf, balance) (the frame itself before there is a
    PSF); p = latent.shock(*shock), the ramps of blurred edges steepened into steps; mask = p.edge_mask(per_sector), the gradients worth
    trusting, the same number per orientation; raw = frame.psf_raw(p, K_l, regularisation, coupling, mask=mask), the linear solve
    argmin sum |M d p * k - d frame|^2 + gamma |k|^2; psf = `lib._native.psf_project`(raw, threshold), moved by whole pixels so that its
    centroid rounds to the centre (`lib._native.psf_centred`: the solve fixes the PSF only up to a shift it shares with p).  per_sector
    starts at ceil(keep sqrt(H_l W_l) K_l / 4) and grows by 1 / 0.9 per iteration; between levels the PSF is resized like the driver's,
    clipped at 0 and normalised.  Returns the size x size x 3 float32 PSF, every plane of sum 1; info=True: BlindPsf(psf, levels, kept,
    rejected) with the (K, H, W) of every level, the pixels its last mask kept and the share of the raw kernel its last projection cut.
    A `lib._native.DeviceImage` is read where it lies (window (y0, y1, x0, x1), half-open: the region to look at); an H x W x 3 array is
    uploaded once; per iteration only the K x K x 3 raw kernel crosses to the host; every frame, mask and workspace goes back to the
    context's pool on every way out.  tests/edges_ref.py restates it.  It serves compact PSFs: it does not recover one-pixel-wide motion
    lines on small cluttered frames, structures smaller than the PSF, or a blur that varies over the window (README).  ValueError, before
    anything is uploaded where the arguments show it: size even or outside 3 .. 255, a window smaller than 4 size, bad arguments, a frame
    that is "not finite: despeckle first", "no gradients to select".  NativeError (ICS_ENOSUP): the transform limits of `wiener`.  There
    is no CPU fallback."""
    dev = isinstance(src, _native.DeviceImage)
    if not dev:
        arr = np.asarray(src)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    shape = src.shape if dev else arr.shape
    size, iterations, shock, keep, regularisation, threshold, balance, coupling, (y0, y1, x0, x1), levels = _native.blind_psf_args(
        size, iterations, shock, keep, regularisation, threshold, balance, coupling, window, shape)
    if not dev and not np.isfinite(arr[y0:y1, x0:x1]).all():
        raise ValueError("the frame is not finite: despeckle first")
    import contextlib
    with contextlib.ExitStack() as held:
        def hold(obj, stack=held):
            stack.callback(obj.close)
            return obj
        if dev:
            base = src if (y0, y1, x0, x1) == (0, shape[0], 0, shape[1]) else hold(src.crop(y0, y1, x0, x1))
        else:
            base = hold(_native.DeviceImage.from_host(np.ascontiguousarray(arr[y0:y1, x0:x1], dtype=np.float32)))
        H, W = y1 - y0, x1 - x0
        psf, kept, rejected = None, [], []
        for K, Hl, Wl in levels:
            with contextlib.ExitStack() as level:
                frame = base if (Hl, Wl) == (H, W) else hold(base.resize(Hl, Wl), level)
                if psf is not None:
                    up = np.maximum(base.ctx.resize_bicubic(np.ascontiguousarray(psf, dtype=np.float64), (K, K)), 0.0)
                    psf = np.ascontiguousarray(up / up.sum(axis=(0, 1)), dtype=np.float32)
                per_sector = float(np.ceil(keep * np.sqrt(Hl * Wl) * K / 4))
                for _ in range(iterations):
                    with contextlib.ExitStack() as step:
                        latent = frame if psf is None else hold(frame.wiener(psf, balance), step)
                        p = hold(latent.shock(*shock, coupling), step)
                        try:
                            got = p.edge_mask(int(np.ceil(per_sector)), coupling)
                        except ValueError:       # (a NaN spreads over a whole coarse level; on this way out only, the window is looked at)
                            if not np.isfinite(base.to_host()).all():
                                raise ValueError("the frame is not finite: despeckle first")
                            raise
                        hold(got.mask, step)
                        try:
                            raw, _ = frame.psf_raw(p, K, regularisation, coupling, mask=got.mask)
                        except ValueError as exc:
                            if "not finite" in str(exc):
                                raise ValueError("the frame is not finite: despeckle first")
                            raise
                    try:
                        projected, rej = _native.psf_project(raw, threshold)
                    except ValueError as exc:
                        if "not finite" in str(exc):
                            raise ValueError("the frame is not finite: despeckle first")
                        raise
                    psf = _native.psf_centred(projected)
                    per_sector /= 0.9
                kept.append(got.kept)
                rejected.append(rej)
    return BlindPsf(psf, levels, kept, rejected) if info else psf


def _estimate_psf_registered(blurred, sharp, size, regularisation, threshold, coupling, window, info, register):
    """estimate_psf(register=...): align `sharp` to `blurred`, warp it to the shape of `blurred`, estimate"""
    b, s, arrays = _pair_on_device(blurred, sharp, ("blurred", "sharp"))
    size, regularisation, threshold, coupling, window = _native.psf_estimate_args(size, regularisation, threshold, coupling, window, b.shape, b.shape)
    _native.align_args(register, True, None, 30, 1e-3, None, window, s.shape, b.shape)                          # refused before anything is uploaded
    if arrays is not None:
        b, s = _upload_pair(arrays)
    warped = None
    try:
        got = s.align(b, register, True, window=window)
        print("Register : %s, %.2g px last step, rms %.4f, coverage %.0f %%" % (register, got.last_step, got.rms, 100.0 * got.coverage))
        warped = s.warp(got.matrix, b.shape)
        raw, _ = b.psf_raw(warped, size, regularisation, coupling, window)
    finally:
        if warped is not None:
            warped.close()
        if arrays is not None:
            b.close(); s.close()
    psf, rejected = _native.psf_project(raw, threshold)
    if not info:
        return psf
    res = PsfEstimate(psf, raw, rejected)
    res.matrix = got.matrix
    return res


def tv_deconvolve(src, psf, fidelity=2000.0, penalty=10.0, iterations=10, coupling="vector"):
    """Not in the reference's lib/utils.py: deconvolution of a picture by a known PSF under the total-variation prior the loop itself
    uses, by the fast splitting method (FTVd, Wang, Yang, Yin, Zhang 2008; split Bregman, Goldstein and Osher 2009) -- `iterations`
    times one shrinkage of the gradient per pixel and one solve in the frequency domain, on the transform of `wiener`.  It sits
    between the two: `wiener` has no image prior, the loop takes most of a `deblur_module` call.  psf: K x K or K x K x 3, K odd,
    3 .. 255 -- the `psf` that `deblur_module` returns, or one you already hold; every channel is normalised to sum 1.  fidelity
    trades noise against sharpness: 2000 for a clean frame, lower for a noisier one; the defaults come from synthetic frames with
    noise of sigma 0.002 (`DeviceImage.tv_deconvolve` has the figures).  coupling "vector" shrinks the three channels by their
    common gradient magnitude (the reference's "handcuffs between channels"), "channel" each by its own.  Nothing is clipped.  A
    `lib._native.DeviceImage` gives a new DeviceImage (nothing crosses PCIe); an H x W x 3 array is uploaded once and the float32
    result downloaded once (csrc/ics_img_tvdeconv.hip).  There is no CPU fallback."""
    if isinstance(src, _native.DeviceImage):
        return src.tv_deconvolve(psf, fidelity, penalty, iterations, coupling)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.tv_deconvolve_args(psf, fidelity, penalty, iterations, coupling, arr.shape)     # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.tv_deconvolve(psf, fidelity, penalty, iterations, coupling)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


def tv_deconvolve_masked(src, psf, observed=None, clip=None, fidelity=2000.0, penalty=10.0, data_penalty=None, iterations=10, coupling="vector", count=False):
    """Not in the reference's lib/utils.py: `tv_deconvolve` with a masked data term -- what is not data is not fitted (Almeida and
    Figueiredo, "Deconvolving images with unknown boundaries using the alternating direction method of multipliers", 2013).  Always
    unobserved: the pixels beyond the frame's edges, which `tv_deconvolve` extends by a ramp and then fits, and every pixel with a NaN
    or an infinity in it; with clip (0.99 for a picture scaled to 1): the clipped highlights, which otherwise ring; with observed, an
    H x W array: every pixel where it is 0.  psf, fidelity, penalty, iterations, coupling as for `tv_deconvolve`; data_penalty ties
    the blurred estimate to its splitting variable (None: fidelity).  The unknown edges pay at once, 9 to 20 % less rms error at 10
    iterations on the synthetic frames; near clipped lights the mask pays only from about 30 iterations.  Nothing is clipped and
    nothing keeps the result positive.  count=True: (result, unobserved pixels of the frame).  A `lib._native.DeviceImage` gives a new
    DeviceImage (only the mask crosses PCIe); an H x W x 3 array is uploaded once and the float32 result downloaded once
    (csrc/ics_img_tvmdeconv.hip).  There is no CPU fallback."""
    if isinstance(src, _native.DeviceImage):
        return src.tv_deconvolve_masked(psf, observed, clip, fidelity, penalty, data_penalty, iterations, coupling, count)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.tv_deconvolve_masked_args(psf, observed, clip, fidelity, penalty, data_penalty, iterations, coupling, arr.shape)     # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res, n = img.tv_deconvolve_masked(psf, observed, clip, fidelity, penalty, data_penalty, iterations, coupling, count=True)
    finally:
        img.close()
    try:
        return (res.to_host(), n) if count else res.to_host()
    finally:
        res.close()


def local_laplacian(src, sigma, detail, edges=1.0, levels=None, samples=8, coupling="vector"):
    """Not in the reference's lib/utils.py (its README advises to add local contrast after the deconvolution "through wavelets
    high-pass filter and a laplacian filter"; `wavelet_equalizer` is the first, this the second): the fast local Laplacian filter.
    Differences below sigma (pixel values in [0, 1]) are multiplied by `detail`, differences well above it by `edges`, at every scale
    of a Laplacian pyramid of `levels` halvings (None: down to 16 px) and without halos: sigma=0.2, detail=1.8, edges=1 adds clarity
    at tens to hundreds of pixels, sigma=0.2, detail=1, edges=0.6 compresses the tonal range and keeps the detail.  `samples`
    (2 .. 16) remapped copies are interpolated; 8 is within 1e-2 of the exact filter.  coupling "vector" filters the luma and adds
    its change to the three channels (no hue shift), "channel" every channel by itself.  A `lib._native.DeviceImage` gives a new
    DeviceImage (nothing crosses PCIe); an H x W x 3 array is uploaded once and the float32 result downloaded once
    (`DeviceImage.local_laplacian`, csrc/ics_img_llf.hip)."""
    if isinstance(src, _native.DeviceImage):
        return src.local_laplacian(sigma, detail, edges, levels, samples, coupling)
    arr = np.asarray(src)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("expected a DeviceImage or an H x W x 3 array, got shape %s" % (arr.shape,))
    _native.llf_args(sigma, detail, edges, levels, samples, coupling)    # refused before anything is uploaded
    img = _native.DeviceImage.from_host(np.ascontiguousarray(arr, dtype=np.float32))
    try:
        res = img.local_laplacian(sigma, detail, edges, levels, samples, coupling)
    finally:
        img.close()
    try:
        return res.to_host()
    finally:
        res.close()


def bessel_blur(src, radius, amount):
    """lib/utils.py:237-249: convolve2d(src, kaiser_kernel(radius, amount), mode="same", boundary="symm")"""
    if isinstance(src, _native.DeviceImage):
        return src.bessel_blur(radius, amount)
    return _native.Context.get().conv2d_symm(_as2d(src), kaiser_kernel(radius, amount))


def gaussian_blur(src, radius, amount):
    """lib/utils.py:252-264: convolve2d(src, gaussian_kernel(radius, amount), mode="same", boundary="symm")"""
    if isinstance(src, _native.DeviceImage):
        return src.gaussian_blur(radius, amount)
    return _native.Context.get().conv2d_symm(_as2d(src), gaussian_kernel(radius, amount))


def USM(src, radius, strength, amount, method="bessel"):
    """lib/utils.py:267-277: src + (src - blur(src, radius, strength)) * amount, fused on the device."""
    if isinstance(src, _native.DeviceImage):
        return src.usm(radius, strength, amount, method)
    kern = {"bessel": kaiser_kernel, "gauss": gaussian_kernel}[method](radius, strength)
    return _native.Context.get().usm(_as2d(src), kern, float(amount))


# ---- I/O ------------------------------------------------------------------------------------------
def _write_tiff_rgb16(path, arr):
    """Minimal baseline TIFF writer: uncompressed, little-endian, 16 bits x 3 samples, chunky RGB.
    (The reference vendors tifffile for this, lib/utils.py:312; one strip is all `save` needs.)"""
    h, w, c = arr.shape
    assert c == 3 and arr.dtype == np.uint16
    data = np.ascontiguousarray(arr).astype("<u2").tobytes()
    n_entries = 10
    ifd_off = 8
    bps_off = ifd_off + 2 + n_entries * 12 + 4
    data_off = bps_off + 6
    def ent(tag, typ, count, value):
        return struct.pack("<HHII", tag, typ, count, value)
    ifd = struct.pack("<H", n_entries)
    ifd += ent(256, 4, 1, w) + ent(257, 4, 1, h) + ent(258, 3, 3, bps_off) + ent(259, 3, 1, 1)
    ifd += ent(262, 3, 1, 2) + ent(273, 4, 1, data_off) + ent(277, 3, 1, 3) + ent(278, 4, 1, h)
    ifd += ent(279, 4, 1, len(data)) + ent(284, 3, 1, 1)
    ifd += struct.pack("<I", 0)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd_off))
        f.write(ifd)
        f.write(struct.pack("<HHH", 16, 16, 16))
        f.write(data)


def save(pic, name, dest_path):
    """lib/utils.py:303-312: 16-bit RGB TIFF `<dest_path>/<name>.tif`."""
    _write_tiff_rgb16(join(dest_path, name + ".tif"), np.asarray(pic).astype(np.uint16))


def convolve(a, b, domain):
    """lib/utils.py:420-447 (pyFFTW in the reference, unused by it): FFT convolution of two 2-D arrays,
    `domain` in {"same", "valid", "full"}; output = the first (Y, X) samples of the full result like the
    reference's irfft2(c_temp, (Y, X))."""
    MK, NK = b.shape[0], b.shape[1]
    M, N = a.shape[0], a.shape[1]
    if domain == "same":
        Y, X = M, N
    elif domain == "valid":
        Y, X = M - MK + 1, N - NK + 1
    elif domain == "full":
        Y, X = M + MK - 1, N + NK - 1
    else:
        raise SyntaxError
    s = (M + MK - 1, N + NK - 1)
    c_temp = np.fft.rfft2(a, s=s) * np.fft.rfft2(b, s=s)
    return np.fft.irfft2(c_temp, (Y, X))
