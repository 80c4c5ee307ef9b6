# -*- coding: utf-8 -*-
"""Driver with the call surface of the reference's `deconvolve.py` (pad_image :24-37, build_pyramid
:40-60, deblur_module :65-368), feeding the GPU solver in `lib.deconvolution`.

What is kept from the reference: argument names/defaults of `deblur_module`, the validation errors
(:117-120, :145-148), gamma and bit-depth scaling (:97-103, :346-352), odd-size padding (:164-175), the
pyramid schedule, the mask-window arithmetic (:209-230) and the three call shapes into
`richardson_lucy_MM` (:277-313) including their positional arguments.

What differs, and why:
  * `skimage.transform.resize(order=3, mode="edge")` (:245-249) is an un-vendored dependency that is
    not installed in this image; `resize_bicubic` below runs its documented algorithm (Gaussian anti-aliasing
    when shrinking + cubic B-spline interpolation) on the GPU (csrc/ics_resize.hip), checked against
    scipy.ndimage in oracle/resize_oracle.py.  PARITY with skimage itself is UNPINNED for the pyramid levels
    below 1.0; with `pyramid=False` (one level, scale 1) no resize is involved.
  * matplotlib pop-ups (:331-336) only when `display=True` and matplotlib is importable.
  * the 16-bit TIFF is written by `lib.utils.save` (own minimal writer instead of the vendored tifffile).
"""
import numpy as np

from lib import utils
from lib import deconvolution as dc


def pad_image(image, pad, mode="edge"):
    """deconvolve.py:24-37 -- grow the two spatial axes of an H x W x 3 picture; `pad` is whatever numpy.pad takes for a 2-D array
    (a width, a (before, after) pair for both axes, or one pair per axis); the channel axis is never padded.  float32, C-contiguous."""
    widths = np.broadcast_to(np.asarray(pad, dtype=int), (2, 2))
    grown = np.pad(np.asarray(image), (tuple(widths[0]), tuple(widths[1]), (0, 0)), mode=mode)
    return np.ascontiguousarray(grown, dtype=np.float32)


def build_pyramid(psf_size, lambd):
    """deconvolve.py:40-60 -- the coarse-to-fine schedule: every level shrinks the picture by sqrt(2) and the PSF with it, the PSF size
    rounded up and then made odd (never below 3); the last level is the first whose PSF is 3 x 3.  Returns (scales, sizes), finest first.
    (`lambd` is accepted and unused, as in the reference.)"""
    root2 = np.sqrt(2)
    scales, sizes = [1.], [psf_size]
    while sizes[-1] > 3:
        k = int(np.ceil(sizes[-1] / root2))
        k -= 1 - k % 2                      # even -> the odd size below
        sizes.append(max(k, 3))
        scales.append(scales[-1] / root2)
    return scales, sizes


def resize_bicubic(img, shape):
    """skimage.transform.resize(img, shape, order=3, mode="edge", preserve_range=True) (deconvolve.py:245-249) on the GPU:
    Gaussian anti-aliasing when shrinking + cubic B-spline interpolation, `ics_resize_bicubic` (csrc/ics_resize.hip)."""
    img = np.asarray(img, dtype=np.float64)
    if img.shape[:2] == (int(shape[0]), int(shape[1])):   # scale 1: the interpolating spline reproduces the samples
        return img.copy()
    from lib import _native
    return _native.Context.get().resize_bicubic(img, shape)


def mask_window(i, top, bottom, left, right):
    """deconvolve.py:209-230 -- scale the mask box to pyramid level `i` and make it odd and square,
    with the reference's exact (and slightly odd) tie-breaking."""
    temp_top, temp_bottom = int(i * top), int(i * bottom)
    temp_left, temp_right = int(i * left), int(i * right)
    if int(temp_bottom - temp_top) % 2 == 0:
        if int(temp_bottom - temp_top) < int(temp_right - temp_left):
            temp_bottom += 1
        elif int(temp_bottom - temp_top) > int(temp_right - temp_left):
            temp_top += 1
        else:
            temp_top -= 1
    if int(temp_right - temp_left) % 2 == 0:
        if int(temp_bottom - temp_top) < int(temp_right - temp_left):
            temp_left += 1
        elif int(temp_bottom - temp_top) > int(temp_bottom - temp_top):   # (sic) never true, deconvolve.py:227
            temp_right += 1
        else:
            temp_right -= -1                                              # (sic) deconvolve.py:230
    return temp_top, temp_bottom, temp_left, temp_right


@utils.timeit
def deblur_module(pic, filename, dest_path, blur_width, confidence=10, tolerance=1, quality="normal", bits=8,
                  mask=None, display=True, blur="static", preview=False, p=1, order=2, norm=1, priority=0, mask_size=255,
                  iterations=200, refocus=False, pyramid=True, solver=None, save=True, device_resident=None, sharpen=None, denoise=None,
                  local_contrast=None, detail=None, clarity=None, despeckle=None, nonblind="rl", blind="rl"):
    """deconvolve.py:65-368.  Extra keyword arguments (not in the reference): `pyramid=False` runs the
    single scale-1 level only, `solver` replaces `dc.richardson_lucy_MM` (tests record the calls),
    `save=False` returns the float image instead of writing the TIFF, `device_resident=True` keeps every frame in HBM
    from the first upload to the final download (`_deblur_device`; same arithmetic, same calls into the solver; the two
    paths differ by float32 `powf` of the gamma steps, numpy vs device: <= 2e-5 of the 16-bit range, tests/test_driver.py).
    Default (None): resident unless a `solver` is given or `display` asks for the matplotlib pop-up of the host frames --
    2048^2, 15-px blur, 20 iterations: 0.085 s resident, 0.6-0.9 s with the frames on the host between the solver calls.
    `sharpen=(radius, strength, amount)` or `(radius, strength, amount, method)`: `utils.USM` with these arguments on the
    deblurred frame, in the gamma-encoded domain, immediately before the final clip to [0, 1] (the local contrast the
    reference's README advises to add afterwards); on the resident path the frame is sharpened in HBM.
    `denoise=(weight, iterations)` or `(weight, iterations, coupling)`: `utils.tv_denoise` with these arguments (coupling
    "vector" unless given) on the deblurred frame, in the gamma-encoded domain, before `sharpen` and before the final clip:
    Richardson-Lucy amplifies noise, and the total-variation denoiser removes it without blunting the restored edges; on the
    resident path the frame stays in HBM.
    `local_contrast=(gains,)`, `(gains, thresholds)` or `(gains, thresholds, coupling)`: `utils.wavelet_equalizer` with these
    arguments (residual 1, coupling "vector" unless given) on the deblurred frame, in the gamma-encoded domain, after `denoise`,
    before `sharpen` and before the final clip: the scale-by-scale form of the README's advice -- the 4 to 16 px detail that
    Richardson-Lucy leaves flat is lifted by the gains of scales 2 to 4 while the 1 px noise it amplified keeps gain 1 or is
    thresholded away; on the resident path the frame stays in HBM.  thresholds "auto" or ("auto", strength): the noise the
    deconvolution left in this frame is estimated where the frame lies (`utils.noise_estimate`, same coupling; only its few result
    floats come back) and every scale is thresholded at `strength` (3 unless given) standard deviations of it.
    `detail=(radius, eps, gain)` or `(radius, eps, gain, coupling)`: `utils.guided_filter` with these arguments (coupling
    "vector" unless given) on the deblurred frame, in the gamma-encoded domain, after `local_contrast`, before `sharpen` and before
    the final clip: the frame's guided-filter base layer plus `gain` times its detail -- a gain above 1 sharpens at radii of 8 to
    32 px without the halos a Gaussian mask of that size puts around the edges Richardson-Lucy has just restored, a gain below 1
    smooths texture and keeps them; on the resident path the frame stays in HBM.
    `clarity=(sigma, detail)`, `(sigma, detail, edges)` or `(sigma, detail, edges, coupling)`: `utils.local_laplacian` with these
    arguments (edges 1, coupling "vector" unless given; default levels, 8 samples) on the deblurred frame, in the gamma-encoded
    domain, after `denoise` and before `local_contrast`: the steps run coarse to fine -- tone and clarity at tens to hundreds of
    pixels, then the scale gains, then the guided detail, then the mask, then the clip.  (0.2, 1.8) adds clarity, (0.2, 1, 0.6)
    compresses the tonal range and keeps the detail; on the resident path the frame stays in HBM.
    `despeckle=(threshold,)`, `(threshold, radius)` or `(threshold, radius, coupling)`: `utils.despeckle` with these arguments (radius
    1, coupling "vector" unless given; threshold a value, three for "channel", "auto" or ("auto", strength)) on the INPUT picture, in
    the gamma-encoded domain, before the odd-size padding and before either deconvolution phase: a hot or dead pixel, which
    Richardson-Lucy would turn into a PSF-sized ring at every pyramid level, or a NaN, which would spread over the frame, is
    replaced by the median of its window and nothing else is touched; one line "Despeckle : <counts> replaced" is printed.
    `despeckle=("auto",)` takes six sigma of the picture's own noise.  On the resident path the frame stays in HBM.
    `blur_width="auto"` or `("auto", max_width)` (max_width 63 unless given, odd): the width is read from the picture
    (`utils.estimate_blur_width`: the autocorrelation of the derivatives, the reference's "TODO : automatically evaluate blur size"),
    on the gamma-encoded frame the solver will see, after `despeckle` and before the odd-size padding, over the mask box where `mask`
    is given and over the whole frame otherwise; one line "Blur width : 9 (x 8.41, y 7.63)" is printed and everything runs as if
    that integer had been passed.  On the resident path the frame is read where it lies and only the profiles come back.
    `mask="auto"` or `("auto", clip)` (clip 0.99 unless given): the centre of the PSF-estimation box is chosen from the picture
    (`utils.best_mask`: the box whose structure tensor of luma differences has the largest smaller eigenvalue -- edges in every
    orientation -- pixels with a channel at or above `clip` left out), on the gamma-encoded frame the solver will see, after
    `despeckle`, before the automatic blur width (which is then read over the chosen box) and before the odd-size padding, among the
    boxes that lie inside the picture; one line "Mask : [95, 143] (score 2.93e-03, clipped 0.0 %)" is printed before "Mask size :" and
    everything runs as if that centre had been passed.  On the resident path the frame is read where it lies.
    `mask=("auto", clip, (lo, hi))`: the same choice among the boxes whose local blur width (`utils.blur_map`, a Gaussian-equivalent
    sigma in pixels) lies in [lo, hi] -- the subject under a defocus that varies over the frame, where the plain choice takes the zone
    in focus; the line reads "Mask : [95, 143] (score 2.93e-03, clipped 0.0 %, blur 2.31)", ValueError where no box qualifies.
    `nonblind="rl"` (the default: the reference's second phase, the loop on the whole frame), `"wiener"` or `("wiener", balance)`
    (balance 0.01 unless given): the blind phase runs as ever, and the second phase is one `utils.wiener` of the full-resolution
    gamma-encoded frame with the PSF the blind phase returned -- milliseconds where the loop takes most of the run, to try a PSF on
    the whole picture; "===== WIENER DECONVOLUTION =====" and one line "Wiener : balance 0.01, 8192 × 8192 transform" are printed,
    and `denoise`, `clarity`, ... and the clip follow as after the loop.  On the resident path the frame stays in HBM.
    `nonblind="tv"`, `("tv", fidelity)`, `("tv", fidelity, iterations)` or `("tv", fidelity, iterations, coupling)` (fidelity 2000, 10
    iterations, coupling "vector" unless given; the penalty is 10): likewise, the second phase being one `utils.tv_deconvolve` -- the
    loop's total-variation prior on `wiener`'s transform, tens of milliseconds, lower fidelity for noisier frames;
    "===== TV DECONVOLUTION =====" and one line "TV : fidelity 2000, penalty 10, 10 iterations, vector, 8192 × 8192 transform" are
    printed.
    `nonblind="tv-masked"` or `("tv-masked", fidelity[, iterations[, coupling[, clip]]])` (fidelity 2000, 10 iterations, coupling
    "vector", clip 0.99 unless given; the penalties are 10 and the fidelity): likewise, the second phase being one
    `utils.tv_deconvolve_masked` -- "tv" with the pixels beyond the frame's edges and those with a channel at or above `clip` (None:
    none) unobserved instead of fitted; the edges pay at once, the clipped highlights only from about 30 iterations;
    "===== MASKED TV DECONVOLUTION =====" and one line "TV-masked : fidelity 2000, penalties 10 / 2000, 10 iterations, vector, clip
    0.99, 8192 × 8192 transform, 1.72 % unobserved" are printed.
    `blind="rl"` (the default: the reference's first phase, the blind loop through the pyramid; the call as it always was), `"fast"` or
    `("fast", iterations)` (5 per level unless given): the first phase is `utils.blind_psf` on the mask box of the gamma-encoded frame
    (after `despeckle=`, `mask="auto"`, `blur_width="auto"` and the odd-size padding) with size = blur_width -- edge prediction and a
    masked pair solve in turns, milliseconds where the loop takes tens --; "===== FAST BLIND PSF =====" and one line per level,
    "Level : PSF 15, frame 255 × 255, 14048 gradients kept, 3.1 % of the raw kernel cut", are printed, `last_phase_seconds["blind"]` is
    filled, and the PSF enters the second phase where the loop's does, for every `nonblind=`.  It serves compact PSFs, not thin motion
    lines: `blur="motion"` with it is refused."""
    fast_phase = _nonblind_args(nonblind)
    fast_blind = _blind_args(blind, blur)
    despeckle = _despeckle_args(despeckle)
    auto_width = _blur_width_args(blur_width)
    auto_mask = _mask_args(mask)
    sharpen = _sharpen_args(sharpen)
    denoise = _denoise_args(denoise)
    local_contrast = _local_contrast_args(local_contrast)
    detail = _detail_args(detail)
    clarity = _clarity_args(clarity)
    if device_resident is None:
        device_resident = solver is None and not display
    if device_resident:
        if solver is not None:
            raise ValueError("device_resident=True runs the GPU solver; `solver` cannot be replaced")
        return _deblur_device(pic, filename, dest_path, blur_width, confidence, tolerance, quality, bits, mask, display, blur, preview, p,
                              order, norm, priority, mask_size, iterations, refocus, pyramid, save, despeckle, sharpen, denoise, local_contrast, detail, clarity,
                              *(() if fast_phase is None and fast_blind is None else (fast_phase, fast_blind)))   # (nonblind="rl", blind="rl": the call as it always was)
    rl = solver if solver is not None else dc.richardson_lucy_MM
    pic = np.ascontiguousarray(pic, dtype=np.float32)
    pic = pad_image(pic, (1, 1)).astype(np.float32)                       # :94
    samples = 2 ** bits - 1                                               # :97
    pic = pic / samples
    pic = pic ** (1 / 2.2)                                                # :103
    if despeckle is not None:
        pic, replaced = utils.despeckle(np.ascontiguousarray(pic, dtype=np.float32), *despeckle, count=True)
        print("Despeckle :", ", ".join(str(n) for n in replaced), "replaced")
    step = {"normal": 1e-3, "high": 5e-4, "veryhigh": 1e-4, "low": 5e-3}[quality]   # :106-113
    if auto_width is None:
        if blur_width < 3:
            raise ValueError("The blur width should be at least 3 pixels.")
        elif blur_width % 2 == 0:
            raise ValueError("The blur width should be odd. You can use %i." % (blur_width + 1))
    M, N = pic.shape[0], pic.shape[1]
    if auto_mask is not None:
        mask = _auto_mask(pic, mask_size, auto_mask)
    whole_frame = mask is None
    if mask is None:
        mask = [M // 2, N // 2]
    top, bottom = mask[0] - mask_size // 2, mask[0] + mask_size // 2       # :138-141
    left, right = mask[1] - mask_size // 2, mask[1] + mask_size // 2
    print("Mask size :", (bottom - top + 1), "×", (right - left + 1))
    if not (top > 0 and bottom < M and left > 0 and right < N):
        raise ValueError("The mask is outside the picture boundaries. Move its center inside or reduce the blur size.")
    if auto_width is not None:
        blur_width = _auto_blur_width(pic, auto_width, None if whole_frame else (top, bottom + 1, left, right + 1))
    correlation = {"static": False, "motion": True}[blur]                 # :154-157
    tolerance /= 100.
    odd_vert = odd_hor = False
    if pic.shape[0] % 2 == 0:                                             # :167-175
        pic = pad_image(pic, ((1, 0), (0, 0))).astype(np.float32)
        odd_vert = True
        print("Padded vertically")
    if pic.shape[1] % 2 == 0:
        pic = pad_image(pic, ((0, 0), (1, 0))).astype(np.float32)
        odd_hor = True
        print("Padded horizontally")
    M, N = pic.shape[0], pic.shape[1]
    psf = utils.uniform_kernel(blur_width)                                # :178-179
    psf = np.dstack((psf, psf, psf))
    images, kernels = build_pyramid(blur_width, confidence)               # :182
    if not pyramid:
        images, kernels = images[:1], kernels[:1]
    deblured_image = pic
    try:
        for case in ["blind", "non-blind"]:                               # :193
            if case == "non-blind" and fast_phase is not None:
                deblured_image = _fast_phase(pic, psf, fast_phase)
                break
            if case == "blind" and fast_blind is not None:
                psf = _fast_blind(pic, (top, bottom + 1, left, right + 1), blur_width, fast_blind)
                continue
            print("\n===== %s DECONVOLUTION =====" % case)
            deblured_image = pic.copy()
            lambd = confidence * 1000                                     # :200
            for i, k in zip(reversed(images), reversed(kernels)):        # :204
                print("======== Pyramid step %1.3f ========" % i)
                temp_top, temp_bottom, temp_left, temp_right = mask_window(i, top, bottom, left, right)
                temp_width, temp_height = int(np.floor(i * N)), int(np.floor(i * M))
                if temp_width % 2 == 0:
                    temp_width += 1
                if temp_height % 2 == 0:
                    temp_height += 1
                shape = (temp_height, temp_width, 3)
                temp_blurry_image = resize_bicubic(pic, shape).astype(np.float32)              # :245
                deblured_image = resize_bicubic(deblured_image, shape).astype(np.float32)      # :246
                if case == "blind":
                    psf_copy = np.ascontiguousarray(resize_bicubic(psf, (k, k, 3)).astype(np.float32))   # :249
                    dc.normalize_kernel(psf_copy, k)
                else:
                    psf_copy = np.ascontiguousarray(psf, dtype=np.float32).copy()
                    k = kernels[0]
                temp_blurry_image = pad_image(temp_blurry_image, (1, 1)).astype(np.float32)    # :256-257
                deblured_image = pad_image(deblured_image, (1, 1)).astype(np.float32)
                pad = int(np.floor(k / 2))
                print("Image size", temp_blurry_image.shape)
                print("u size", deblured_image.shape)
                print("Mask size", (temp_bottom - temp_top), (temp_right - temp_left))
                print("PSF size", psf_copy.shape)
                tolerance_temp = tolerance if i == 1. else 0
                win = (pad + 1, temp_bottom - temp_top - pad - 1, pad + 1, temp_bottom - temp_top - pad - 1)
                if case == "blind":                                       # :277-288
                    deblured_image[temp_top - 1:temp_bottom + 1, temp_left - 1:temp_right + 1, ...] = rl(
                        temp_blurry_image[temp_top - 1:temp_bottom + 1, temp_left - 1:temp_right + 1, ...],
                        deblured_image[temp_top - pad - 1:temp_bottom + pad + 1, temp_left - pad - 1:temp_right + pad + 1, ...],
                        psf_copy, *win, 0, temp_bottom - temp_top + 2, temp_right - temp_left + 2, 3,
                        k, iterations, step, lambd, blind=True, p=p, correlation=correlation, order=order, norm=2,
                        priority=0, refocus=refocus)
                    psf = psf_copy.copy()
                elif preview:                                             # :290-300
                    deblured_image[temp_top - 1:temp_bottom + 1, temp_left - 1:temp_right + 1, ...] = rl(
                        temp_blurry_image[temp_top - 1:temp_bottom + 1, temp_left - 1:temp_right + 1, ...],
                        deblured_image[temp_top - pad - 1:temp_bottom + pad + 1, temp_left - pad - 1:temp_right + pad + 1, ...],
                        psf_copy, *win, tolerance_temp, temp_bottom - temp_top + 2, temp_right - temp_left + 2, 3,
                        k, iterations, step, lambd, blind=False, p=p, order=order, norm=2, priority=priority, refocus=refocus)
                else:                                                     # :301-316
                    deblured_image = pad_image(deblured_image, (pad, pad)).astype(np.float32)
                    deblured_image[pad:-pad, pad:-pad, ...] = rl(
                        temp_blurry_image, deblured_image, psf_copy, *win, tolerance_temp,
                        temp_height + 2, temp_width + 2, 3,
                        k, iterations, step, lambd, blind=False, p=p, order=order, norm=2, priority=priority, refocus=refocus)
                    deblured_image = deblured_image[pad:-pad, pad:-pad, ...]
                temp_blurry_image = temp_blurry_image[1:-1, 1:-1, ...]    # :322-323
                deblured_image = deblured_image[1:-1, 1:-1, ...]
            if display and case == "blind":                               # :331-336
                try:
                    import matplotlib.pyplot as plt
                    psf_check = (psf - np.amin(psf)) / (np.amax(psf) - np.amin(psf))
                    plt.imshow(psf_check, interpolation="lanczos", aspect="equal", vmin=0, vmax=1)
                    plt.show()
                except ImportError:
                    pass
    except KeyboardInterrupt:                                             # :338-342
        pass
    if denoise is not None:
        deblured_image = utils.tv_denoise(np.ascontiguousarray(deblured_image, dtype=np.float32), *denoise)
    if clarity is not None:
        sigma, gain, edges, coupling = clarity
        deblured_image = utils.local_laplacian(np.ascontiguousarray(deblured_image, dtype=np.float32), sigma, gain, edges, None, 8, coupling)
    if local_contrast is not None:
        gains, thresholds, coupling = local_contrast
        deblured_image = utils.wavelet_equalizer(np.ascontiguousarray(deblured_image, dtype=np.float32), gains, thresholds, 1.0, coupling)
    if detail is not None:
        deblured_image = utils.guided_filter(np.ascontiguousarray(deblured_image, dtype=np.float32), *detail)
    if sharpen is not None:                                               # per channel, as a user of lib.utils would
        deblured_image = np.dstack([utils.USM(deblured_image[..., c], *sharpen) for c in range(3)]).astype(np.float32)
    deblured_image = np.clip(deblured_image, 0., 1.)                      # :346
    deblured_image = deblured_image ** 2.2
    deblured_image = deblured_image * (2 ** 16 - 1)
    if preview:
        filename = filename + "-preview"
        deblured_image = deblured_image[top:bottom, left:right, ...]
    else:
        if odd_hor:
            deblured_image = deblured_image[:, 1:, ...]
        if odd_vert:
            deblured_image = deblured_image[1:, :, ...]
        deblured_image = deblured_image[1:-1, 1:-1, ...]
    if save:
        utils.save(deblured_image, filename, dest_path)
    return deblured_image, psf


def _blind_args(blind, blur):
    """`blind` of deblur_module -> None for "rl" (the loop), the iterations per level of "fast" / ("fast", iterations), checked
    (ValueError)"""
    form = "blind takes \"rl\", \"fast\" or (\"fast\", iterations), got %r" % (blind,)
    if isinstance(blind, str):
        if blind not in ("rl", "fast"):
            raise ValueError(form)
        n = None if blind == "rl" else 5
    elif isinstance(blind, (tuple, list)) and len(blind) == 2 and blind[0] == "fast":
        n = blind[1]
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("blind: iterations %r (a whole number, 1 or more)" % (n,))
        n = int(n)
    else:
        raise ValueError(form)
    if n is not None and blur == "motion":
        raise ValueError("blind=\"fast\" does not serve blur=\"motion\": the edge prediction does not recover thin motion lines (use blind=\"rl\")")
    return n


def _fast_blind(frame, window, blur_width, iterations):
    """the blind phase of deblur_module(blind="fast") on the mask box of the gamma-encoded frame (an array or a DeviceImage): its
    printed lines, the PSF"""
    print("\n===== FAST BLIND PSF =====")
    got = utils.blind_psf(frame, blur_width, iterations, window=window, info=True)
    for (k, h, w), kept, rejected in zip(got.levels, got.kept, got.rejected):
        print("Level : PSF %d, frame %d × %d, %d gradients kept, %.1f %% of the raw kernel cut" % (k, h, w, kept, 100.0 * max(rejected)))
    return got.psf


def _nonblind_args(nonblind):
    """`nonblind` of deblur_module -> None for "rl" (the loop), the balance of "wiener" / ("wiener", balance),
    ("tv", fidelity, iterations, coupling) of "tv" / ("tv", fidelity[, iterations[, coupling]]), or
    ("tv-masked", fidelity, iterations, coupling, clip) of "tv-masked" / ("tv-masked", fidelity[, iterations[, coupling[, clip]]]),
    checked (ValueError)"""
    form = ("nonblind takes \"rl\", \"wiener\", (\"wiener\", balance), \"tv\", (\"tv\", fidelity[, iterations[, coupling]]), "
            "\"tv-masked\" or (\"tv-masked\", fidelity[, iterations[, coupling[, clip]]]), got %r" % (nonblind,))
    if isinstance(nonblind, str):
        if nonblind not in ("rl", "wiener", "tv", "tv-masked"):
            raise ValueError(form)
        return {"rl": None, "wiener": 0.01, "tv": ("tv",) + _TV_PHASE, "tv-masked": ("tv-masked",) + _TVM_PHASE}[nonblind]
    if not isinstance(nonblind, (tuple, list)) or len(nonblind) < 2 or not isinstance(nonblind[0], str):
        raise ValueError(form)
    from lib import _native
    if nonblind[0] == "tv-masked" and len(nonblind) <= 5:
        fidelity, iterations, coupling, clip = tuple(nonblind[1:]) + _TVM_PHASE[len(nonblind) - 1:]
        try:                                      # (the PSF is the blind phase's: a stand-in passes its checks here)
            _, _, clip, fidelity, _, _, iterations, coupling = _native.tv_deconvolve_masked_args(np.ones((3, 3)), None, clip, fidelity, _TV_PENALTY, None, iterations,
                                                                                                 coupling, (3, 3))
        except ValueError as exc:
            raise ValueError("nonblind: %s" % exc)
        return ("tv-masked", fidelity, iterations, coupling, clip)
    if nonblind[0] == "tv" and len(nonblind) <= 4:
        fidelity, iterations, coupling = tuple(nonblind[1:]) + _TV_PHASE[len(nonblind) - 1:]
        try:                                      # (the PSF is the blind phase's: a stand-in passes its checks here)
            _, fidelity, _, iterations, coupling = _native.tv_deconvolve_args(np.ones((3, 3)), fidelity, _TV_PENALTY, iterations, coupling, (3, 3))
        except ValueError as exc:
            raise ValueError("nonblind: %s" % exc)
        return ("tv", fidelity, iterations, coupling)
    if len(nonblind) != 2 or nonblind[0] != "wiener":
        raise ValueError(form)
    if not _native._finite32(nonblind[1], scalar=True) or not np.float32(nonblind[1]) > 0:
        raise ValueError("nonblind: balance %r (must be finite and > 0)" % (nonblind[1],))
    return float(nonblind[1])


_TV_PHASE = (2000.0, 10, "vector")      # fidelity, iterations, coupling of nonblind="tv" where not given
_TV_PENALTY = 10.0
_TVM_PHASE = _TV_PHASE + (0.99,)        # ... and clip of nonblind="tv-masked"


def _fast_phase(frame, psf, choice):
    """the second phase of deblur_module where `nonblind` is not the loop (`choice`: what _nonblind_args returned)"""
    if isinstance(choice, tuple):
        return (_tvm_phase if choice[0] == "tv-masked" else _tv_phase)(frame, psf, *choice[1:])
    return _wiener_phase(frame, psf, choice)


def _tvm_phase(frame, psf, fidelity, iterations, coupling, clip):
    """the second phase of deblur_module(nonblind="tv-masked") on the full-resolution gamma-encoded frame (an array or a DeviceImage):
    its two printed lines (the second once the count is back), the deconvolved frame"""
    from lib import _native
    print("\n===== MASKED TV DECONVOLUTION =====")
    plan = _native.tv_deconvolve_masked_plan(frame.shape[0], frame.shape[1], np.shape(psf)[0])
    out, unobserved = utils.tv_deconvolve_masked(frame, psf, None, clip, fidelity, _TV_PENALTY, None, iterations, coupling, count=True)
    print("TV-masked : fidelity %g, penalties %g / %g, %d iterations, %s, clip %s, %d × %d transform, %.2f %% unobserved"
          % (fidelity, _TV_PENALTY, fidelity, iterations, coupling, "none" if clip == float("inf") else "%g" % clip, plan.Py, plan.Px,
             100.0 * unobserved / (frame.shape[0] * frame.shape[1])))
    return out


def _tv_phase(frame, psf, fidelity, iterations, coupling):
    """the second phase of deblur_module(nonblind="tv") on the full-resolution gamma-encoded frame (an array or a DeviceImage): its
    two printed lines, the deconvolved frame"""
    from lib import _native
    print("\n===== TV DECONVOLUTION =====")
    plan = _native.tv_deconvolve_plan(frame.shape[0], frame.shape[1], np.shape(psf)[0])
    print("TV : fidelity %g, penalty %g, %d iterations, %s, %d × %d transform" % (fidelity, _TV_PENALTY, iterations, coupling, plan.Py, plan.Px))
    return utils.tv_deconvolve(frame, psf, fidelity, _TV_PENALTY, iterations, coupling)


def _wiener_phase(frame, psf, balance):
    """the second phase of deblur_module(nonblind="wiener") on the full-resolution gamma-encoded frame (an array or a DeviceImage):
    its two printed lines, the filtered frame"""
    from lib import _native
    print("\n===== WIENER DECONVOLUTION =====")
    plan = _native.wiener_plan(frame.shape[0], frame.shape[1], np.shape(psf)[0])
    print("Wiener : balance %g, %d × %d transform" % (balance, plan.Py, plan.Px))
    return utils.wiener(frame, psf, balance)


def _sharpen_args(sharpen):
    """`sharpen` of deblur_module -> None or (radius, strength, amount, method)"""
    if sharpen is None:
        return None
    sharpen = tuple(sharpen)
    if len(sharpen) == 3:
        sharpen += ("bessel",)
    if len(sharpen) != 4:
        raise ValueError("sharpen takes (radius, strength, amount) or (radius, strength, amount, method), got %d values" % len(sharpen))
    if sharpen[3] not in ("bessel", "gauss"):
        raise ValueError("sharpen method %r (bessel or gauss)" % (sharpen[3],))
    return sharpen


def _denoise_args(denoise):
    """`denoise` of deblur_module -> None or (weight, iterations, coupling)"""
    if denoise is None:
        return None
    denoise = tuple(denoise)
    if len(denoise) == 2:
        denoise += ("vector",)
    if len(denoise) != 3:
        raise ValueError("denoise takes (weight, iterations) or (weight, iterations, coupling), got %d values" % len(denoise))
    weight, iterations, coupling = denoise
    from lib._native import _coupling
    _coupling(coupling, "denoise coupling")
    if not (np.isfinite(weight) and weight > 0):
        raise ValueError("denoise weight %r (must be positive and finite)" % (weight,))
    if int(iterations) != iterations or iterations < 0:
        raise ValueError("denoise iterations %r (a non-negative integer)" % (iterations,))
    return float(weight), int(iterations), coupling


def _blur_width_args(blur_width):
    """`blur_width` of deblur_module -> None for a number (the reference's two checks apply to it) or the max_width of "auto" /
    ("auto", max_width), checked (ValueError)"""
    if isinstance(blur_width, str):
        if blur_width != "auto":
            raise ValueError("blur_width takes an odd integer, \"auto\" or (\"auto\", max_width), got %r" % (blur_width,))
        return utils.blur_width_args()
    if isinstance(blur_width, (tuple, list)):
        if len(blur_width) != 2 or blur_width[0] != "auto":
            raise ValueError("blur_width takes an odd integer, \"auto\" or (\"auto\", max_width), got %r" % (blur_width,))
        try:
            return utils.blur_width_args(blur_width[1])
        except ValueError as exc:
            raise ValueError("blur_width: %s" % exc)
    return None


def _auto_blur_width(frame, max_width, window):
    """the estimate on the frame (an array or a DeviceImage), its one printed line, the width"""
    est = utils.estimate_blur_width(frame, max_width, window)
    print("Blur width : %d (x %.2f, y %.2f)" % est)
    return est.width


def _mask_args(mask):
    """`mask` of deblur_module -> None for None or a centre [y, x] of two integers, the clip level of "auto" / ("auto", clip),
    (clip, (lo, hi)) of ("auto", clip, (lo, hi)), checked (ValueError)"""
    from lib import _native
    form = "mask takes None, a centre [y, x] of two integers, \"auto\", (\"auto\", clip) or (\"auto\", clip, (lo, hi)), got %r" % (mask,)
    if mask is None:
        return None
    if isinstance(mask, str):
        if mask != "auto":
            raise ValueError(form)
        return 0.99
    if not isinstance(mask, (list, tuple, np.ndarray)):
        raise ValueError(form)
    pair = len(mask) == 2
    if len(mask) in (2, 3) and isinstance(mask[0], str):
        if mask[0] != "auto":
            raise ValueError(form)
        try:
            clip = _native.window_scores_args(_native.IMG_MASK_CELL, None, mask[1], (_native.IMG_MASK_CELL, _native.IMG_MASK_CELL))[2]
            return clip if pair else (clip, utils.mask_blur_args(mask[2]))
        except ValueError as exc:
            raise ValueError("mask: %s" % exc)
    if not pair or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in mask):
        raise ValueError(form)
    return None


def _auto_mask(frame, mask_size, clip):
    """the choice on the 1-px-padded frame (an array or a DeviceImage) among the boxes the reference's boundary test accepts, its one
    printed line, the centre"""
    M, N = frame.shape[0], frame.shape[1]
    if 2 * (mask_size // 2) + 1 > min(M, N) - 2:
        raise ValueError("The mask is outside the picture boundaries. Move its center inside or reduce the blur size.")
    if isinstance(clip, tuple):                                             # ("auto", clip, (lo, hi)): the best box whose blur lies in the range
        got = utils.best_mask(frame, mask_size, clip[0], (1, M - 1, 1, N - 1), blur=clip[1])
        print("Mask : [%d, %d] (score %.2e, clipped %.1f %%, blur %.2f)" % (got.center_y, got.center_x, got.score, 100.0 * got.clipped, got.sigma))
        return [got.center_y, got.center_x]
    got = utils.best_mask(frame, mask_size, clip, (1, M - 1, 1, N - 1))
    print("Mask : [%d, %d] (score %.2e, clipped %.1f %%)" % (got.center_y, got.center_x, got.score, 100.0 * got.clipped))
    return [got.center_y, got.center_x]


def _despeckle_args(despeckle):
    """`despeckle` of deblur_module -> None or (threshold, radius, coupling): threshold a float, a tuple of three floats or
    ("auto", strength)"""
    if despeckle is None:
        return None
    forms = "despeckle takes (threshold,), (threshold, radius) or (threshold, radius, coupling)"
    if isinstance(despeckle, str):
        raise ValueError("%s, got %r" % (forms, despeckle))
    try:
        despeckle = tuple(despeckle)
    except TypeError:
        raise ValueError("%s, got %r" % (forms, despeckle))
    if not 1 <= len(despeckle) <= 3:
        raise ValueError("%s, got %d values" % (forms, len(despeckle)))
    threshold, radius, coupling = (despeckle + (1, "vector")[len(despeckle) - 1:])[:3]
    from lib._native import despeckle_args
    try:
        t, radius, coupling, _ = despeckle_args(threshold, radius, coupling)
    except (ValueError, TypeError) as exc:
        raise ValueError("despeckle: %s" % exc)
    if t[0] != "auto":
        t = t[0] if len(set(t)) == 1 and np.ndim(threshold) == 0 else t
    return t, radius, coupling


def _local_contrast_args(local_contrast):
    """`local_contrast` of deblur_module -> None or (gains, thresholds or None, coupling), gains and thresholds as tuples of floats;
    thresholds "auto" or ("auto", strength) as ("auto", strength)"""
    if local_contrast is None:
        return None
    try:
        local_contrast = tuple(local_contrast)
    except TypeError:
        raise ValueError("local_contrast takes (gains,), (gains, thresholds) or (gains, thresholds, coupling), got %r" % (local_contrast,))
    if not 1 <= len(local_contrast) <= 3:
        raise ValueError("local_contrast takes (gains,), (gains, thresholds) or (gains, thresholds, coupling), got %d values" % len(local_contrast))
    gains, thresholds, coupling = (local_contrast + (None, "vector")[len(local_contrast) - 1:])[:3]
    from lib._native import wavelet_args
    try:
        checked = wavelet_args(gains, thresholds, 1.0, coupling)
    except (ValueError, TypeError) as exc:
        raise ValueError("local_contrast: %s" % exc)
    as_floats = lambda v: tuple(float(x) for x in np.atleast_1d(np.asarray(v, dtype=np.float64)))     # noqa: E731
    if isinstance(checked[1], tuple):                                    # "auto" or ("auto", strength): estimated on the frame it filters
        return as_floats(gains), checked[1], coupling
    return as_floats(gains), None if thresholds is None else as_floats(thresholds), coupling


def _detail_args(detail):
    """`detail` of deblur_module -> None or (radius, eps, gain, coupling)"""
    if detail is None:
        return None
    try:
        detail = tuple(detail)
    except TypeError:
        raise ValueError("detail takes (radius, eps, gain) or (radius, eps, gain, coupling), got %r" % (detail,))
    if len(detail) not in (3, 4):
        raise ValueError("detail takes (radius, eps, gain) or (radius, eps, gain, coupling), got %d values" % len(detail))
    radius, eps, gain, coupling = (detail + ("vector",))[:4]
    from lib._native import guided_args
    try:
        radius, eps, gain, coupling, _ = guided_args(radius, eps, gain, coupling)
    except ValueError as exc:
        raise ValueError("detail: %s" % exc)
    return radius, eps, gain, coupling


def _clarity_args(clarity):
    """`clarity` of deblur_module -> None or (sigma, detail, edges, coupling)"""
    if clarity is None:
        return None
    forms = "clarity takes (sigma, detail), (sigma, detail, edges) or (sigma, detail, edges, coupling)"
    try:
        clarity = tuple(clarity)
    except TypeError:
        raise ValueError("%s, got %r" % (forms, clarity))
    if len(clarity) not in (2, 3, 4):
        raise ValueError("%s, got %d values" % (forms, len(clarity)))
    sigma, gain, edges, coupling = (clarity + (1.0, "vector")[len(clarity) - 2:])[:4]
    from lib._native import llf_args
    try:
        sigma, gain, edges, _, _, coupling, _ = llf_args(sigma, gain, edges, None, 8, coupling)
    except ValueError as exc:
        raise ValueError("clarity: %s" % exc)
    return sigma, gain, edges, coupling


def _level_shape(i, M, N):
    """deconvolve.py:232-243 -- odd size of pyramid level `i`"""
    temp_width, temp_height = int(np.floor(i * N)), int(np.floor(i * M))
    if temp_width % 2 == 0:
        temp_width += 1
    if temp_height % 2 == 0:
        temp_height += 1
    return temp_height, temp_width


def _deblur_device(pic, filename, dest_path, blur_width, confidence, tolerance, quality, bits, mask, display, blur, preview, p, order, norm,
                   priority, mask_size, iterations, refocus, pyramid, save, despeckle=None, sharpen=None, denoise=None, local_contrast=None,
                   detail=None, clarity=None, fast_phase=None, fast_blind=None):
    """`deblur_module` (deconvolve.py:65-368) with every frame resident in HBM: one upload of the picture,
    one download of the result; pad_image, gamma, the window views, the resize between pyramid levels and the solver all
    work on `lib._native.DeviceImage`s.  Line references as in `deblur_module` above."""
    from lib._native import DeviceImage
    auto_width = _blur_width_args(blur_width)
    auto_mask = _mask_args(mask)
    if auto_width is None:
        if blur_width < 3:
            raise ValueError("The blur width should be at least 3 pixels.")
        elif blur_width % 2 == 0:
            raise ValueError("The blur width should be odd. You can use %i." % (blur_width + 1))
    raw = DeviceImage.from_host(pic)              # (uint8 / uint16 pictures cross PCIe as they are and become float32 on the device)
    pic_d = raw.pad_edge(1, 1, 1, 1)                                        # :94
    raw.close()
    pic_d.gamma(2 ** bits - 1, 1 / 2.2)                                     # :97-103
    if despeckle is not None:
        (pic_d, replaced), old = pic_d.despeckle(*despeckle, count=True), pic_d
        old.close()
        print("Despeckle :", ", ".join(str(n) for n in replaced), "replaced")
    step = {"normal": 1e-3, "high": 5e-4, "veryhigh": 1e-4, "low": 5e-3}[quality]
    M, N, _ = pic_d.shape
    if auto_mask is not None:
        mask = _auto_mask(pic_d, mask_size, auto_mask)
    whole_frame = mask is None
    if mask is None:
        mask = [M // 2, N // 2]
    top, bottom = mask[0] - mask_size // 2, mask[0] + mask_size // 2
    left, right = mask[1] - mask_size // 2, mask[1] + mask_size // 2
    print("Mask size :", (bottom - top + 1), "×", (right - left + 1))
    if not (top > 0 and bottom < M and left > 0 and right < N):
        raise ValueError("The mask is outside the picture boundaries. Move its center inside or reduce the blur size.")
    if auto_width is not None:
        blur_width = _auto_blur_width(pic_d, auto_width, None if whole_frame else (top, bottom + 1, left, right + 1))
    correlation = {"static": False, "motion": True}[blur]
    tolerance /= 100.
    odd_vert = odd_hor = False
    if M % 2 == 0:                                                          # :167-175
        pic_d, old = pic_d.pad_edge(1, 0, 0, 0), pic_d
        old.close()
        odd_vert = True
        print("Padded vertically")
    if N % 2 == 0:
        pic_d, old = pic_d.pad_edge(0, 0, 1, 0), pic_d
        old.close()
        odd_hor = True
        print("Padded horizontally")
    M, N, _ = pic_d.shape
    psf = utils.uniform_kernel(blur_width)
    psf = np.dstack((psf, psf, psf))
    images, kernels = build_pyramid(blur_width, confidence)
    if not pyramid:
        images, kernels = images[:1], kernels[:1]
    deb = pic_d.copy()
    import time
    from lib import _native
    phases = deblur_module.last_phase_seconds = {}      # wall time per phase of this call, device drained at the phase boundaries (bench.py reports it)
    try:
        for case in ["blind", "non-blind"]:
            _native.Context.get().synchronize()
            t_case = time.perf_counter()
            if case == "non-blind" and fast_phase is not None:
                deb, old = _fast_phase(pic_d, psf, fast_phase), deb
                old.close()
                _native.Context.get().synchronize()
                phases[case] = time.perf_counter() - t_case
                break
            if case == "blind" and fast_blind is not None:
                psf = _fast_blind(pic_d, (top, bottom + 1, left, right + 1), blur_width, fast_blind)
                _native.Context.get().synchronize()
                phases[case] = time.perf_counter() - t_case
                continue
            print("\n===== %s DECONVOLUTION =====" % case)
            deb.close()
            deb = pic_d.copy()
            lambd = confidence * 1000
            for i, k in zip(reversed(images), reversed(kernels)):
                print("======== Pyramid step %1.3f ========" % i)
                tt, tb, tl, tr = mask_window(i, top, bottom, left, right)
                th, tw = _level_shape(i, M, N)
                blurry = pic_d.resize(th, tw)                                # :245
                deb, old = deb.resize(th, tw), deb                           # :246
                old.close()
                if case == "blind":
                    psf_copy = np.ascontiguousarray(resize_bicubic(psf, (k, k, 3)).astype(np.float32))   # :249
                    dc.normalize_kernel(psf_copy, k)
                else:
                    psf_copy = np.ascontiguousarray(psf, dtype=np.float32).copy()
                    k = kernels[0]
                blurry, old = blurry.pad_edge(1, 1, 1, 1), blurry            # :256-257
                old.close()
                deb, old = deb.pad_edge(1, 1, 1, 1), deb
                old.close()
                pad = int(np.floor(k / 2))
                print("Image size", blurry.shape)
                print("u size", deb.shape)
                print("Mask size", (tb - tt), (tr - tl))
                print("PSF size", psf_copy.shape)
                tolerance_temp = tolerance if i == 1. else 0
                win = (pad + 1, tb - tt - pad - 1, pad + 1, tb - tt - pad - 1)
                if case == "blind" or preview:                               # :277-300: windows of both frames
                    dc.richardson_lucy_MM_device(
                        blurry, (tt - 1, tl - 1), deb, (tt - pad - 1, tl - pad - 1), psf_copy, *win,
                        0 if case == "blind" else tolerance_temp, tb - tt + 2, tr - tl + 2, 3, k, iterations, step, lambd,
                        blind=(case == "blind"), p=p, correlation=(correlation if case == "blind" else False), order=order, norm=2,
                        priority=(0 if case == "blind" else priority), refocus=refocus)
                    if case == "blind":
                        psf = psf_copy.copy()
                else:                                                        # :301-316: the whole frame
                    big = deb.pad_edge(pad, pad, pad, pad)
                    dc.richardson_lucy_MM_device(blurry, (0, 0), big, (0, 0), psf_copy, *win, tolerance_temp, th + 2, tw + 2, 3, k,
                                                 iterations, step, lambd, blind=False, p=p, order=order, norm=2, priority=priority,
                                                 refocus=refocus)
                    deb.close()
                    H2, W2, _ = big.shape
                    deb = big.crop(pad, H2 - pad, pad, W2 - pad)
                    big.close()
                blurry.close()
                H1, W1, _ = deb.shape
                deb, old = deb.crop(1, H1 - 1, 1, W1 - 1), deb               # :322-323
                old.close()
            _native.Context.get().synchronize()
            phases[case] = time.perf_counter() - t_case
    except KeyboardInterrupt:
        pass
    if denoise is not None:
        deb, old = deb.tv_denoise(*denoise), deb
        old.close()
    if clarity is not None:
        sigma, gain, edges, coupling = clarity
        deb, old = deb.local_laplacian(sigma, gain, edges, None, 8, coupling), deb
        old.close()
    if local_contrast is not None:
        gains, thresholds, coupling = local_contrast
        deb, old = deb.wavelet_equalize(gains, thresholds, 1.0, coupling), deb
        old.close()
    if detail is not None:
        deb, old = deb.guided_filter(*detail), deb
        old.close()
    if sharpen is not None:
        deb, old = deb.usm(*sharpen), deb
        old.close()
    deb.gamma(1.0, 2.2, 2 ** 16 - 1, clip01=True)                           # :346-352
    out = deb.to_host()
    deb.close()
    pic_d.close()
    if preview:
        filename = filename + "-preview"
        out = out[top:bottom, left:right, ...]
    else:
        if odd_hor:
            out = out[:, 1:, ...]
        if odd_vert:
            out = out[1:, :, ...]
        out = out[1:-1, 1:-1, ...]
    if save:
        utils.save(out, filename, dest_path)
    return out, psf


deblur_module.last_phase_seconds = {}


if __name__ == '__main__':
    import sys
    from PIL import Image
    if len(sys.argv) < 4:
        raise SystemExit("usage: python deconvolve.py <picture> <dest_dir> <blur_width> [mask_y mask_x]")
    with Image.open(sys.argv[1]) as pic:
        mask = [int(sys.argv[4]), int(sys.argv[5])] if len(sys.argv) >= 6 else None
        deblur_module(pic, sys.argv[1].rsplit("/", 1)[-1] + "-ics", sys.argv[2], int(sys.argv[3]), mask=mask, display=False)
