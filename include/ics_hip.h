/*
 * ics_hip.h -- C ABI of libics_hip.so: the MI355X (gfx950) implementation of the
 * Richardson-Lucy / MM deconvolution hot path of aurelienpierre/Image-Cases-Studies.
 *
 * This is the drop-in boundary.  Everything is `extern "C"`, plain pointers and sizes; host
 * arrays are float32, C-contiguous, HWC (channel fastest, 3 channels) exactly as the reference
 * passes numpy buffers to lib/deconvolution.pyx.  Every entry point returns 0 on success or a
 * negative ICS_E* code; ics_last_error() returns a thread-local description (HIP error string
 * included).  No entry point falls back to a CPU path: without a usable gfx950 device every
 * compute call fails with ICS_ENODEV.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   ics_rl_*               lib/deconvolution.pyx:341-675   richardson_lucy_MM (cpdef, :341-342)
 *   ics_normalize_kernel   lib/deconvolution.pyx:47-75     normalize_kernel (cpdef, :73-75)
 *   ics_tv                 lib/deconvolution.pyx:137-239   TV (cdef)
 *   ics_conv2d_symm        lib/utils.py:237-264            bessel_blur / gaussian_blur
 *                                                          (scipy.signal.convolve2d same/symm)
 *   ics_usm                lib/utils.py:267-277            USM
 *   ics_bilateral          lib/utils.py:173-234            bilateral_filter
 *   ics_img_*              deconvolve.py:24-37,:94-103,:245-257,:303,:322-323,:346-352
 *                                                          the frames the driver keeps between two
 *                                                          richardson_lucy_MM calls (pad_image, gamma, window
 *                                                          views, resize), device-resident
 *   ics_group_*            (none: the reference is single-process; SURVEY.md 8e defines image-per-GPU sharding)
 *   ics_resize_bicubic     deconvolve.py:245-249           skimage.transform.resize(order=3, mode="edge")
 *                                                          between pyramid levels (un-vendored dependency of
 *                                                          the reference: restated on scipy.ndimage semantics)
 * The Python side that binds these (ctypes) is image-cases-studies_amd/lib/_native.py; the
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef ICS_HIP_H
#define ICS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICS_ABI_VERSION 4 /* 3: self-describing ics_rl_params / ics_rl_stats (struct_size first), caller-owned traces,
                             per-outer-iteration callback, ics_group_allreduce_sum
                             4: the callback returns int (non-zero = stop after this outer iteration, stats.stopped = 2);
                                ics_rl_describe (which kernel family a run will use); the DoF ratio at exact 0/0 is 1 */

/* error codes */
#define ICS_OK 0
#define ICS_EINVAL (-1)  /* bad argument                                        */
#define ICS_ENODEV (-2)  /* no usable HIP device / wrong architecture            */
#define ICS_EHIP (-3)    /* a HIP runtime call failed (see ics_last_error)       */
#define ICS_ENOMEM (-4)  /* device or host allocation failed                     */
#define ICS_ESTATE (-5)  /* call sequence error (e.g. run before upload)         */
#define ICS_ENOSUP (-6)  /* unsupported size: PSF > 255, frame > 2 GiB */

typedef struct ics_ctx ics_ctx; /* one per (process, device): stream, events, scratch   */
typedef struct ics_rl ics_rl;   /* one deconvolution job: device-resident frames        */

/* ---- library / device ------------------------------------------------------------------ */
int ics_abi_version(void);
const char *ics_last_error(void);
int ics_device_count(int *count);
/* Creates a context on `device` (hipSetDevice + one non-blocking stream).  Fails with
 * ICS_ENODEV when the device is not gfx950. */
int ics_ctx_create(int device, ics_ctx **out);
void ics_ctx_destroy(ics_ctx *ctx);
int ics_ctx_synchronize(ics_ctx *ctx);
/* Device time in ms of the kernels of the last ics_conv2d_symm / ics_usm / ics_bilateral call (HIP events, transfers excluded). */
int ics_ctx_last_kernel_ms(ics_ctx *ctx, float *ms);
/* Device description: name (<=255 chars), compute units, HBM bytes. */
int ics_ctx_info(ics_ctx *ctx, char *name, size_t name_len, int *compute_units, uint64_t *hbm_bytes);

/* ---- Richardson-Lucy / MM job (lib/deconvolution.pyx:341-675) --------------------------- */

/* Called by ics_rl_run on the calling thread right after each outer iteration's statistics are known (pyx:593-659: the point
 * where the reference prints its progress lines), so that a binding can print them live.  `it` = outer iterations completed
 * (1-based), `stopped` = the stop test fired on this iteration.
 * Return value: 0 = go on; non-zero = ABORT: ics_rl_run leaves the loop after this outer iteration exactly as if `iterations`
 * had been `it` (u, psf and the statistics are those of iteration `it`, downloadable as usual) and reports
 * ics_rl_stats.stopped = 2.  This is the channel for deconvolve.py:338-342, which swallows a KeyboardInterrupt and keeps the
 * partial, in-place-updated `u`: a binding turns the interrupt it catches inside the callback into a non-zero return. */
typedef int (*ics_rl_progress_fn)(void *user, int it, int stopped, float dof_min, float dof_max, float M_r, float Hu, float varu);

/* Arguments of richardson_lucy_MM that are scalars (pyx:341-342).  `p, norm, order, priority,
 * refocus` are accepted and ignored by the reference and therefore absent.
 * struct_size MUST be sizeof(ics_rl_params) of the header the caller was built against: the library refuses any other
 * value with ICS_EINVAL instead of reading fields the caller never wrote (ics_rl_params_size() returns what it expects). */
typedef struct ics_rl_params {
  uint32_t struct_size;         /* = sizeof(ics_rl_params)                                 */
  int top, bottom, left, right; /* stats window, image coordinates (pyx:600-601,627)      */
  float tau;                    /* non-blind stop threshold (pyx:652)                      */
  int iterations;               /* max OUTER iterations, 5 inner each (pyx:375,460)        */
  float step_factor;            /* pyx:524,574                                             */
  float lambd;                  /* pyx:519                                                 */
  int blind;                    /* pyx:434,501,555                                         */
  int correlation;              /* pyx:584-585 (channel tie + caller-array rebinding quirk)*/
  int channels;                 /* `C`: bounds the blind channel loops (pyx:557,570); 3    */
  int tv_mode;                  /* ICS_TV_*: 0 = shipped behaviour (TV term dead)          */
  int stop_test;                /* 1 = evaluate the residual-whiteness stop test (pyx:623-654)
                                   on device every outer iteration (the reference always
                                   does); 0 = never stop early, M_r not computed;
                                   2 = compute M_r every outer iteration but never stop
                                   (fixed-length benchmark runs with the full workload)    */
  int profile;                  /* k > 0: bracket the kernel launches of every k-th inner iteration (k = 1:
                                   all) and the per-outer kernels with HIP events on the job's stream;
                                   per-kernel averages are reported in ics_rl_stats         */
  int fuse;                     /* 1: the image update of inner iteration i is fused in front of the next
                                   convolution (one kernel, u ping-pong; the fused kernel is an fp32 one: bit-identical results on the fp32 routes;
                                   on a matrix-core route A1 then takes fp32 products instead of fp16-split ones
                                   after the first inner iteration of an outer one, so results differ there in
                                   rounding (<= 1e-5 relative, tests/test_gpu_route_matrix.py).  Default 0:
                                   measured SLOWER on MI355X at 4096^2/15x15 (0.67 ms vs 0.28 + 0.19 ms),
                                   the 1.8x halo recompute with two IEEE divisions per element outweighs
                                   the saved frame pass (NOTES_r01.md section 4)                            */
  int conv;                     /* ICS_CONV_*: which kernels run the convolutions A1/A3 and the PSF gradient A13    */
  int flags;                    /* ICS_FLAG_* bits, 0 = defaults                                                     */
  int band_row0, band_row1;     /* ICS_STAGE_BAND_* only: the rows [row0, row1) this job OWNS when one image is split into
                                   row bands over several jobs / GPUs; u-frame rows for BAND_REDUCE,
                                   image rows for BAND_MASK_E.  Ignored everywhere else.                                */
  ics_rl_progress_fn progress;  /* NULL or the per-outer-iteration callback above (ics_rl_run only)                   */
  void *progress_user;
} ics_rl_params;
size_t ics_rl_params_size(void); /* sizeof(ics_rl_params) as the library was built */

#define ICS_FLAG_NO_FUSED_GRADK 1 /* blind, matrix-core path, MK <= 15: run A11 and A13 as two kernels (k_conv_mfma<K,0> +
                                     k_gradk_mfma) instead of the fused k_synth_gradk (ics_synth_gradk_mfma.hip); env
                                     ICS_FUSED_GRADK=0 does the same for an unmodified caller.  With the fused kernel the
                                     residual frame (ICS_BUF_ERROR) holds e' of pyx:555-565 only on the 64x64 tiles that
                                     meet the stats window -- the only place the loop reads it (pyx:600-601,627)         */
#define ICS_FLAG_STAGE_ASYNC 2    /* ics_rl_stage: return when the stage is queued on the job's stream instead of when it has run.  The ordering
                                     contract, as implemented: ics_rl_read*, ics_rl_scalars, ics_rl_copy_rows and the all-reduces are queued on
                                     (or synchronise with) the job's stream, so they see every stage queued before them.  ics_rl_exchange_rows
                                     is HOST-SYNCHRONOUS on both sides: it first drains the job's stream, runs its send / receive on the
                                     group's own stream and returns when that stream has drained -- stages queued after it see the halo rows,
                                     stages queued before it have finished.  A stage under ICS_CONV_FFT converts its frames back and drains the
                                     stream whatever this flag says.  So a sequence of stages needs no host synchronisation of its own
                                     (lib/banded.py BandRank: one per outer iteration, where the stop decision is taken); code that removes the
                                     exchange's host waits must replace them by events between the two streams.  Ignored by ics_rl_run.  */

#define ICS_CONV_AUTO 0   /* the library's choice (ics_rl_describe tells): inside ics_rl_run the fp32 transform tiles on large frames -- from 0.5 ... 12 Mpx
                             depending on the PSF size, every size 3 ... 255 (csrc/ics_route.hip fft_preferred) --, the cooperative fp32
                             iteration kernel on small ones -- up to ~290 px a side, MK <= 31, shipped loop (ics_small.hip) -- and the fp16x2-split
                             matrix-core kernels between (convolutions: MK <= 49 directly, above as tap blocks of <= 33 x 33; PSF gradient: MK <= 31
                             directly, above as tap blocks of <= 31 x 31); single stages (ics_rl_stage) always the latter; env
                             ICS_CONV_PATH=vector|matrix|fft overrides the choice of AUTO                     */
#define ICS_CONV_VECTOR 1 /* packed-fp32 VALU convolutions (ics_conv.hip; ics_big.hip above 63) + fp32 PSF gradient: fp32 products */
#define ICS_CONV_MATRIX 2 /* fp16 MFMA kernels (ics_conv_mfma.hip MK <= 49, ics_gradk_mfma.hip MK <= 31): operands split
                             into two fp16 terms (22 significand bits), three MFMAs per product, fp32 accumulate */
#define ICS_CONV_FFT 3    /* transform tiles (ics_conv_fft.hip, round 5; since round 6 every MK: one tile to 85, tap blocks to 255): A1 / A3 / A11 as 128 x 128 overlap-save
                             FFTs held in LDS, fp32 throughout -- the reference's own method (scipy's complex64 FFT over the frame,
                             lib/deconvolution.pyx:478,491), tile by tile; against float64 direct sums 2 - 5e-7 of the largest
                             convolution value.  The frames live as channel-planar mirrors for the duration of a run; the PSF gradient
                             runs on the same tiles (two forward transforms per tile pair, products added up in the frequency domain; env
                             ICS_FFT_GRADK=0: on the matrix cores).  Round 6: A11 + A13 as one three-transform unit per tile pair
                             (ICS_FFT_FUSED=0: two kernels) and, up to 25 x 25, A1 + A3 as one unit whose interior tiles never leave the
                             frequency domain (ICS_FFT_CONV2=0: two kernels).  What ICS_CONV_AUTO picks inside ics_rl_run on large frames
                             (above); env ICS_CONV_PATH=fft forces it wherever it is built.
                             The PAM kinds (tv_mode 2, 3) run on it as well (TV term, back-projection epilogue G = T + lambd * gradu and
                             update on the planar mirrors); tv_mode 1 is refused.  Where image and u are exactly 0 the
                             transforms return rounding noise instead of exact zeros, like the reference's (see "DoF ratio" below) */

/* Accuracy of the matrix-core path (tests/test_gpu_precision.py drives it with adversarial inputs).  Every fp32 operand x of a
 * 78 x 80-pixel tile is scaled by a power of two s (tile maximum m -> [2^14, 2^15)) and split, x s = hi + lo + r, hi and lo
 * fp16.  fp16 carries 11 significand bits down to 2^-14 and a fixed quantum of 2^-24 below, so
 *        |r| / s  <=  max( 2^-22 |x| , 2^-39 m ):
 * 22 bits for every element within 2^17 of the tile maximum, an ABSOLUTE error of 2^-39 of the tile maximum for smaller
 * ones (the PSF taps likewise, against the largest tap).  Products drop the lo*lo term (< 2^-22 |x w|) and accumulate in fp32:
 *        |err(sum w x)|  <=  8 * 2^-22 * sum |w||x|  +  2^-38 * ( m * sum |w|  +  w_max * sum |x| ).
 * Measured: local relative error 0.6 - 1.4e-6 (the fp32 kernels: 0.7 - 2.5e-6) on ordinary frames, on 0..65535 frames and with
 * pixels 10^4 above their tile; for residuals of 1e-7 next to an isolated 1.0 the absolute error is 5e-13 (1.6e-5 of the
 * local values).  For comparison the reference's own convolution, scipy's FFT in complex64 (lib/deconvolution.pyx:478),
 * has an absolute error of ~1e-7 of the FRAME maximum at every pixel.  There is therefore no data-dependent fall-back to
 * the fp32 kernels in ICS_CONV_AUTO; ICS_CONV_VECTOR remains for callers who want fp32 products regardless. */

/* DoF ratio (lib/deconvolution.pyx:499, A5).  The mask is D = ((g - f)/(g + f))^2 with g the raw back-projection and f the image,
 * evaluated in IEEE float32 like the reference -- with ONE defined exception: where g == 0 and f == 0 EXACTLY the ratio is 1, not
 * 0/0 = NaN.  Reason: in a region where image and u are exactly black (clipped shadows, letterbox bars, zero borders of at least
 * 2 MK - 1 px) the reference's g is the rounding noise of scipy's complex64 FFT (~1e-10, either sign), and (g - 0)/(g + 0) is 1 for
 * EVERY non-zero g: the reference returns a finite picture there (22 of 24 black-row cases run with the compiled reference,
 * tests/golden/rl_black.npz) unless one noise value happens to be exactly 0, in which case its whole frame becomes NaN (the 2 other
 * cases, and most frames with black COLUMNS, whose noise is coarsely quantised).  This library's convolutions are exact sums:
 * g = 0 there, and IEEE 0/0 would lose every such frame through the next convolution and the NaN-propagating maxima.  With the
 * rule the results match the reference wherever the reference is finite (u <= 3e-7, psf <= 2e-7; tests/test_gpu_black.py), and
 * stay finite where it is not.  Nothing else is touched: g + f == 0 with g != 0 is +-inf as in the reference, and a NaN that is
 * already in the image or in u propagates (and is reported through ics_rl_stats.has_nan) exactly as before. */

#define ICS_TV_SHIPPED 0 /* lib/deconvolution.pyx as shipped: else-branches :519/:545        */
#define ICS_TV_MM_ACTIVE 1 /* BUILD-DEFINED extension, parity unpinned: the if-branches :517/:543 made
                              reachable (TV_ut from the majoriser, image denoising step :547-549 live);
                              exact definition in oracle/rl_ext_oracle.py.  `image` is modified.      */
#define ICS_TV_PAM_ISO 2   /* BUILD-DEFINED, parity unpinned: PAM u-step (Perrone & Favaro 2014; reference
                              README.md:42,106 prose only) with an isotropic TV gradient, PSF step as
                              pyx:555-589; no majoriser term, no DoF blend (oracle/rl_ext_oracle.py)  */
#define ICS_TV_PAM_COLLAB 3 /* same with the collaborative L-inf,1,1 RGB TV gradient (README.md:113-114) */

/* Scalars the reference only prints (pyx:593,648,659,665-669).  The per-outer-iteration traces go into CALLER-OWNED arrays
 * of `trace_cap` floats each (any of them may be NULL; trace_cap = params.iterations holds every iteration -- the reference
 * has no limit on the number of outer iterations and neither has this).  struct_size as in ics_rl_params; the library
 * preserves struct_size, trace_cap and the five pointers and overwrites everything else. */
typedef struct ics_rl_stats {
  uint32_t struct_size; /* in: sizeof(ics_rl_stats)                                        */
  int iterations_done; /* `it` at exit                                                    */
  int stopped;         /* stop_flag (1: the stop test fired, pyx:643-654); 2: the progress callback asked to stop */
  int has_nan;         /* np.any(np.isnan(u)) (pyx:671)                                   */
  float M_r, Hu, varu; /* values at exit (pyx:669)                                        */
  float dof_min, dof_max;
  int trace_len;       /* out: entries written = min(iterations_done, trace_cap)          */
  int trace_cap;       /* in                                                              */
  float *trace_M_r, *trace_Hu, *trace_varu, *trace_dof_min, *trace_dof_max; /* in: arrays of trace_cap floats or NULL */
  /* timing of the last ics_rl_run, measured with HIP events on the job's stream */
  float ms_total;      /* whole run (first launch -> last kernel), device time             */
  int inner_iterations;/* inner iterations executed                                       */
  /* params.profile = 1: average milliseconds per launch and launch count per kernel class */
  float ms_kernel[12];  /* ICS_KERNEL_COUNT */
  int launches[12];
} ics_rl_stats;
size_t ics_rl_stats_size(void);

/* Allocates the device frames for an M x N x 3 image and MK x MK x 3 PSF (MK odd, 3 <= MK <= 255):
 * u is (M+2*(MK/2)) x (N+2*(MK/2)) x 3 as in pyx:372-376.  All sizes run on the matrix cores (to 49 directly, above as tap
 * blocks; 65 ... 255: shipped loop only, tv_mode 0, fuse 0); fp32-product kernels behind ICS_CONV_VECTOR (to 127).  Limits (the reference has none; each
 * fails with ICS_ENOSUP and a message, never silently): PSF sizes above 255 (the reference's own examples go to 45,
 * deconvolve.py:409), frames of 2 GiB and more (32-bit buffer offsets: about 13000 x 13000 px).  Stats windows of any size a
 * job can hold are evaluated: up to 4096 px a side with P x P transforms in LDS, larger ones with per-axis transforms of up to
 * 32768 points (a window that would need more, which no job below 2 GiB can hold, fails with ICS_ENOSUP). */
int ics_rl_create(ics_ctx *ctx, int M, int N, int MK, ics_rl **out);
void ics_rl_destroy(ics_rl *job);
/* Host -> device.  image: M*N*3, u: uM*uN*3, psf: MK*MK*3 floats, C-contiguous HWC. */
int ics_rl_upload(ics_rl *job, const float *image, const float *u, const float *psf);
/* Device -> host; any pointer may be NULL.  `psf_caller` is what the reference leaves in the
 * CALLER's psf array (differs from the local psf when correlation != 0, pyx:585). */
int ics_rl_download(ics_rl *job, float *u, float *psf_local, float *psf_caller);
/* Runs the whole loop (pyx:460-659) on the device.  Host synchronisation happens once per outer
 * iteration (to read the stop-test scalars), never inside the 5 inner iterations. */
int ics_rl_run(ics_rl *job, const ics_rl_params *params, ics_rl_stats *stats);

/* Which kernels ics_rl_run will launch for this job and these parameters.  (ics_rl_stage takes the same route EXCEPT for the transform
 * tiles: single stages run on them only under an explicit params.conv = ICS_CONV_FFT with tv_mode 0 -- under ICS_CONV_AUTO, and for the PAM
 * kinds, a stage-driven loop such as lib/banded.py runs the matrix-core / vector kernels where ics_rl_run would take the tiles; describe
 * such a loop with params.conv = ICS_CONV_MATRIX.)  Inputs: (PSF size, params.conv, tv_mode, fuse,
 * flags, the ICS_CONV_PATH override): the route ics_rl_run resolves and launches from, so that a benchmark labels its precision and
 * traffic figures from what actually runs.  Families:  convolutions A1/A3 -- 1 fp16-split matrix cores (whole PSF), 2 the same as tap blocks
 * (PSF > 49), 3 packed-fp32 kernels compiled per size, 4 run-time-sized fp32 kernels (ics_big.hip), 5 fp32 transform tiles on planar
 * mirrors (ics_conv_fft.hip), 6 the cooperative small-frame iteration kernel (ics_small.hip: the five inner iterations of an outer one in
 * ONE launch, a tile of a channel per compute unit, fp32 FMAs; frames up to ~290 px a side, PSF <= 31, shipped loop, ICS_CONV_AUTO only;
 * the PSF gradient is then family 8, inside the same launch);  PSF gradient A13 -- 1 fused with
 * A11 (k_synth_gradk, MK <= 15), 2 fp16-split matrix cores (k_gradk_mfma), 3 the same as tap blocks (MK >= 33), 4 fp32 MFMA
 * (k_gradk), 5 run-time-sized fp32 (k_gradk_big), 6 fp32 transform tiles (k_gradk_fft, ics_gradk_fft.hip),
 * 7 fused with A11 on the fp32 transform tiles (k_synth_gradk_fft: three transforms per tile pair); 0 = not run (non-blind).  products_fp16_split = 1 when the products of that
 * stage are formed from two fp16 terms per operand (22 significand bits, fp32 accumulation), 0 = fp32 products. */
typedef struct ics_rl_route {
  uint32_t struct_size; /* in: sizeof(ics_rl_route) */
  int conv_family, conv_fp16_split;
  int gradk_family, gradk_fp16_split;
  int image_in_accumulator_order; /* the residual kernels read the read-only accumulator-order copy of the image (ics_image_acc.h) */
  int graph;                      /* kept for the layout: always 0 */
} ics_rl_route;
int ics_rl_describe(ics_rl *job, const ics_rl_params *params, ics_rl_route *route);
/* The same for a shape alone -- no device and no job needed (a benchmark or a test labels its lines before anything is allocated). */
int ics_describe(int M, int N, int MK, const ics_rl_params *params, ics_rl_route *route);
/* Bytes ONE frame buffer of such a job takes on the device (aprons and tile padding included), 0 for an invalid shape: ics_rl_create refuses
   2 GiB and more (32-bit buffer offsets in the kernels).  No device needed.  lib/deconvolution.py uses it to send larger images through the row
   bands on one GPU (lib/banded.py) instead of failing -- the reference, lib/deconvolution.pyx:341, has no such limit. */
#define ICS_FRAME_LIMIT_BYTES 0x80000000ull
unsigned long long ics_rl_frame_bytes(int M, int N, int MK);

/* Stage-level entry points (parity tests, profiling).  They operate on the job's device frames. */
#define ICS_STAGE_SYNTH_RESIDUAL 1 /* A1+A2: error = conv_valid(u, psf) - image   (pyx:477-488)   */
#define ICS_STAGE_BACKPROJECT 2    /* A3 (+A7 reductions): gradu = corr_full(error, psf) (:490-491) */
#define ICS_STAGE_UPDATE 3         /* A5,A6,A8,A10: u update + DoF blend          (pyx:499-552)   */
#define ICS_STAGE_PSF_GRADIENT 4   /* A13: gradk                                   (pyx:567-571)   */
#define ICS_STAGE_PSF_UPDATE 5     /* A14-A17: psf step, tie, normalise, rotate    (pyx:574-589)   */
#define ICS_STAGE_MAJORIZE 6       /* ut = u                                       (pyx:462)       */
#define ICS_STAGE_STATS 7          /* A18+A19 on device -> stats scalars           (pyx:593-638)   */
#define ICS_STAGE_UPDATE_SYNTH 8   /* ICS_STAGE_UPDATE fused with ICS_STAGE_SYNTH_RESIDUAL (one kernel) */
#define ICS_STAGE_TVTERM 9         /* tv_mode 1: TV term T of u against ut (+ max|T_k|, max image_k)     */
#define ICS_STAGE_SYNTH_GRADK 10   /* A11 + A13 in one kernel (MK <= 15): gradk, and the residual e' over the whole frame */
/* One image over several jobs (row bands, lib/banded.py): a band job holds its rows plus a halo and computes everything on
 * them; only its OWNED rows are exact.  These two stages restrict the two global quantities of an inner iteration to them: */
#define ICS_STAGE_BAND_REDUCE 11   /* the step-size maxima of pyx:523-524 (max|g_k|, max u_k) over u-frame rows
                                      [band_row0, band_row1) only, from the back-projection of ICS_STAGE_BACKPROJECT: replaces
                                      the keys of ICS_BUF_RED; the caller combines them over the bands and writes them back */
#define ICS_STAGE_BAND_MASK_E 12   /* residual rows outside image rows [band_row0, band_row1) := 0, so that the PSF gradient
                                      of ICS_STAGE_PSF_GRADIENT sums the owned rows only (the caller adds the bands)       */
#define ICS_STAGE_SYNTH_BACKPROJECT 13 /* params.conv = ICS_CONV_FFT only: A1 + A2 + A3 (+A7) as ONE unit per tile pair (k_conv_fft<2>): gradu and the
                                          step-size maxima straight from u and the image; the residual frame is not written   */
int ics_rl_stage(ics_rl *job, int stage, const ics_rl_params *params);

/* Reads one device frame back in the reference's shape. */
#define ICS_BUF_U 0      /* uM x uN x 3 : after ics_rl_run, what ics_rl_download returns, on every family */
#define ICS_BUF_UT 1     /* uM x uN x 3 : the majoriser.  After ics_rl_run of n outer iterations: u as the last outer iteration found it (u after n - 1
                            iterations; the upload for n = 1) on the multi-launch HWC families and the small-frame kernel (families 1 ... 4, 6).  On the
                            transform tiles (family 5) the frames rotate as planar mirrors and only u and the residual are converted back: the buffer
                            read here is then undefined from n = 2 on.  ics_rl_write and ICS_STAGE_MAJORIZE define it for single stages */
#define ICS_BUF_GRADU 2  /* uM x uN x 3 : raw back-projection (A3), before A6.  After ics_rl_run: the last inner iteration's on the multi-launch families;
                            on the transform tiles (family 5) it lives in the frame's planar mirror and the buffer read here is not refreshed; the
                            cooperative small-frame kernel (family 6) never stores it (it stays in LDS) -- single stages (ics_rl_stage) always write it */
#define ICS_BUF_IMAGE 3  /* M x N x 3 : the image as uploaded, on every family (tv_mode 1 steps it on the device, pyx:547-549).  Every writer -- ics_rl_upload,
                            ics_rl_upload_img, ics_rl_write, ics_rl_write_rows, ics_rl_copy_rows, ics_rl_exchange_rows, that update -- drops the copies
                            the kernels keep of it (accumulator order, negated, planar mirror, the spectra of mode 2): the next run rebuilds them */
#define ICS_BUF_ERROR 4  /* M x N x 3    */
#define ICS_BUF_PSF 5    /* MK x MK x 3 : the local PSF (ics_rl_download's psf_local).  ics_rl_write of it repacks every weight table but, unlike
                            ics_rl_upload, touches neither psf_caller nor the flag that says a run with correlation = 1 has detached it: while the
                            flag is set, ICS_STAGE_PSF_UPDATE steps this buffer alone.  ics_rl_run resets the flag when it starts */
#define ICS_BUF_GRADK 6  /* MK x MK x 3 : after a blind ics_rl_run, the gradient of its last inner iteration */
#define ICS_BUF_TV 8      /* uM x uN x 3 : TV term T (tv_mode 1) */
#define ICS_BUF_SCALARS 7 /* 16 floats: dt[3], maxu[3], maxg[3], dtpsf, M_r, Hu, varu, dof_min, dof_max, 0.  ics_rl_run zeroes them when it starts
                             (dtpsf stays 0 behind a non-blind run, whatever ran on the job before) */
#define ICS_BUF_RED 9     /* 16 words (bit patterns in float slots): reduction keys of stage calls -- [0..2] max|g_k|,
                             [3..5] max u_k as order-preserving uint32 keys (larger key = larger float; NaN = 0xFFC00000);
                             read only: [12] min key, [13] max key, [14] NaN flag of the DoF mask of the last update (pyx:593) */
int ics_rl_read(ics_rl *job, int which, float *host, size_t count);
int ics_rl_write(ics_rl *job, int which, const float *host, size_t count);
/* Rows [row0, row0 + nrows) of a frame buffer (ICS_BUF_U / UT / GRADU: uN*3 floats per row; IMAGE / ERROR: N*3). */
int ics_rl_read_rows(ics_rl *job, int which, int row0, int nrows, float *host);
int ics_rl_write_rows(ics_rl *job, int which, int row0, int nrows, const float *host);
/* Rows of a frame buffer of one job into a frame buffer of another, device to device (the halo exchange and the stop-test
   gather of the row-band split, lib/banded.py): the two frames must have the same row length.  Jobs on different GPUs need peer
   access (xGMI); ICS_ENOSUP if the devices cannot reach each other -- the caller then goes through the host. */
int ics_rl_copy_rows(ics_rl *dst, int dst_which, int dst_row0, ics_rl *src, int src_which, int src_row0, int nrows);

/* Kernel classes indexing ics_rl_stats.ms_kernel / launches. */
#define ICS_K_SYNTH 0        /* A1+A2 convolution kernel        */
#define ICS_K_BACKPROJECT 1  /* A3 correlation kernel (+A7)     */
#define ICS_K_UPDATE 2       /* A5/A6/A8/A10 elementwise kernel */
#define ICS_K_PSF_GRADIENT 3 /* A13 MFMA kernel (+ reduction)   */
#define ICS_K_PSF_UPDATE 4   /* A14-A17                         */
#define ICS_K_MAJORIZE 5     /* ut = u copy                     */
#define ICS_K_STATS 6        /* A18/A19 window statistics + FFT */
#define ICS_K_UPDATE_SYNTH 7 /* fused A5-A10 + A1/A2 (or A11) kernel */
#define ICS_K_SYNTH_GRADK 8  /* fused A11 + A13 kernel (+ reduction)  */
#define ICS_K_SYNTH_BACKPROJECT 9 /* A1 + A2 + A3 (+A7) in one unit per tile pair (transform tiles, small PSFs) */
#define ICS_K_SMALL_ITER 10   /* small frames: the inner iterations of an outer one as ONE cooperative launch (ics_small.hip) */
#define ICS_KERNEL_COUNT 12  /* (11 reserved) */

/* ---- small standalone operators ---------------------------------------------------------- */
/* lib/deconvolution.pyx:73-75 -- in place on a host MK*MK*3 float32 array, computed on device. */
int ics_normalize_kernel(ics_ctx *ctx, float *kern, int MK);
/* lib/deconvolution.pyx:137-239 -- u: M*N*3 -> out, div (borders untouched = 0). */
int ics_tv(ics_ctx *ctx, const float *u, int M, int N, float epsilon, int order, int norm, float *out, float *div);
/* lib/utils.py:237-264 -- scipy.signal.convolve2d(src, kern, mode="same", boundary="symm"), float64.  LDS-tiled; a rank-1
 * kernel (every lib/utils.py window is one) runs as a row pass and a column pass.  The three filters keep their device
 * scratch in the context between calls. */
int ics_conv2d_symm(ics_ctx *ctx, const double *src, int H, int W, const double *kern, int KH, int KW, double *out);
/* lib/utils.py:267-277 -- src + (src - conv2d_symm(src, kern)) * amount. */
int ics_usm(ics_ctx *ctx, const double *src, int H, int W, const double *kern, int KH, int KW, double amount, double *out);
/* lib/utils.py:173-234 -- bilateral filter, symmetric padding, gaussian(x, s) = exp(-x^2/(2 s^2)). */
int ics_bilateral(ics_ctx *ctx, const double *src, int H, int W, int radius, double std_i, double std_s, double *out);

/* deconvolve.py:245-249 -- src: H x W x C float64 (HWC) -> out: OH x OW x C.  Gaussian anti-aliasing with
 * sigma = (scale - 1) / 2 per axis when shrinking, cubic B-spline interpolation at the pixel-centre grid, edge mode
 * "nearest"; the algorithm is written out in oracle/resize_oracle.py and pinned there against scipy.ndimage. */
int ics_resize_bicubic(ics_ctx *ctx, const double *src, int H, int W, int C, double *out, int OH, int OW);

/* ---- device-resident images -----------------------------------------------
 * H x W x 3 float32 HWC images in HBM, so that deblur_module (deconvolve.py:65-368) keeps its frames on the
 * device across pyramid levels and between the blind and the non-blind phase.  Operations are queued on the
 * context's stream; upload / download synchronise.  Functions with an `out` argument create a new image. */
typedef struct ics_img ics_img;
int ics_img_create(ics_ctx *ctx, int H, int W, ics_img **out);
void ics_img_destroy(ics_img *img);
int ics_img_shape(const ics_img *img, int *H, int *W);
int ics_img_upload(ics_img *img, const float *host);        /* H*W*3 floats */
/* the same from 8- or 16-bit pixels (what deconvolve.py:357-368 reads from its files): bytes_per_value = 1 (uint8) or 2 (uint16); the
 * values cross PCIe as they are and become float32 on the device (exact: np.float32(v)) -- a quarter / half of the float transfer and
 * no host-side conversion pass */
int ics_img_upload_int(ics_img *img, const void *host, int bytes_per_value);
int ics_img_download(const ics_img *img, float *host);
/* deconvolve.py:24-37 pad_image (np.pad mode="edge" on the two spatial axes) */
int ics_img_pad_edge(const ics_img *src, int top, int bottom, int left, int right, ics_img **out);
/* src[y0:y0+H, x0:x0+W] (the slices of deconvolve.py:322-323, :360-366) */
int ics_img_crop(const ics_img *src, int y0, int x0, int H, int W, ics_img **out);
/* dst[y0:y0+h, x0:x0+w] = src */
int ics_img_paste(ics_img *dst, int y0, int x0, const ics_img *src);
/* in place: x = powf(clip01 ? clip(x / div, 0, 1) : x / div, exponent) * mul
 * (deconvolve.py:100-103: div = 2^bits - 1, exponent = 1/2.2; :346-352: clip, exponent = 2.2, mul = 65535) */
int ics_img_gamma(ics_img *img, float div, float exponent, float mul, int clip01);
/* deconvolve.py:245-249 on a device image (ics_resize_bicubic semantics, result rounded to float32) */
int ics_img_resize(const ics_img *src, int OH, int OW, ics_img **out);
/* The lib/utils.py filters on a device image, each channel on its own (the reference filters pic[..., i] one after the other):
 * float32 arithmetic, FMA accumulation in a fixed order (two runs give identical bits).  Queued like the other ics_img_*
 * operations: no synchronisation, the result comes from the context's pool; ics_ctx_last_kernel_ms afterwards waits for the
 * kernels of the last one and returns their device time.
 * convolve: scipy.signal.convolve2d(channel, kern, mode="same", boundary="symm") (lib/utils.py:237-264); kern: KH x KW float32,
 *   row-major.  An outer product (every lib/utils.py window) runs as a row pass and a column pass, anything else as one
 *   KH x KW pass; ICS_ENOSUP when tile + halo exceed the 160 KB of LDS (rank 1: KW > 764 or KH > 129; otherwise e.g. above 71 x 71).
 * usm: src + (src - convolve(src, kern)) * amount (lib/utils.py:267-277), the epilogue of the last pass.
 * bilateral: lib/utils.py:173-234, symmetric padding by `radius`, gaussian(x, s) = exp(-x^2 / (2 s^2)); ICS_ENOSUP when the
 *   tile + halo exceed LDS (radius > 34). */
int ics_img_convolve(const ics_img *src, const float *kern, int KH, int KW, ics_img **out);
int ics_img_usm(const ics_img *src, const float *kern, int KH, int KW, float amount, ics_img **out);
int ics_img_bilateral(const ics_img *src, int radius, float std_i, float std_s, ics_img **out);
/* TV (Rudin-Osher-Fatemi) denoising of a device image: Chambolle's dual projection iteration for
 * min_u 1/2 |u - src|^2 + weight * TV(u), a fixed number of iterations (no early stop), tau = 1/8 (the step Chambolle's proof
 * covers; float32 rounding then does not grow with the iteration count).  q = (qx, qy) starts at 0 and per iteration
 *   u = src + div q,  (div q)[y,x] = qx[y,x] - qx[y,x-1] + qy[y,x] - qy[y-1,x]  (terms with index -1 are 0)
 *   gx = u[y,x+1] - u[y,x], gy = u[y+1,x] - u[y,x]  (0 in the last column / row),  s = gx^2 + gy^2
 *   q = (q + tau g) / (1 + (tau / weight) sqrt(s))
 * the result is src + div q; iterations = 0 copies src.  coupling 0 (channel): every channel on its own; 1 (vector): s is summed
 * over the three channels and shared by them (one edge set for all channels: chromatic noise is not kept as colour edges).
 * route 1: one launch per iteration; 2: ICS_IMG_TV_BLOCK iterations per launch on a tile in LDS; 0: the library's choice (see
 * DESIGN.md).  The routes give identical bits, and so do two runs.  Queued like the other image filters (no synchronisation;
 * ics_ctx_last_kernel_ms afterwards returns the device time of its kernels); src is not written.  ICS_EINVAL: weight <= 0 or
 * not finite, iterations < 0, unknown coupling or route.  Not pinned against skimage.restoration.denoise_tv_chambolle (which
 * steps with tau = 1/4). */
#define ICS_IMG_TV_BLOCK 4
int ics_img_tv_denoise(const ics_img *src, float weight, int iterations, int coupling, int route, ics_img **out);
/* Wavelet equaliser of a device image: an undecimated B3-spline ("a trous", starlet) decomposition into `scales` detail scales
 * (1 .. ICS_IMG_WAVELET_MAX_SCALES) whose details are soft-thresholded, multiplied by a gain and summed back.  c_0 = src and
 *   c_{j+1} = V_j(H_j(c_j)):  taps [1 4 6 4 1] / 16 at offsets {-2 .. 2} * 2^j along x (H_j), then along y (V_j); an index outside
 *     the picture folds as numpy.pad(mode="symmetric") (i mod 2n, then 2n - 1 - i if >= n: repeatedly on narrow frames); one axis
 *     pass is ((a[-2] + a[+2]) / 16 + (a[-1] + a[+1]) * 4 / 16) + a[0] * 6 / 16, without FMA
 *   w_j = c_j - c_{j+1},  s_j = shrink(w_j, thresholds[j])  (thresholds == NULL: all 0)
 *     coupling 0 (channel): sign(w) max(|w| - t, 0) per value;  1 (vector): w_c * (max(m - t, 0) / m) with
 *     m = sqrt(w_r^2 + w_g^2 + w_b^2), the squares added smallest first, 0 where m = 0 (IEEE square root and division)
 *   out = residual * c_J + (((gains[0] s_0) + gains[1] s_1) + ... ), accumulated in that order from zero.
 * gains all 1, thresholds 0, residual 1 gives src back up to rounding; gains above 1 lift the local contrast of their scale;
 * thresholds on the finest scales remove noise and leave the coarser scales alone.  route 1: one launch per scale; 2: the first
 * ICS_IMG_WAVELET_FUSED scales in one launch on a tile in LDS, the others as in route 1; 0: the library's choice.  The
 * routes give identical bits, and so do two runs.  Queued like the other image filters; src is not written.  ICS_EINVAL: scales
 * outside 1 .. 8, gains NULL, a gain / threshold / residual that is not finite, a negative threshold, unknown coupling or route. */
#define ICS_IMG_WAVELET_MAX_SCALES 8
#define ICS_IMG_WAVELET_FUSED 3
int ics_img_wavelet_equalize(const ics_img *src, int scales, const float *gains, const float *thresholds /* may be NULL */,
                             float residual, int coupling, int route, ics_img **out);
/* Noise estimate of a device image from the finest detail scale of the wavelet equaliser above (Donoho and Johnstone's robust
 * estimator; Starck and Murtagh for the starlet): w_0 = src - c_1 with exactly that arithmetic, and
 *   coupling 0 (channel): median[c] = the lower median of |w_0| of channel c, three results;
 *   coupling 1 (vector):  the lower median of m = sqrt(w_r^2 + w_g^2 + w_b^2), the squares added smallest first, in all three slots.
 * The lower median of n = H W values is the one of rank (n - 1) / 2 (from 0) in ascending order: exact, an element of the population,
 * found by a radix select on the device (no sort, no bins wider than one value); two runs and both routes give identical bits.  The
 * picture is taken to be finite.  The host derives, in double from the float32 median and rounded to float32,
 *   level = median / kappa, kappa = 0.6744897501960817 (channel: the median of |N(0, 1)|) or 1.5381722544550522 / sqrt(3) (vector: the
 *     median of a chi with 3 degrees of freedom over its rms): the rms of the thresholded quantity at scale 0 under Gaussian noise;
 *   sigma = level / e_0 (channel), level / (sqrt(3) e_0) (vector): the per-channel standard deviation of white noise in the picture,
 * where e_j (ICS_IMG_NOISE_E) is the L2 norm of the response of w_j to a unit impulse.  A threshold of `strength` standard deviations
 * at scale j is strength * level * e_j / e_0 (ICS_IMG_NOISE_STRENGTH: the 3 sigma rule); the Python layer's thresholds="auto" does
 * this.  route 1: every pass of the select recomputes w_0 from src; 2: the first pass writes the keys to a pooled buffer (12 / 4 bytes
 * per pixel), the later passes read them; 0: the library's choice.  Queued on the context's stream, its kernels bracketed
 * for ics_ctx_last_kernel_ms; then the results are copied back and WAITED FOR: with ics_img_download this is the only image entry
 * that synchronises.  src is not written.  ICS_EINVAL: src or an output NULL, unknown coupling or route. */
#define ICS_IMG_NOISE_STRENGTH 3.0f
#define ICS_IMG_NOISE_E {0.89079631027875839, 0.20066385102441897, 0.085507504753369934, 0.041217444374316202, \
                         0.020424966592781431, 0.01018975924921329, 0.0050920466808193074, 0.0025456694579151255}
int ics_img_noise_estimate(const ics_img *src, int coupling, int route, float median[3], float level[3], float sigma[3]);
/* Guided filter of a device image with the picture as its own guide (He, Sun, Tang): an edge-preserving base layer q from box means
 * and one closed-form solve per pixel, and the detail src - q scaled back onto it.  I' = src - 0.5;
 *   mean(x) = the sum of x over the (2 radius + 1)^2 window clipped to the picture / its pixel count; a sum runs along x first, then
 *     along y, the taps added from zero in ascending offset order, without running sums
 *   coupling 0 (channel), per channel: mu = mean(I'), v = mean(I'^2) - mu mu, a = v / (v + eps), b = mu - a mu
 *   coupling 1 (vector): mu_i = mean(I'_i), S_ij = mean(I'_i I'_j) - mu_i mu_j, M = S + eps E, c_ij its six cofactors,
 *     det = (M00 c00 + M01 c01) + M02 c02, A_ij = [i = j] - eps (c_ij / det) (= M^-1 S, symmetric), b_i = mu_i - sum_j A_ij mu_j:
 *     one set of edges for the three channels
 *   q = mean(a) I' + mean(b) + 0.5 (vector: mean(A) I' + mean(b) + 0.5);  out = q when detail == 0, else q + detail (src - q).
 * detail above 1 lifts texture without halos at the edges, between 0 and 1 smooths it; eps is the variance (of values in [0, 1])
 * below which a window counts as flat.  No FMA, IEEE division (restated in tests/guided_ref.py).  route 1: two launches, any radius
 * up to ICS_IMG_GUIDED_MAX_RADIUS; 2: one launch with the coefficients kept in LDS, radius <= ICS_IMG_GUIDED_FUSED_RADIUS; 0: the
 * library's choice.  The routes give identical bits, and so do two runs.  Queued like the other image filters; src is
 * not written.  ICS_EINVAL: radius outside 1 .. 32, eps not finite or <= 0, detail not finite, unknown coupling or route, route 2
 * with a radius above ICS_IMG_GUIDED_FUSED_RADIUS. */
#define ICS_IMG_GUIDED_MAX_RADIUS 32
#define ICS_IMG_GUIDED_FUSED_RADIUS 8
int ics_img_guided(const ics_img *src, int radius, float eps, float detail, int coupling, int route, ics_img **out);
/* Fast local Laplacian filter of a device image (Paris, Hasinoff, Kautz 2011; sampled as Aubry et al. 2014): contrast at scales of
 * tens to hundreds of pixels lifted or smoothed without halos, and the tonal range compressed with the detail kept.
 *   signal: coupling 0 (channel) each channel by itself; 1 (vector) Y = (0.2126 R + 0.7152 G) + 0.0722 B and out_c = in_c + (Y' - Y)
 *   reduce, n -> (n + 1) / 2: taps 1 4 6 4 1 at 2 y - 2 .. 2 y + 2, indices folded as numpy.pad(mode="symmetric"),
 *     (((a0 + a4) + 2 a2) + 4 a2) + 4 (a1 + a3) along y, then along x, then times 1 / 256 (the 6 split so that a constant stays exact)
 *   expand to a size, indices clamped: position 2 k (((c[k-1] + c[k+1]) + 2 c[k]) + 4 c[k]) / 8, 2 k + 1 (c[k] + c[k+1]) / 2; y, then x
 *   remap about g, d = i - g: r_g(i) = g + d (edges + (detail - edges) exp(-d d / (2 sigma^2)))
 *   samples g_k = k / (samples - 1); G the Gaussian pyramid of the signal, P_k that of r_{g_k}(signal), L_k[l] = P_k[l] - expand(P_k[l+1])
 *   level l < levels, pixel p: t = clamp(G[l](p) (samples - 1), 0, samples - 1), k0 = min(floor(t), samples - 2), f = t - k0,
 *     OL[l](p) = a + f (b - a), a = L_k0[l](p), b = L_{k0+1}[l](p);  R[levels] = G[levels], R[l] = OL[l] + expand(R[l+1]); result R[0].
 * detail: gain of differences well below sigma (above 1 clarity, below 1 smoothing); edges: gain of differences well above sigma
 * (below 1 compresses the tonal range).  No FMA, one expf (restated in tests/llf_ref.py).  Every `levels` is legal for every size
 * (sizes bottom out at 1) and values outside [0, 1] are legal (t is clamped).  route 1: a reduce chain per sample; 2: one reduce
 * launch per level for all samples, the frame read once; 0: the library's choice.  The routes give identical bits, and so
 * do two runs.  Queued like the other image filters; src is not written.  ICS_EINVAL: sigma not finite or <= 0, detail not finite or
 * < 0, edges not finite or <= 0, detail > 3 edges (the remap would stop being monotone near 3.24 edges), levels outside
 * 1 .. ICS_IMG_LLF_MAX_LEVELS, samples outside 2 .. ICS_IMG_LLF_MAX_SAMPLES, unknown coupling or route. */
#define ICS_IMG_LLF_MAX_LEVELS 10
#define ICS_IMG_LLF_MAX_SAMPLES 16
int ics_img_local_laplacian(const ics_img *src, float sigma, float detail, float edges, int levels, int samples, int coupling, int route,
                            ics_img **out);
/* Despeckle of a device image: a thresholded median that removes impulses (hot and dead sensor pixels, salt and pepper, NaN / inf
 * from an upstream tool) before a deconvolution would spread them, and leaves every other value bit for bit as it was.
 *   order: values are ordered by the integer key of their bits b, key = b ^ 0xFFFFFFFF if the sign bit is set, else b | 0x80000000:
 *     a total order, -0 below +0, NaNs at the two ends by sign; selection is by key, never by a floating-point compare
 *   window of (y, x): the (2 radius + 1)^2 pixels at (clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)): n = 9 or 25 values
 *   med_c = the value of rank (n - 1) / 2 of channel c of the window in key order: one of the input values, no arithmetic
 *   d_c = |src_c - med_c| (one float32 subtraction), hit_c = !(d_c <= t_c): a NaN difference counts as a hit
 *   coupling 0 (channel): out_c = hit_c ? med_c : src_c with threshold[c]; replaced[c] = the hits of channel c
 *   coupling 1 (vector): one threshold, threshold[0]; hit = hit_0 || hit_1 || hit_2, all three channels of a hit pixel become their
 *     medians (a defect leaves no coloured remainder); replaced[0] = the hit pixels, replaced[1] = replaced[2] = 0.
 * threshold 0 replaces every value that differs from its median: the plain median filter.  ICS_IMG_DESPECKLE_STRENGTH: the Python
 * layer's threshold "auto" is this many sigma of ics_img_noise_estimate of the same frame (a convention).  Restated in
 * tests/despeckle_ref.py; the result is a selection and the decision one correctly rounded subtraction, so routes, runs and the
 * restatement agree bit for bit.  route 1: a lane reads its windows from the frame; 2: a workgroup stages its tile and halo in LDS; 0:
 * the library's choice.  Queued like the other image filters, its kernel bracketed for ics_ctx_last_kernel_ms; src is not
 * written.  replaced may be NULL; given, the three counters are copied back and WAITED FOR.  ICS_EINVAL (*out NULL): src, out or
 * threshold NULL, radius outside 1 .. ICS_IMG_DESPECKLE_MAX_RADIUS, a threshold that is read and is negative, NaN or infinite,
 * unknown coupling or route. */
#define ICS_IMG_DESPECKLE_MAX_RADIUS 2
#define ICS_IMG_DESPECKLE_STRENGTH 6.0f
int ics_img_despeckle(const ics_img *src, int radius, const float threshold[3], int coupling, int route, ics_img **out, unsigned replaced[3]);
/* Blur profile of a device image: the autocorrelation of the picture's derivatives along x and along y, from which the blur width is
 * read (the derivative of a sharp picture is close to white along its axis, so that of a blurred one correlates with itself over
 * as many pixels as the PSF is wide and no further; Yitzhaky and Kopeika).  Over the half-open window [y0, y1) x [x0, x1):
 *   Y = (R + G + B) * (1 / 3), every operation rounded once to float32
 *   dx[y,x] = Y[y,x+1] - Y[y,x], dy[y,x] = Y[y+1,x] - Y[y,x], for both pixels inside the window
 *   Sx(l) = the sum over the window of dx[y,x] * dx[y,x+l] for every pair inside it, nx(l) = the number of such pairs
 *     = (y1 - y0) * max(x1 - x0 - 1 - l, 0); Sy(l), ny(l) likewise with dy along y;  l = 0 .. max_lag
 *   ax[l] = Sx(l) / nx(l), ay[l] = Sy(l) / ny(l), 0 where the count is 0.
 * Products and the sums inside a tile of 32 x 64 difference values are float32, in one fixed order; the tiles are summed in row-major
 * order and divided in double.  No atomics: two runs give identical bits.  ax, ay, nx, ny hold max_lag + 1 entries each.  The rule
 * that turns a profile into an extent (half-maximum line fit, lags 0 and 1 left to the picture's noise) is the Python layer's
 * blur_extent; it is restated with the profiles in tests/blur_width_ref.py.  One route.  Queued on the context's stream, its kernels
 * bracketed for ics_ctx_last_kernel_ms, then the 2 (max_lag + 1) doubles are copied back and WAITED FOR.  src is not written.
 * ICS_EINVAL: src or an output NULL, an empty window or one outside the frame, max_lag < 0 or > ICS_IMG_BLURWIDTH_MAX_LAG. */
#define ICS_IMG_BLURWIDTH_MAX_LAG 128
int ics_img_blur_profile(const ics_img *src, int y0, int y1, int x0, int x1, int max_lag, double *ax, double *ay, long long *nx, long long *ny);
/* Window scores of a device image: the box of `size` pixels a side, inside the half-open region [y0, y1) x [x0, x1), on which the blind
 * phase should estimate the PSF.  A window is good for that when it holds strong edges in every orientation (one dominant direction
 * leaves the PSF free along it) and no clipped pixels (they break the linear blur model): the score is the smaller eigenvalue of the
 * window's structure tensor of luma differences (Shi and Tomasi's criterion on a whole window), clipped pixels taken out of the sums.
 *   usable: fabsf(v) < clip for all three channels (a NaN or an inf is never usable; clip = inf keeps every finite pixel)
 *   Y = (R + G + B) * (1 / 3), every operation rounded once to float32
 *   dx[y,x] = Y[y,x+1] - Y[y,x] where x + 1 < x1 and both pixels are usable, else 0; dy[y,x] = Y[y+1,x] - Y[y,x] likewise with y + 1 < y1
 *   cells of 16 x 16 pixels, n = size / 16, off = (size - 16 n) / 2, the grid anchored at (y0 + off, x0 + off); per cell
 *     Sxx = sum dx dx, Syy = sum dy dy, Sxy = sum dx dy (float32, one fixed order, no contraction) and the number of unusable pixels
 *   candidates: boxes with origin (y0 + 16 i, x0 + 16 j), i = 0 .. (y1 - y0 - size) / 16, j likewise; box (i, j) is scored over the
 *     cells [i, i + n) x [j, j + n) -- the whole cells centred in the box, its inner 16 n pixels -- added in double in row-major order:
 *     trace = (Sxx + Syy) / (16 n)^2, score = max(0, (Sxx + Syy - sqrt((Sxx - Syy)^2 + 4 Sxy^2)) / 2 / (16 n)^2), clipped = the count
 *   choice: the largest score, ties to the lowest i, then the lowest j (a flat or wholly clipped frame: box (0, 0), score 0).
 * box_y, box_x: the origin of the chosen box in the frame (y0 + 16 i, x0 + 16 j); score, trace, clipped: its values.  map (may be
 * NULL): the score of every candidate, row-major, map_rows x map_cols == the candidate grid.  No atomics: two runs give identical bits.
 * One route.  Queued on the context's stream, its kernels bracketed for ics_ctx_last_kernel_ms, then the result block (and the map) is
 * copied back and WAITED FOR.  src is not written.  ICS_EINVAL, the message naming the argument: src or a scalar output NULL, a region
 * that is empty or outside the frame, size < 16, a region smaller than size on either axis, clip not positive (or NaN), a map of
 * another shape than the candidate grid. */
#define ICS_IMG_MASK_CELL 16
int ics_img_window_scores(const ics_img *src, int y0, int y1, int x0, int x1, int size, float clip, int *box_y, int *box_x, double *score, double *trace,
                          long long *clipped, double *map, int map_rows, int map_cols);
/* Blur map of a device image: the local blur width on a grid of 16 x 16 cells, in one launch (Zhuo and Sim's gradient ratio: the luma
 * smoothed by two Gaussians sigma_a < sigma_b; at an edge pixel of a step blurred by a Gaussian of s the gradient magnitudes stand in
 * the ratio R = sqrt((s^2 + sigma_b^2) / (s^2 + sigma_a^2))).  Over the half-open window [y0, y1) x [x0, x1), every coordinate clamped
 * to the window, every operation rounded once to float32:
 *   Y = (R + G + B) * (1 / 3)
 *   taps g_s[i] = exp(-i^2 / (2 s^2)), i = -r .. r, r = ceilf(3.f * s), normalised in double on the host, rounded to float32
 *   S_s = the rows pass, then the columns pass: acc = 0, acc = acc + g[i] * v for i ascending
 *   gx = 0.5 * (S[y, x+1] - S[y, x-1]), gy likewise; A = sqrt(gx gx + gy gy) of S_sigma_a, B of S_sigma_b
 *   sector of the gradient of S_sigma_a by ics_img_edge_mask's rule; neighbour offsets (dy, dx) = (0, 1), (1, 1), (1, 0), (1, -1)
 *   kept: A > A[y+dy, x+dx], A >= A[y-dy, x-dx], A >= edge, B > 0, R = A / B > 1,
 *     s2 = (sigma_b^2 - (R R) sigma_a^2) / (R R - 1) <= max_sigma^2; its value is sigma = sqrt(max(s2, 0))
 *   cell (i, j) = the pixels [y0 + 16 i, y0 + 16 i + 16) x [x0 + 16 j, ...) of the window (ragged at the far edges): weight = sum A,
 *     moment = sum A sigma, count, over its kept pixels -- a row left to right, the row sums top to bottom, a pixel that is not kept
 *     adding exactly 0.  The cell's blur width is moment / weight.
 * weight, moment, count: rows x cols entries, row-major, rows == ceil((y1 - y0) / 16), cols == ceil((x1 - x0) / 16).  *bad: the number
 * of pixels of the window whose luma is not finite (the map around such a pixel means nothing: despeckle first).  sparse (may be NULL):
 * (y1 - y0) x (x1 - x0) floats, sigma at the kept pixels and -1 elsewhere, written by the same launch.  No atomics: two runs give
 * identical bits (restated in tests/blur_map_ref.py).  One route.  Queued on the context's stream, its kernel bracketed for
 * ics_ctx_last_kernel_ms, then the grid (and the plane) is copied back and WAITED FOR.  src is not written.  ICS_EINVAL, the message
 * naming the argument: src or an output NULL, a window that is empty or outside the frame, sigmas outside 0.5 <= sigma_a < sigma_b with
 * ceilf(3.f * sigma_b) <= ICS_IMG_BLURMAP_MAX_RADIUS, edge or max_sigma not positive (or NaN), a grid of another shape. */
#define ICS_IMG_BLURMAP_CELL 16
#define ICS_IMG_BLURMAP_MAX_RADIUS 8
int ics_img_blur_map(const ics_img *src, int y0, int y1, int x0, int x1, float sigma_a, float sigma_b, float edge, float max_sigma,
                     float *weight, float *moment, int *count, long long *bad, float *sparse, int rows, int cols);
/* Wiener deconvolution of a device image by a known PSF: a regularised inverse filter on one 2-D transform of the whole frame, the
 * fast non-blind step beside the Richardson-Lucy loop.  psf: K x K x 3 host floats (HWC like ics_rl_upload), K odd, 3 .. 255,
 * K <= min(H, W), every channel of sum 1 (the Python layer normalises); balance > 0.
 *   Py, Px = the smallest powers of two >= H + K - 1, W + K - 1
 *   ext: the frame extended to Py x Px without a step at the wrap-around: along y, for every column, rows H .. Py - 1 are
 *     (1 - t / g) f[H - 1] + (t / g) f[0], g = Py - H + 1, t = 1 .. g - 1; then the same along x on all Py rows with W and Px
 *   Hc = the transform of channel c of the PSF, zero padded to Py x Px, its centre tap (K / 2, K / 2) rolled to (0, 0)
 *   L(ky, kx) = 4 - 2 cos(2 pi ky / Py) - 2 cos(2 pi kx / Px)   (the Laplacian skimage.restoration.wiener regularises with)
 *   G = conj(Hc) / (|Hc|^2 + balance L^2);  out_c = real(inverse transform(G transform(ext_c)))[:H, :W].  Nothing is clipped.
 * float32 throughout, no atomics: two runs give identical bits (restated in float64 in tests/wiener_ref.py).  A delta PSF does not
 * return the input (G = 1 / (1 + balance L^2) is a low-pass); a NaN spreads over the whole frame.  Queued like the other image
 * filters, its kernels bracketed for ics_ctx_last_kernel_ms; src is not written.  ICS_EINVAL (*out NULL): src, psf or out NULL, K even
 * or outside 3 .. 255 or above min(H, W), balance not finite or <= 0.  ICS_ENOSUP: H + K - 1 or W + K - 1 above
 * ICS_IMG_WIENER_MAX (a line and its ping-pong copy fill the LDS of a compute unit).
 * ics_img_wiener_plan: the transform sizes and the device bytes such a call takes from the context's pool (no device needed); same
 * checks on H, W, K. */
#define ICS_IMG_WIENER_MAX 8192
int ics_img_wiener(const ics_img *src, const float *psf, int K, float balance, ics_img **out);
int ics_img_wiener_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);
/* TV-regularised deconvolution of a device image by a known PSF: minimise sum |Du| + (fidelity / 2) |h * u - f|^2, total variation
 * plus a quadratic data term, by variable splitting (FTVd, Wang, Yang, Yin, Zhang 2008, in its split-Bregman / ADMM form, Goldstein and
 * Osher 2009): every iteration is one shrinkage of the gradient per pixel and one linear solve that is diagonal under the 2-D
 * transform.  The method between ics_img_wiener (no image prior) and the Richardson-Lucy loop.  psf, K, Py, Px, ext, Hc, L as for
 * ics_img_wiener (L itself, not its square: it is the transfer of D^T D for periodic forward differences); everything runs on the
 * periodic Py x Px domain.  mu = fidelity > 0, beta = penalty > 0, n = iterations, 1 .. ICS_IMG_TVD_MAX_ITERATIONS (a fixed count, no
 * stopping rule); coupling 0: every channel is shrunk by its own gradient magnitude, 1: the three by their common one.
 *   N0c = mu conj(Hc) transform(ext_c),  Gc = 1 / (mu |Hc|^2 + beta L),  u = ext, bx = by = 0;  n times (indices mod Px, Py):
 *     vx = u[y, x+1] - u[y, x] + bx,  vy = u[y+1, x] - u[y, x] + by
 *     m = sqrt(vx^2 + vy^2) (coupling 1: summed over the three channels too);  s = (m - 1 / beta) / m where m > 1 / beta, else 0
 *     wx = s vx, wy = s vy;  bx = vx - wx, by = vy - wy;  px = wx - bx, py = wy - by
 *     z = (px[y, x-1] - px[y, x]) + (py[y-1, x] - py[y, x]);  u_c = real(inverse transform((N0c + beta transform(z_c)) Gc))
 *   out = u[:H, :W].  Nothing is clipped.
 * float32 throughout, every operation of the shrinkage rounded once, no atomics: two runs give identical bits (restated in float64
 * in tests/tv_deconv_ref.py).  A NaN spreads over the whole frame.  Queued like the other image filters, its kernels bracketed for
 * ics_ctx_last_kernel_ms; src is not written.  ICS_EINVAL (*out NULL): src, psf or out NULL, K even or outside 3 .. 255 or above
 * min(H, W), fidelity or penalty not finite or <= 0, iterations outside 1 .. ICS_IMG_TVD_MAX_ITERATIONS, coupling neither 0 nor 1.
 * ICS_ENOSUP: H + K - 1 or W + K - 1 above ICS_IMG_WIENER_MAX.
 * ics_img_tv_deconvolve_plan: the transform sizes and the device bytes such a call takes from the context's pool, 11 floats per
 * transform point and channel and the tables (no device needed); same checks on H, W, K. */
#define ICS_IMG_TVD_MAX_ITERATIONS 500
int ics_img_tv_deconvolve(const ics_img *src, const float *psf, int K, float fidelity, float penalty, int iterations, int coupling, ics_img **out);
int ics_img_tv_deconvolve_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);
/* ics_img_tv_deconvolve with a masked data term: minimise sum |Du| + (fidelity / 2) |M (h * u - f)|^2, M a 0/1 plane shared by the
 * three channels.  What is not data is not fitted: the extension of the frame to the transform size (the pixels beyond the frame that
 * the PSF mixed into its rim are unknown), clipped highlights, non-finite pixels, and whatever the caller marks.  The mask breaks the
 * diagonal solve; one more splitting variable v = h * u with its multiplier d and its penalty gamma = data_penalty restores it
 * (Almeida and Figueiredo, "Deconvolving images with unknown boundaries using the alternating direction method of multipliers", IEEE
 * TIP 2013).  psf, K, Py, Px, Hc, L, mu, beta, n, coupling as for ics_img_tv_deconvolve.  observed: H W host bytes, row-major, or
 * NULL for all non-zero; clip: a pixel with a channel at or above it is unobserved, +inf for none.
 *   m = observed != 0 and the three channels finite and the three channels < clip;  f0 = f with non-finite values 0
 *   ext = the ramp extension of f0;  M = m on the frame, 0 on every extension pixel
 *   Gc = 1 / (gamma |Hc|^2 + beta L),  u = ext, bx = by = d = 0, r_c = real(inverse transform(Hc transform(ext_c)));  n times:
 *     u, bx, by -> bx, by, z: the shrinkage of ics_img_tv_deconvolve
 *     t = r + d;  v = (mu M ext + gamma t) / (mu M + gamma);  d = t - v;  q = v - d
 *     U_c = (gamma conj(Hc) transform(q_c) + beta transform(z_c)) Gc;  u_c = real(inverse transform(U_c)),  r_c = real(inverse transform(Hc U_c))
 *   out = u[:H, :W].  Nothing is clipped.  *unobserved (where not NULL): the frame pixels with m false.
 * float32 throughout, no atomics, every sum in one order: two runs give identical bits (restated in float64 in
 * tests/tvm_deconv_ref.py).  Near clipped highlights the mask pays from about 30 iterations, not at 10; nothing keeps the result
 * positive.  Queued like the other image filters, its kernels bracketed for ics_ctx_last_kernel_ms; with unobserved given the call
 * waits for the count.  src is not written.  ICS_EINVAL (*out NULL): as ics_img_tv_deconvolve, and clip not above 0 (NaN included),
 * data_penalty not finite or <= 0.  ICS_ENOSUP: H + K - 1 or W + K - 1 above ICS_IMG_WIENER_MAX.
 * ics_img_tv_deconvolve_masked_plan: the transform sizes and the device bytes such a call takes from the context's pool,
 * 4 (43 Py Px + Py + 4) + Py Px and the tables of ics_img_wiener (14 1/3 floats per transform point and channel, the row counts, a
 * byte per point for the caller's mask); no device needed; same checks on H, W, K. */
int ics_img_tv_deconvolve_masked(const ics_img *src, const float *psf, int K, const unsigned char *observed, float clip, float fidelity, float penalty, float data_penalty, int iterations, int coupling, long long *unobserved, ics_img **out);
int ics_img_tv_deconvolve_masked_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);
/* The PSF that takes a sharp device image to a blurred one of the same scene, the linear solve of the fast blind methods (Cho and Lee
 * 2009; Xu and Jia 2010) on image derivatives: k = argmin sum |d s * k - d b|^2 + gamma |k|^2, diagonal under the 2-D transform.
 * (y0, y1, x0, x1): a half-open box inside both frames, H x W its sides; K odd, 3 .. 255, K <= min(H, W); regularisation > 0;
 * coupling 0: a PSF per channel, 1: one PSF from the three channels, its plane three times in raw and its energy three times.
 *   Py, Px = those of ics_img_wiener for H, W, K
 *   wy[y] = 0.5 - 0.5 cos(pi (j + 0.5) / Ty) for j = min(y, H - 1 - y) < Ty = min(K, H / 2), else 1; wx likewise; w = wy (x) wx
 *     (the pair obeys b = s * k only away from the border)
 *   d_x f[y, x] = w[y, x] (f[y, x+1] - f[y, x]), 0 at x = W - 1; d_y f likewise; zero beyond H x W up to Py x Px (no ramp)
 *   A = transform(d s_c), B = transform(d b_c);  N = sum conj(A) B,  D = sum |A|^2,  S = sum over the pixels of (d s_c)^2, over the
 *     two directions (coupling 1: and the three channels)
 *   full = real(inverse transform(N / (D + regularisation S)));  raw[i, j] = full[(i - K / 2) mod Py, (j - K / 2) mod Px]
 * so that b ~ s * raw, a true convolution with the centre tap at (K / 2, K / 2): ics_img_wiener(b, raw normalised) undoes it.
 * raw: K K 3 host floats (HWC), nothing clipped or normalised (the Python layer projects); energy: S per channel.  float32
 * throughout, the energy summed in double, no atomics, every sum in one order: two runs give identical bits (restated in float64 in
 * tests/psf_est_ref.py).  s must be registered to b; a NaN spreads; a sharp frame without gradients gives energy 0 and a raw that
 * means nothing.  Its kernels are bracketed for ics_ctx_last_kernel_ms; the call waits for raw and energy; neither frame is written.
 * ICS_EINVAL, before a frame is touched: a NULL pointer, an empty box or one with a negative corner, K even or outside 3 .. 255 or
 * above the box, regularisation not finite or <= 0, coupling neither 0 nor 1; then: frames of different shape or context, a box
 * outside them.  ICS_ENOSUP: H + K - 1 or W + K - 1 above ICS_IMG_WIENER_MAX.
 * ics_img_psf_estimate_plan: the transform sizes and the device bytes such a call takes from the context's pool: twelve complex
 * planes of Py Px points, 3 K Px complex values, the tables (no device needed); same checks on H, W, K. */
int ics_img_psf_estimate(const ics_img *blurred, const ics_img *sharp, int y0, int y1, int x0, int x1, int K,
                         float regularisation, int coupling, float *raw /* K*K*3 */, double energy[3]);
int ics_img_psf_estimate_plan(int H, int W, int K, int *Py, int *Px, size_t *workspace_bytes);
/* Edge prediction on a device image (Cho and Lee 2009): the shock filter that turns the ramps of a blurred frame into steps, and the
 * choice of the gradients worth trusting, the same number for every orientation (csrc/ics_img_edges.hip; restated in
 * tests/edges_ref.py, whose float32 evaluation every route gives bit for bit: no FMA, IEEE square roots).
 * ics_img_shock: `iterations` steps of (Osher and Rudin; every read of a neighbour through coordinates clamped to the picture)
 *   Y   = ((R + G) + B) * float32(1 / 3) (coupling 1, vector; coupling 0, channel: Y = the channel itself, three times)
 *   Ys  = the binomial 1 2 1 along x, then along y, of Y: ((a[-1] + a[+1]) + (a[0] + a[0])) * 0.25
 *   s   = min(max((((Ys[x-1] + Ys[x+1]) + (Ys[y-1] + Ys[y+1])) - 4 Ys) * float32(1 / flat), -1), 1)
 *   g   = sqrt(m(u - u[x-1], u[x+1] - u)^2 + m(u - u[y-1], u[y+1] - u)^2),  m(p, q) = p q > 0 ? copysign(min(|p|, |q|), p) : 0
 *   out = u - (dt s) g                                        per channel u
 * route 1: a launch per step; 2: ICS_IMG_SHOCK_BLOCK steps per launch on LDS tiles; 0: the library's choice.  Queued like
 * the other image filters; src is not written.  ICS_EINVAL: iterations < 0, dt or flat not finite or flat <= 0, unknown coupling
 * or route.
 * ics_img_edge_mask: forward differences gx, gy per channel (0 in the last column / row);
 *   coupling 1: g = sqrt((q0 + q1) + q2), q_c = gx_c^2 + gy_c^2, sx = (gx0 + gx1) + gx2, sy likewise: one mask;
 *   coupling 0: g = sqrt(q_c), sx = gx_c, sy = gy_c: three independent masks;
 *   sector: none where g is not > 0; 0 where |sy| <= 0.41421357f |sx|; 2 where |sx| <= 0.41421357f |sy|; else 1 if sx sy > 0, else 3;
 *   t_b = the per_sector-th largest g of sector b, its smallest where it holds fewer; t = the smallest t_b of the sectors that hold
 *   any; mask = g >= t.  An exact radix select on the device, as in ics_img_noise_estimate.
 * *out: an ics_mask of H x W bytes per plane, one plane (coupling 1) or three (coupling 0), 0 or 1; threshold[c], kept[c]: t and the
 * pixels of the mask per plane (coupling 1: in all three slots).  route 1: every pass forms g from the frame; 2: the first pass stores
 * keys and sectors (4 + 1 bytes per pixel and plane, the bytes in the mask itself); 0: the library's choice.  The frame is taken to be
 * finite.  Like ics_img_noise_estimate it copies its results back and waits.  A plane that has no pixel with g > 0 has nothing to
 * select: its threshold comes back as NaN (the bits 0xFFFFFFFF), its mask all 0 and its count 0 -- the Python layer raises "no gradients
 * to select" on it.  ICS_EINVAL: a NULL pointer, per_sector < 1, unknown coupling or route. */
#define ICS_IMG_SHOCK_BLOCK 4
typedef struct ics_mask ics_mask;
int ics_img_shock(const ics_img *src, int iterations, float dt, float flat, int coupling, int route, ics_img **out);
int ics_img_edge_mask(const ics_img *src, unsigned per_sector, int coupling, int route, ics_mask **out, float threshold[3], unsigned kept[3]);
int ics_mask_create(ics_ctx *ctx, int H, int W, int planes /* 1 or 3 */, const unsigned char *host /* planes * H * W, 0 or 1 */, ics_mask **out);
int ics_mask_shape(const ics_mask *m, int *H, int *W, int *planes);
int ics_mask_download(const ics_mask *m, unsigned char *host /* planes * H * W */);
void ics_mask_destroy(ics_mask *m);
/* ics_img_psf_estimate with the sharp frame's derivatives multiplied by mask[y][x] before the taper (Cho and Lee's
 * argmin sum |M d p * k - d b|^2 + gamma |k|^2 around a predicted frame p): the energy S is summed over what remains, `blurred` is
 * untouched.  mask: of the frames' shape and context, one plane with coupling 1, three with coupling 0 (what ics_img_edge_mask makes
 * with the same coupling); the window applies to it as to the frames.  An all-ones mask gives the bits of ics_img_psf_estimate.
 * ICS_EINVAL: as ics_img_psf_estimate, and a NULL mask, one of another shape, context or number of planes. */
int ics_img_psf_estimate_masked(const ics_img *blurred, const ics_img *sharp, const ics_mask *mask, int y0, int y1, int x0, int x1, int K,
                                float regularisation, int coupling, float *raw /* K*K*3 */, double energy[3]);
/* Registration of two device images and the projective warp of one.  M, 3 x 3 row-major with M[8] = 1, takes a pixel (x, y, 1) of
 * `fixed` to the position (u, v) = (M0 . p, M1 . p) / (M2 . p) in `moving`.  ics_img_align finds it by coarse-to-fine Gauss-Newton on the
 * luma of both frames (forward-additive Lucas-Kanade, Levenberg's damping), with a gain a and a bias b where photometric != 0: the
 * residual is r = a I(M x) + b - T(x), T the luma of the box (y0, y1, x0, x1) of `fixed`, I that of all of `moving`.
 *   luma     Y = ((R + G) + B) * (1 / 3), smoothed by the binomial 1 2 1 each way inside the box / frame (the edge repeated), so that
 *            the bilinear sample and its central differences describe one surface on hard edges; pyramid level l + 1 = ((a + b) + (c + d)) * 0.25 of a 2 x 2 block, an odd last row or column
 *            dropped, pixel centres X = 2 (x + 0.5) - 0.5.  levels 0: halve while the smaller side of the next level of either plane
 *            stays >= 64, at most ICS_IMG_ALIGN_MAX_LEVELS; no level may be smaller than 16 px a side.
 *   model    0 translation (2 parameters), 1 affine (6), 2 homography (8); photometric adds a and b.
 *   a step   at a level: for every pixel of the fixed plane whose position (u, v) has 1 <= u < Wm - 2 and 1 <= v < Hm - 2, I and the
 *            central differences of I sampled bilinearly, the row J = a grad I . d(u, v)/dp (and I, 1), with the coordinates of both
 *            planes taken from their centres and divided by half their longer sides; S = sum J^T J, g = sum J^T r, sum r^2 and the
 *            count, float32 inside a 32 x 32 tile, double across the tiles, every sum in one order; (S + lambda diag S) d = -g by
 *            Cholesky in double on the host; lambda starts at 1e-6 at every level; a step that raises sum r^2 / count is rejected
 *            and lambda multiplied by 10, an accepted one divides it by 10.  A level ends when the largest motion of its four corners
 *            under a step is below `tolerance` px, or after `iterations` steps.
 * M: in the start, out the result; gain_bias: in the start (1, 0 for none), out the result (unchanged where photometric == 0, though
 * applied); stats: the rms of r at full resolution, count / pixels of the box, steps taken over all levels, levels used, the corner
 * motion in px of the last step at full resolution (one entry more than first planned: the line estimate_psf prints needs it).  Restated in
 * float64 in tests/align_ref.py.  Two runs give identical bits; neither frame is written; the frames may differ in shape; the call
 * waits for one read-back of at most 67 doubles per step.
 * ICS_EINVAL, before a frame is touched: a NULL pointer, model outside 0 .. 2, M not finite or singular, gain 0 or not finite, an empty
 * box or one with a negative corner, iterations < 1, tolerance not finite or <= 0, levels outside 0 .. ICS_IMG_ALIGN_MAX_LEVELS; then:
 * frames of different contexts, a box outside `fixed`, a level below 16 px; while it runs, with these words in ics_last_error: "not
 * finite: despeckle first" (a sum that is NaN or inf), "frames do not overlap enough" (count below a quarter of the plane at any step),
 * "no texture to align on" (the damped matrix is not positive definite).
 * ics_img_align_sums: one evaluation of the sums at full resolution for the given M, gain and bias: the upper triangle of S row-major,
 * g, sum r^2, the count -- n (n + 1) / 2 + n + 2 doubles for n parameters (`count` must say so), in the normalised coordinates above.
 * ics_img_warp: *out[y][x][c] = src sampled at M (x, y, 1), oh x ow pixels, by Keys' cubic convolution (a = -0.5) over 4 x 4 taps whose
 * coordinates are clamped to the frame; float32, every operation rounded once (tests/align_ref.py warp); an identity or an integer
 * shift copies finite pixels bit for bit.  ICS_EINVAL: a NULL pointer, M not finite or singular, oh or ow < 1.
 * ics_img_align_plan: the levels an H x W box against an H x W moving frame uses and the device bytes the call takes from the
 * context's pool (both pyramids, 67 floats a tile, the sums); no device needed; same checks on H, W, levels. */
#define ICS_IMG_ALIGN_MAX_LEVELS 8
int ics_img_align(const ics_img *moving, const ics_img *fixed, int y0, int y1, int x0, int x1, int model, int photometric, int levels,
                  int iterations, double tolerance, double M[9] /* in: start, out: result */, double gain_bias[2] /* in/out */,
                  double stats[5] /* rms, coverage, steps taken, levels used, last step px */);
int ics_img_align_sums(const ics_img *moving, const ics_img *fixed, int y0, int y1, int x0, int x1, int model, int photometric,
                       const double M[9], double gain, double bias, double *sums, int count);
int ics_img_warp(const ics_img *src, const double M[9], int oh, int ow, ics_img **out);
int ics_img_align_plan(int H, int W, int levels, int *used, size_t *workspace_bytes);
/* richardson_lucy_MM(image[iy:iy+M, ix:ix+N], u[uy:uy+uM, ux:ux+uN], psf, ...) with both windows taken from device
 * images (deconvolve.py:277-313 passes such views); psf is a host MK*MK*3 array as in ics_rl_upload. */
int ics_rl_upload_img(ics_rl *job, const ics_img *image, int iy, int ix, const ics_img *u, int uy, int ux, const float *psf);
/* The reference updates the caller's `u` view in place, border ring included (pyx:527-531): the whole u frame goes
 * back to dst[y:y+uM, x:x+uN]. */
int ics_rl_download_img(ics_rl *job, ics_img *dst, int y, int x);

/* ---- one image per GPU (BASELINE.json configs[4]) ------------------------------------------------
 * The reference has no multi-device code: every richardson_lucy_MM call (lib/deconvolution.pyx:341) is an independent
 * job, so N GPUs run N jobs, one process per GPU, and nothing is exchanged during the iterations.  The only collective
 * is the gather of a small per-rank record at the end -- RCCL over xGMI, called directly from this library (librccl.so
 * is dlopen'ed by ics_group_create when world > 1).  `rendezvous` is a file path shared by the ranks of the node: rank
 * 0 publishes the RCCL unique id there, the others wait up to `timeout_s` seconds for it.  With world == 1 every call
 * is a local no-op / copy and no device is touched.  count <= 49152 doubles per call (3 x 127^2 fits). */
typedef struct ics_group ics_group;
int ics_group_create(int device, int rank, int world, const char *rendezvous, int timeout_s, ics_group **out);
void ics_group_destroy(ics_group *g);
int ics_group_info(const ics_group *g, int *rank, int *world);
int ics_group_barrier(ics_group *g);
int ics_group_allreduce_max(ics_group *g, double *inout, int count);
int ics_group_allreduce_sum(ics_group *g, double *inout, int count); /* summed in rank order by RCCL (ncclSum, float64) */
/* How the group is connected: *backend = 0 local (world 1, no communicator), 1 RCCL; *nranks = ranks RCCL reports for the
 * communicator (ncclCommCount), lib = path or soname of the RCCL library in use ("" when local). */
int ics_group_describe(const ics_group *g, int *backend, int *nranks, char *lib, size_t lib_len);
int ics_group_allgather(ics_group *g, const double *send, int count, double *recv /* world * count */);
/* One image over several ranks (row bands, one process per GPU: lib/banded.py rank mode).  Rows [send_row0, + send_rows) of frame
 * buffer `which` of this rank's band job go to rank send_peer, rows [recv_row0, + recv_rows) arrive from rank recv_peer (a peer
 * < 0 switches that side off): RCCL point-to-point over xGMI between the two jobs' device frames, both directions in one group
 * call so that neighbours exchanging halos cannot deadlock.  Synchronous: returns when the rows are in place. */
int ics_rl_exchange_rows(ics_rl *job, ics_group *g, int which, int send_row0, int send_rows, int send_peer, int recv_row0, int recv_rows, int recv_peer);
/* The two per-iteration reductions of the row-band split, IN PLACE on the band job's device buffers and on the job's own stream -- one
 * RCCL call each, no host staging, no synchronisation (round 3 moved them through the host in chunks of 64 doubles):
 *   ics_rl_allreduce_keys   the six step-size keys of ICS_BUF_RED [0..5] (order-preserving uint32 keys: ncclMax on ncclUint32 is exact);
 *   ics_rl_allreduce_gradk  the 3 MK^2 PSF-gradient sums of ICS_BUF_GRADK: widened to float64 on the device, summed over the ranks
 *                           (ncclSum, float64), rounded to float32 once.
 * With a one-rank local group both return at once. */
int ics_rl_allreduce_keys(ics_rl *job, ics_group *g);
int ics_rl_allreduce_gradk(ics_rl *job, ics_group *g);

#ifdef __cplusplus
}
#endif
#endif /* ICS_HIP_H */
