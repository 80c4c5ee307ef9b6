// ics_kernels.h -- launchers of the non-convolution kernels (ics_kernels.hip, ics_stats.hip, ics_filters.hip).
#pragma once
#include "ics_common.h"

// ---- A5/A6/A8/A10 (lib/deconvolution.pyx:499-552): image update + DoF blend -------------------
struct IcsUpdateArgs {
  const float* u;      // frame origin of the current u
  float* u_out;        // frame that receives the updated u (== u for an in-place update)
  const float* ut;     // majoriser (pyx:462)
  const float* g;      // raw back-projection (A3)
  const float* f;      // image
  const float* tv;     // extended modes: T frame (NULL in the shipped mode)
  int tv_kind;         // 0 shipped, 1 active MM-TV, 2/3 PAM
  float* f_rw;         // active MM-TV: the image frame is updated in place (pyx:549)
  const uint32_t* red; // reduction keys of this inner iteration (ICS_RED_*)
  float* scal;         // device scalar block (ICS_SC_*): dt, maxu, maxg are recorded
  uint32_t* dofkeys;   // [0] = min key, [1] = max key, [2] = NaN flag (only when want_dof)
  float step, lambd;
  int blind;
  int want_dof;
  IcsGeom geo;
};
hipError_t ics_launch_update(const IcsUpdateArgs& a, hipStream_t s);

// ---- active MM-TV (build-defined extension, pyx:517/:543 made reachable): TV term of u against ut ---
struct IcsTvTermArgs {
  const float* u;      // frame origin
  const float* ut;     // majoriser
  const float* f;      // image (for max image_k, pyx:548)
  float* tv;           // T frame written
  uint32_t* red;       // ICS_RED_MAXT / ICS_RED_MAXF keys of this inner iteration
  float epsilon;       // 1e-2 blind / 1e-6 non-blind (pyx:434-437)
  int kind;            // 1 MM-TV term, 2 isotropic TV gradient, 3 collaborative L-inf,1,1 TV gradient
  IcsGeom geo;
  int planar = 0;      // kinds 2 / 3 only: u and tv are ORIGINS of channel-planar mirrors (ics_common.h), the transform-tile pipeline's frames
};
hipError_t ics_launch_tvterm(const IcsTvTermArgs& a, hipStream_t s);

// ---- A13 (pyx:567-571): PSF gradient, fp32 MFMA ------------------------------------------------
struct IcsGradkArgs {
  const float* e;   // residual frame origin (zero outside the M x N interior)
  const float* u;   // u frame origin
  float* partial;   // [nblocks][3][16nb][16nb] per-workgroup partial sums
  IcsGeom geo;
  int planar;       // matrix-core kernel only: e and u are ORIGINS of channel-planar mirrors (ics_common.h, the FFT-tile pipeline)
};
int ics_gradk_blocks(const IcsGeom& g, int cus);  // grid size (persistent workgroups)
hipError_t ics_launch_gradk(const IcsGradkArgs& a, int nblocks, hipStream_t s);
// matrix-core variant for PSF sizes <= 15 (ics_gradk_mfma.hip): fp16-split operands, same partial layout
bool ics_gradk_mfma_supported(int K);
hipError_t ics_launch_gradk_mfma(const IcsGradkArgs& a, int nblocks, hipStream_t s);
// ---- A11 + A13 fused (ics_synth_gradk_mfma.hip, PSF sizes <= 15): e' = conv(u, psf) - image never leaves the CU ---------
struct IcsFusedArgs {
  const float* u;     // u frame origin
  const float* f;     // image frame origin
  float* e_out;       // residual frame origin: e' is stored only where tiles meet the window below (or everywhere: store_all)
  const void* bt;     // weight table of the matrix-core convolution, conv orientation (ics_common.h)
  float* partial;     // [nblocks][3][16][16] per-workgroup partial sums (layout of k_gradk_mfma, reduced by k_gradk_reduce)
  int wy0, wy1, wx0, wx1;   // stats window (pyx:600-601,627) in u-frame coordinates
  int store_all;
  const float* facc;  // the image in accumulator order (ics_image_acc.h) in the layout of `rs`, or NULL: the epilogue reads the HWC frame
  int rs;             // tile height: 4 = 64-row tiles, two workgroups per CU (k_synth_gradk); 2 = 32-row tiles, three per CU (k_synth_gradk2)
  IcsGeom g;
};
bool ics_synth_gradk_supported(int K);
// tile height (IcsFusedArgs::rs) and grid size for this frame, from the persistent workgroups of the 64-row / 32-row form
void ics_synth_gradk_plan(const IcsGeom& g, int blocks64, int blocks32, int* rs, int* nblocks);
hipError_t ics_launch_synth_gradk(const IcsFusedArgs& a, int nblocks, hipStream_t s);
// gradk[a][b][c] = sum over workgroups (double accumulation, fixed order)
hipError_t ics_launch_gradk_reduce(const float* partial, int nblocks, float* gradk, const IcsGeom& g, hipStream_t s);
// one La x Lb tap block (partial blocks of 3 * nt * nt floats) into rows a0.., columns b0.. of a Kf x Kf gradient
hipError_t ics_launch_gradk_reduce_block(const float* partial, int nblocks, float* gradk, int nt, int La, int Lb, int Kf, int a0, int b0, hipStream_t s);

// ---- row bands: see include/ics_hip.h ICS_STAGE_BAND_* ----------------------------------------------
hipError_t ics_launch_band_reduce(const float* gr, const float* u, const float* ut, const IcsGeom& g, float lambd, int r0, int r1, uint32_t* red, hipStream_t s);
hipError_t ics_launch_band_mask_e(float* e, const IcsGeom& g, int i0, int i1, hipStream_t s);

// ---- channel-planar mirrors (ics_planar.hip) and the transform tiles (ics_fft_tile.h: ics_conv_fft.hip, ics_gradk_fft.hip) --------------------------------------------
// src / dst: buffer STARTS; rows [y0, y1), pixels [x0, x1) in u-frame coordinates (widened to 4-pixel groups), or the whole buffer
hipError_t ics_launch_planar_convert(bool to_planar, const float* src, float* dst, const IcsGeom& g, bool whole, int y0, int y1, int x0, int x1, hipStream_t s);
hipError_t ics_launch_update_planar(const IcsUpdateArgs& a, hipStream_t s);   // frame pointers = origins of planar mirrors
bool ics_conv_fft_supported(int K);
size_t ics_conv_fft_spectrum_floats();                                        // per orientation
// (blk_n > 0: the spectra of blk_n x blk_n tap blocks of blk_k x blk_k taps, block q at spec + q * ics_conv_fft_spectrum_floats())
hipError_t ics_launch_fft_spectrum(const float* psf, int K, float* spec_conv, float* spec_corr, hipStream_t s, int blk_n = 0, int blk_k = 0);
// PSF sizes above the single-tile range (87 ... 255): the convolutions and the PSF gradient as tap blocks on the tiles -- the blocks' products
// are summed in the frequency domain, one inverse transform per unit (k_conv_fft_blk); modes 0 and 1 of the shipped loop
bool ics_conv_fft_blk_supported(int K);
void ics_conv_fft_blk_shape(int K, int* blk_n, int* blk_k);
hipError_t ics_launch_conv_fft_blk(int mode, const IcsConvArgs& c, const float* spec, int blk_n, int blk_k, hipStream_t s);
hipError_t ics_launch_gradk_fft_blk(const float* u, const float* e, const IcsGeom& g, int blk_n, int blk_k, float* partial, float* gradk, hipStream_t s);
// modes 0 and 1 of ics_launch_conv on the transform tiles; every frame of `a` is the origin of a channel-planar mirror
hipError_t ics_launch_conv_fft(int mode, const IcsConvArgs& a, const float* spec, hipStream_t s);
// mode 2 (k_conv_fft<2>): A1 + A2 + A3 in ONE unit per tile pair -- interior tiles stay in the frequency domain between the two convolutions
// (one forward, one inverse transform; the image enters as the precomputed spectra of its windows), the tiles of the outer ring mask the
// residual in between.  Valid output 128 - 2 K + 2 pixels a side: for small PSFs.  The residual frame is NOT written.
hipError_t ics_launch_conv_fft_region(const IcsConvArgs& c, const float* spec, int oy0, int ox0, int oy1, int ox1, hipStream_t s);   // mode 0 over the tiles of a window
size_t ics_conv2_fft_fspec_floats(const IcsGeom& g);
bool ics_conv2_fft_supported(const IcsGeom& g);
hipError_t ics_launch_fft_image_spectrum(const float* f, const IcsGeom& g, float* fspec, hipStream_t s);
hipError_t ics_launch_conv2_fft(const IcsConvArgs& c, const float* spec_conv, const float* spec_corr, const float* fspec, hipStream_t s, uint32_t* wkeys = nullptr, uint32_t* gmax = nullptr);
// the operand-free form of mode 2 with the kernels beside it (ics_maxg_select.h; ics_conv_fft_sel.hip, ics_maxg_select.hip): the update pass that
// records, into one set `rec` of the ICS_MGS_* words, the key of max u_c and the bits of max |(u_new - ut)/2| per channel over the frame it
// writes (alias_next: the next majoriser is that frame, 0 recorded), and the selection kernel behind the launch
hipError_t ics_launch_update_planar_rec(const IcsUpdateArgs& a, uint32_t* rec, int alias_next, hipStream_t s);
struct IcsMaxgSelectArgs;
int ics_conv2_fft_units(const IcsGeom& g);                                          // work units of mode 2 on this geometry
void ics_conv2_fft_select_grid(const IcsGeom& g, IcsMaxgSelectArgs* m);             // fills the tile grid and the plane layout of *m
hipError_t ics_launch_maxg_select(const IcsMaxgSelectArgs& m, hipStream_t s);
// A12 + A13 on the same tiles (fp32): u, e = origins of planar mirrors; partial = ics_gradk_fft_blocks(cus) * K * K floats of scratch
int ics_gradk_fft_blocks(int cus);
hipError_t ics_launch_gradk_fft(const float* u, const float* e, const IcsGeom& g, float* partial, float* gradk, hipStream_t s);
// A11 + A12 + A13 as one unit per tile pair (three transforms instead of four; the residual stays in the tile buffer and is stored only for
// tiles under the window [wy0, wy1) x [wx0, wx1) of u-frame coordinates, or everywhere with store_all): bit-identical to
// ics_launch_conv_fft(0) followed by ics_launch_gradk_fft
hipError_t ics_launch_synth_gradk_fft(const float* u, const float* f, float* e, const float* spec, const IcsGeom& g, int wy0, int wy1, int wx0, int wx1, int store_all,
                                      float* partial, float* gradk, hipStream_t s);
// A14 ... A17 and both weight spectra in ONE launch (k_psf_spectra, ics_conv_fft.hip; PSF sizes the tiles take whole, <= 85): every one
// of the 96 workgroups of the spectrum launch steps a private copy of the PSF (ics_psf_step.h) and transforms its share of it; workgroup 0
// stores the results.  No workgroup waits for another, so the PSF is read from `psf` and written to `psf_next`: the caller exchanges
// the two afterwards.
struct IcsPsfSpectraArgs {
  const float* psf;     // [K][K][3] local psf before the step
  float* psf_next;      // ... and after it (another buffer)
  float* psf_caller;    // as IcsPsfArgs
  const float* gradk;   // [K][K][3]
  float* scal;          // ICS_SC_DTPSF recorded
  int* frozen;          // as IcsPsfArgs; read and written by workgroup 0 alone
  float* spec_conv;     // the two spectra (ics_launch_fft_spectrum)
  float* spec_corr;
  float step;
  int K, correlation;
};
hipError_t ics_launch_psf_spectra(const IcsPsfSpectraArgs& a, hipStream_t s);

// ---- zero-fill of up to ICS_ZERO_MAX device blocks in one launch (the ~24 buffers of a new job: one launch instead of 24 memsets) ----
#define ICS_ZERO_MAX 32
struct IcsZeroArgs {
  void* p[ICS_ZERO_MAX];                 // 16-byte aligned
  unsigned long long end16[ICS_ZERO_MAX]; // running total of 16-byte units up to and including block i
  int count;
};
hipError_t ics_launch_zero_many(const IcsZeroArgs& a, hipStream_t s);

// the small device state of a job at the start of ics_rl_run, in one launch (was five memsets and two host -> device copies)
struct IcsRunResetArgs {
  int* flags;          // [4]  := 0
  uint32_t* sched;     // [16] := 0
  double* dacc;        // [8]  := 0
  uint32_t* ukey;      // [2]  := 0
  uint32_t* red;       // [nred] := 0
  int nred;
  uint32_t* dofkeys;   // [8] := {0xFFFFFFFF, 0, 0, 0} x 2
  float* scal;         // [ICS_SC_COUNT] := 0 (a non-blind run writes no dtpsf: a reused job must not report the one of the blind run before it)
};
hipError_t ics_launch_run_reset(const IcsRunResetArgs& a, hipStream_t s);

// ---- A14-A17 (pyx:574-589) + weight packing ---------------------------------------------------
struct IcsPsfArgs {
  float* psf;          // [K][K][3] local psf (pyx: the name `psf` inside the function)
  const float* gradk;  // [K][K][3]
  float* wconv;        // [K+1][wrow] row-pair packed rot180(psf): weights of A1 (correlation orientation)
  float* wcorr;        // [K+1][wrow] row-pair packed psf:         weights of A3
  void* bt_conv;       // Toeplitz fragment tables of the matrix-core convolution (ics_common.h), or NULL
  void* bt_corr;
  float* psf_caller;   // what the caller's array holds (correlation quirk, pyx:585)
  float* work;         // PSF sizes above 63 only: 3*K*K floats of scratch (the kernel's working copy; LDS below that)
  float* scal;         // ICS_SC_DTPSF recorded
  int* frozen;         // device flag: caller array detached (pyx:585 rebinding)
  float step;
  int K, wrow;
  int correlation;
  int do_step;         // 0: only (re)pack the weights from psf
};
hipError_t ics_launch_psf(const IcsPsfArgs& a, hipStream_t s);
// PSF sizes 65 ... 127 (ics_big.hip): run-time-sized fp32 kernels; the convolution reads the PSF itself (rot180 for mode 0)
bool ics_big_supported(int K);
hipError_t ics_launch_conv_big(int mode, const IcsConvArgs& a, const float* psf, hipStream_t s);
hipError_t ics_launch_gradk_big(const IcsGradkArgs& a, int nblocks, hipStream_t s);
// tap blocks on the matrix cores (PSF sizes 51 ... 127, ics_big.hip): nblk x nblk weight tables of Kb x Kb taps, and the frame sum
hipError_t ics_launch_pack_blocks(const float* psf, int K, int Kb, int nblk, void* tconv, void* tcorr, size_t table_floats, hipStream_t s);
hipError_t ics_launch_frame_add(float* out, const float* add, int pitch, int y0, int y1, int f0, int f1, hipStream_t s);
hipError_t ics_launch_frame_neg(float* out, const float* in, size_t count, hipStream_t s);   // out = -in over a whole frame buffer

// ---- the inner iterations of an outer iteration as one cooperative launch, small frames (ics_small.hip) ------------------------------
// threads of a workgroup and outputs per thread and kernel row.  (1024 threads with 8 outputs -- all that fits 128 registers -- measured slower at
// every PSF size it was tried for, 3 ... 15: 255^2 / 15 blind 0.051 -> 0.063 ms per inner iteration; more LDS reads and partial sums per product)
constexpr int ics_small_threads(int K) { return 512; }
constexpr int ics_small_cw(int K) { return 16; }
#define ICS_SMALL_MAX_K 31
#define ICS_SMALL_LDS_BYTES 163840
#define ICS_SMALL_BAR_GROUPS 16
#define ICS_SMALL_BAR_WORDS (16 * ICS_SMALL_BAR_GROUPS)   /* 64-bit counters, one per 128 bytes: [16 g] = arrivals of the workgroups w with w % 16 == g */
struct IcsSmallPlan {
  int T, tiles_x, tiles_y, nwg;       // tile edge (32 / 64), tiles of the u-frame, workgroups = 3 x tiles
  int HU, pU, H1, pE, pT;             // LDS regions: U (T + 4 pad)^2 at pitch pU, E and F (T + 2 pad)^2 at pE, UT and G T^2 at pT (odd pitches)
  int chunks1, Cp1, AG1, AGn1;        // A1 on the tile +- pad: 16-column chunks, pitch of the partial sums, kernel rows per group, groups
  int chunksT, CpT, AGT, AGnT;        // A3 / A11 on the tile
  int YG, rpy;                        // A13: row groups of rpy rows
  int off_U, off_E, off_F, off_UT, off_G, off_P, off_W, off_PSF, lds_floats;
  uint32_t m_HU, m_H1, m_T, m_per1, m_perT, m_perG, m_YG;   // 2^32 / d + 1 of the divisors of the index arithmetic (ics_small.hip, udiv)
};
struct IcsSmallArgs {
  const float* u_in;        // u at the start of the outer iteration = its majoriser ut (pyx:462); read only
  float* u_out;             // receives u after every inner iteration
  const float* f;           // image
  float* e;                 // residual: the tile interiors of the last inner iteration (the stop test's operand)
  uint32_t* red;            // inner x ICS_RED_STRIDE keys: the maxima of every inner iteration are left here
  unsigned long long* keys; // inner x workgroups: every tile's max |gradu| (high word) and max u as order-preserving keys
  uint32_t* dofkeys;
  float* scal;
  float* psf; float* psf_caller; int* frozen;   // as IcsPsfArgs
  float* psf_bak;           // not NULL: psf and psf_caller as they are when the launch starts are copied here first (2 x 3 K^2)
  float* part;              // 3 x tiles x K^2: the tiles' shares of the PSF gradient
  float* gradk;             // [K][K][3]
  unsigned long long* bar;  // ICS_SMALL_BAR_WORDS counters, zeroed with the job's state
  unsigned long long bar_gen;   // barriers passed since then
  unsigned long long* trace;    // debug switch small_trace: 64 wall-clock stamps per workgroup, else NULL
  float step, lambd;
  int blind, correlation, inner;
  IcsSmallPlan plan;
  IcsGeom g;
};
// (64-pixel tiles -- frames up to ~570^2 -- are built but measured behind the multi-launch path: allow64 = debug switch small_iter = 2)
bool ics_small_plan(const IcsGeom& g, int cus, IcsSmallPlan* out, bool allow64 = false);
static inline int ics_small_barriers(int blind, int inner) { return blind ? 4 * inner : 2 * inner - 1; }
hipError_t ics_launch_small_iter(const IcsSmallArgs& a, hipStream_t s);

// ---- A18/A19 (pyx:593-638): window statistics and residual-whiteness metric -------------------
struct IcsStatsArgs {
  const float* e;      // residual frame origin
  const float* u;      // u frame origin
  float* scal;         // ICS_SC_MR / HU / VARU written
  uint32_t* dofkeys;   // DoF keys of the outer iteration (read; re-armed when `rearm`)
  uint32_t* red;       // reduction slots of the outer iteration's five inner iterations (8 * ICS_RED_STRIDE words), or nullptr
  int rearm;           // ics_rl_run: the kernel that writes the scalars also resets dofkeys and red for the next outer iteration
  double* dacc;        // 8 double accumulators (zeroed by the launcher)
  uint32_t* ukey;      // 2 keys (max |t|)
  float2* z;           // [3][P][P] complex scratch
  const float2* tw;    // [P/2] twiddles exp(-2 pi i k / P)
  const float* weights;// [H][W] Gaussian window (pyx:393-404)
  int top, bottom, left, right;
  int P, logP;
  int do_mr;
  IcsGeom geo;
  // long-line path (a window side above 4096 px, ics_stats.hip): Py x Px transform, z = [3][H][Px] + its transpose [3][Px][H] complex; Py = 0 selects the P x P path
  int Py, Px;
  const float2* twy;   // [Py] exp(-2 pi i m / Py)
  const float2* twx;   // [Px] exp(-2 pi i m / Px)
};
hipError_t ics_launch_stats(const IcsStatsArgs& a, hipStream_t s);
hipError_t ics_launch_hasnan(const float* u, const IcsGeom& g, int* flag, hipStream_t s);

// ---- standalone operators ----------------------------------------------------------------------
hipError_t ics_launch_normalize(float* kern, int K, hipStream_t s);   // [K][K][3] in place: negatives clamped, each channel divided by its sum
hipError_t ics_launch_tv(const float* u, int M, int N, float eps, int order, int norm, float* out, float* div, hipStream_t s);
// one LDS-tiled pass: out = conv2d_symm(src, kern); usm: out = src0 + (src0 - conv) * amount (lib/utils.py:275)
hipError_t ics_launch_conv2d_symm(const double* src, int H, int W, const double* kern, int KH, int KW, double* out,
                                  const double* src0, int usm, double amount, hipStream_t s);
// ws: (2 radius + 1)^2 spatial weights exp(-(i^2 + j^2) / (2 std_s^2)), j slow (the reference's offset order)
hipError_t ics_launch_bilateral(const double* src, int H, int W, int radius, double std_i, const double* ws, double* out, hipStream_t s);

// ---- bicubic resize between pyramid levels (ics_resize.hip; reference deconvolve.py:245-249) -------------
size_t ics_resize_scratch_doubles(int H, int W, int C);
hipError_t ics_launch_resize(double* src, int H, int W, int C, const double* wy, int ry, const double* wx, int rx, double* scratch,
                             double* out, int OH, int OW, hipStream_t s);
hipError_t ics_launch_resize_f32(const float* src, int H, int W, int C, const double* wy, int ry, const double* wx, int rx, double* scratch,
                                 float* out, int OH, int OW, hipStream_t s);   // float32 in / out, float64 inside

// ---- device-resident images (ics_img.hip; deconvolve.py:24-37, :100-103, :346-352) ----------------------
hipError_t ics_launch_img_pad_edge(const float* in, int H, int W, float* out, int top, int bottom, int left, int right, hipStream_t s);
hipError_t ics_launch_img_gamma(float* a, long n, float div, float exponent, float mul, int clip01, hipStream_t s);
hipError_t ics_launch_f32_to_f64(const float* in, double* out, long n, hipStream_t s);
hipError_t ics_launch_int_to_f32(const void* in, int bytes_per_value, float* out, long n, hipStream_t s);   // uint8 / uint16 -> float32
hipError_t ics_launch_f64_to_f32(const double* in, float* out, long n, hipStream_t s);

// ---- lib/utils.py filters on device-resident images (ics_img_filters.hip): H x W x 3 float32, channels independent --------
// `wr`: the kernel reversed on both axes.  rows: KH x KW taps on a 16-row tile (KH = 1: row pass of a rank-1 kernel; KH > 1: the
// non-separable fallback); cols: KH x 1 taps on a 32-row tile.  usm: out = src0 + (src0 - conv) * amount.  *_lds: dynamic LDS
// bytes of one workgroup (the launch fails above 160 KB).
size_t ics_img_conv_rows_lds(int KH, int KW);
size_t ics_img_conv_cols_lds(int KH);
size_t ics_img_bilateral_lds(int radius);
hipError_t ics_launch_img_conv_rows(const float* src, int H, int W, const float* wr, int KH, int KW, float* out, const float* src0, int usm,
                                    float amount, hipStream_t s);
hipError_t ics_launch_img_conv_cols(const float* src, int H, int W, const float* wr, int KH, float* out, const float* src0, int usm, float amount,
                                    hipStream_t s);
// ki = -1 / (2 std_i^2); ws: (2 radius + 1)^2 float32 spatial weights, x offset slow
hipError_t ics_launch_img_bilateral(const float* src, int H, int W, int radius, float ki, const float* ws, float* out, hipStream_t s);

// ---- TV denoising of device-resident images (ics_img_tvdenoise.hip): Chambolle's dual iteration, tau = 1 / 8 ------------------
// q: up to two frame pairs (qx, qy) of H x W x 3 floats each, q[0..1] and q[2..3], as many as ics_img_tv_pairs says; route 1: a
// launch per iteration, 2: ICS_IMG_TV_BLOCK iterations per launch on an LDS tile; coupling 0: per channel, 1: one s per pixel.
#define ICS_IMG_TV_BLOCK 4      // (== include/ics_hip.h)
size_t ics_img_tv_block_lds();
int ics_img_tv_pairs(int iterations, int route);
hipError_t ics_launch_img_tv_denoise(const float* f, int H, int W, float weight, int iterations, int coupling, int route, float* const q[4],
                                     float* out, hipStream_t s);

// ---- wavelet equaliser of device-resident images (ics_img_wavelet.hip): B3-spline a-trous scales, shrunk, weighted, summed --------
// route 1: a launch per scale; 2: the first ICS_IMG_WAVELET_FUSED scales in one launch on an LDS tile, the rest as in route 1.
// tmp: as many H x W x 3 frames as ics_img_wavelet_frames says (c_j ping-pong); the accumulator lives in `out`.  thresholds may be
// nullptr (all 0); coupling 0: per channel, 1: one magnitude per pixel.
#define ICS_IMG_WAVELET_MAX_SCALES 8      // (== include/ics_hip.h)
#define ICS_IMG_WAVELET_FUSED 3           // (== include/ics_hip.h)
size_t ics_img_wavelet_fused_lds();
int ics_img_wavelet_frames(int scales, int route);
hipError_t ics_launch_img_wavelet(const float* f, int H, int W, int scales, const float* gains, const float* thresholds, float residual,
                                  int coupling, int route, float* const tmp[2], float* out, hipStream_t s);

// ---- noise estimate of device-resident images (ics_img_noise.hip): the exact lower median of the finest starlet detail scale ------
// A radix select in three histogram passes with a one-workgroup select between them, no host round trip.  blk:
// ics_img_noise_block_words words (histograms and state; zeroed by the launcher); afterwards the words from
// ics_img_noise_result_word on hold the medians' bit patterns, three ("channel") or one ("vector").  route 1: every pass recomputes
// the detail from the frame, keys unused; 2: the first pass writes the keys (ics_img_noise_key_words words), the later ones read them.
// cus: compute units of the device (the persistent grids are sized by it and capped by the max_wgs switch).  f is only read.
size_t ics_img_noise_block_words();
size_t ics_img_noise_result_word();
size_t ics_img_noise_key_words(int H, int W, int coupling, int route);
size_t ics_img_noise_keys_lds(int coupling);
hipError_t ics_launch_img_noise(const float* f, int H, int W, int coupling, int route, int cus, unsigned* blk, unsigned* keys, hipStream_t s);

// ---- edge prediction on device-resident images (ics_img_edges.hip): the shock filter and the orientation-balanced gradient mask -----
// shock: tmp: ics_img_shock_frames frames of H W 3 floats the launches ping-pong through; route 1: a launch per step, 2:
// ICS_IMG_SHOCK_BLOCK steps per launch on LDS tiles.  edge mask: blk: ics_img_edge_block_words words (zeroed by the launcher), afterwards
// the words from ics_img_edge_result_word on hold three threshold bit patterns (0xFFFFFFFF: the plane has no gradients) and three counts;
// keys: ics_img_edge_key_words words (route 2); mask: H W bytes per plane, 1 ("vector") or 3 ("channel") planes.  src / f are only read.
// cus: compute units of the device (the persistent grids of the mask's kernels are sized by it and capped by the max_wgs switch).
#define ICS_IMG_SHOCK_BLOCK 4   // (== include/ics_hip.h)
size_t ics_img_shock_block_lds();
int ics_img_shock_frames(int iterations, int route);
hipError_t ics_launch_img_shock(const float* src, int H, int W, int iterations, float dt, float inv_flat, int coupling, int route, float* const tmp[2],
                                float* out, hipStream_t s);
size_t ics_img_edge_block_words();
size_t ics_img_edge_result_word();
size_t ics_img_edge_key_words(int H, int W, int coupling, int route);
size_t ics_img_edge_hist_lds(int coupling);
hipError_t ics_launch_img_edge_mask(const float* f, int H, int W, unsigned per_sector, int coupling, int route, int cus, unsigned* blk, unsigned* keys,
                                    unsigned char* mask, hipStream_t s);

// ---- guided filter of device-resident images (ics_img_guided.hip): box means, a solve per pixel, base layer + detail * (src - base) --
// route 1: coefficients to the planar frame `coef` (ics_img_guided_coef_floats floats), then the output; 2: one launch, coefficients
// in LDS, radius <= ICS_IMG_GUIDED_FUSED_RADIUS, coef unused.  coupling 0: per channel, 1: the RGB pixel as the guide.
#define ICS_IMG_GUIDED_MAX_RADIUS 32      // (== include/ics_hip.h)
#define ICS_IMG_GUIDED_FUSED_RADIUS 8     // (== include/ics_hip.h)
size_t ics_img_guided_coef_floats(int H, int W, int coupling, int route);
hipError_t ics_launch_img_guided(const float* src, int H, int W, int radius, float eps, float detail, int coupling, int route, float* coef, float* out,
                                 hipStream_t s);

// ---- despeckle of device-resident images (ics_img_despeckle.hip): the median of the (2 radius + 1)^2 window by the integer order of the
// float bits, put in place of a value that is further than a threshold from it.  t: three thresholds (coupling 1 reads t[0]); cnt:
// three words, zeroed by the caller on the same stream (outside its kernel-time bracket), afterwards the replaced values per channel (coupling 0) or the replaced pixels in cnt[0]
// (coupling 1).  route 1: a lane reads its windows from the frame; 2: a workgroup stages its tile and halo in LDS.  src is only read.
#define ICS_IMG_DESPECKLE_MAX_RADIUS 2    // (== include/ics_hip.h)
hipError_t ics_launch_img_despeckle(const float* src, int H, int W, int radius, const float t[3], int coupling, int route, float* out, unsigned* cnt,
                                    hipStream_t s);

// ---- local Laplacian filter of device-resident images (ics_img_llf.hip): K remapped Gaussian pyramids, an interpolated Laplacian
// pyramid, collapsed.  pyr: ics_img_llf_pyramid_floats floats (K + 1 pyramids of levels 1 .. J), r0 / r1: ics_img_llf_collapse_floats
// floats each.  route 1: a reduce chain per sample; 2: one reduce launch per level for all samples, the frame read once.  coupling 0:
// per channel (three passes through the same buffers), 1: the luma Y carries the filter.
#define ICS_IMG_LLF_MAX_LEVELS 10         // (== include/ics_hip.h)
#define ICS_IMG_LLF_MAX_SAMPLES 16        // (== include/ics_hip.h)
size_t ics_img_llf_pyramid_floats(int H, int W, int levels, int samples);
size_t ics_img_llf_collapse_floats(int H, int W);
hipError_t ics_launch_img_llf(const float* src, int H, int W, float sigma, float detail, float edges, int levels, int samples, int coupling, int route,
                              float* pyr, float* r0, float* r1, float* out, hipStream_t s);

// ---- blur width of device-resident images (ics_img_blurwidth.hip): the autocorrelation of the luma's differences along x and y over
// the window [y0, y1) x [x0, x1), lags 0 .. L <= ICS_IMG_BLURWIDTH_MAX_LAG.  partial: ics_img_blurwidth_partial_floats floats, every
// one written ([tile][axis][lag], float32 sums of one tile); result: 2 (L + 1) doubles, [axis][lag], the sums over the tiles in tile
// order divided by the pair counts (0 where there is no pair).  cus: compute units of the device (the persistent grid is sized by it
// and capped by the max_wgs switch).  One route; f is only read.
#define ICS_IMG_BLURWIDTH_MAX_LAG 128     // (== include/ics_hip.h)
size_t ics_img_blurwidth_lds(int L);
long ics_img_blurwidth_tiles(int hw, int ww);
size_t ics_img_blurwidth_partial_floats(int hw, int ww, int L);
hipError_t ics_launch_img_blurwidth(const float* f, int H, int W, int y0, int y1, int x0, int x1, int L, int cus, float* partial, double* result,
                                    hipStream_t s);

// ---- mask choice on device-resident images (ics_img_mask.hip): the box of `size` pixels a side inside the region [y0, y1) x [x0, x1) on
// which the blind phase should estimate the PSF: per 16 x 16 cell the structure tensor of the luma differences and the number of
// unusable pixels (a channel at or above clip, NaN, inf), per candidate box (origins on the 16-px grid) the smaller eigenvalue over its
// whole cells, then the arg-max.  ics_img_mask_candidates / ics_img_mask_cells: boxes and cells along one axis of that extent (0: the
// region is smaller than the box).  cells: 4 floats per cell, every one written; table: 3 doubles per candidate (score[], trace[],
// clipped[] as 64-bit integers), every one written; result: 5 doubles {i, j, score, trace, clipped}.  cus: compute units of the device
// (the persistent grid of the cell kernel is sized by it and capped by the max_wgs switch).  One route; f is only read.
#define ICS_IMG_MASK_CELL 16              // (== include/ics_hip.h)
size_t ics_img_mask_lds();
int ics_img_mask_candidates(int extent, int size);
int ics_img_mask_cells(int extent, int size);
hipError_t ics_launch_img_mask(const float* f, int H, int W, int y0, int y1, int x0, int x1, int size, float clip, int cus, float* cells, double* table, double* result,
                               hipStream_t s);

// ---- blur map of device-resident images (ics_img_blurmap.hip): per 16 x 16 cell of the window [y0, y1) x [x0, x1) the sums of A and
// A sigma and the number of the kept edge pixels (gradient ratio of the luma smoothed by sigma_a and sigma_b, include/ics_hip.h), one
// launch.  ics_img_blurmap_radius: ceilf(3.f * sigma); ics_img_blurmap_taps: the 2 r + 1 normalised taps of sigma; taps (device): those of
// sigma_a at [0], those of sigma_b at [2 ICS_IMG_BLURMAP_MAX_RADIUS + 1].  grid: ics_img_blurmap_grid workgroups (persistent, sized by
// the compute units and capped by the max_wgs switch); weight, moment, count: a value per cell, every one written; bad: an integer per
// workgroup, its pixels whose luma is not finite; sparse (or NULL): a float per pixel of the window.  One route; f is only read.
#define ICS_IMG_BLURMAP_CELL 16           // (== include/ics_hip.h)
#define ICS_IMG_BLURMAP_MAX_RADIUS 8      // (== include/ics_hip.h)
size_t ics_img_blurmap_lds(int r);
int ics_img_blurmap_radius(float sigma);
long ics_img_blurmap_tiles(int hw, int ww);
int ics_img_blurmap_grid(int hw, int ww, int cus);
void ics_img_blurmap_taps(float sigma, float* g);
hipError_t ics_launch_img_blurmap(const float* f, int H, int W, int y0, int y1, int x0, int x1, float sigma_a, float sigma_b, float edge, float max_sigma, int grid,
                                  const float* taps, float* weight, float* moment, int* count, int* bad, float* sparse, hipStream_t s);

// ---- Wiener deconvolution of device-resident images (ics_img_wiener.hip): one 2-D transform of the periodically extended frame, the
// filter conj(Hc) / (|Hc|^2 + balance L^2) per channel, the inverse.  ics_img_wiener_sizes: the transform sizes (powers of two >=
// H + K - 1, W + K - 1), 0 where one would be above ICS_IMG_WIENER_MAX.  A, B: ics_img_wiener_frame_bytes each; tables: the block of
// IcsWnTables, its psf holding the PSF as [3][K][K] (every channel of sum 1) before the launch.  ics_img_wiener_lds: dynamic LDS of a
// line kernel at P points.  One route; f is only read.
#define ICS_IMG_WIENER_MAX 8192           // (== include/ics_hip.h)
int ics_img_wiener_sizes(int H, int W, int K, int* Py, int* Px);
size_t ics_img_wiener_frame_bytes(int Py, int Px);
size_t ics_img_wiener_lds(int P);
hipError_t ics_launch_img_wiener(const float* f, int H, int W, int K, float balance, int Py, int Px, float2* A, float2* B, void* tables, float* out,
                                 hipStream_t s);
// the small block of the operators that take a PSF: Hr (the transformed rows of the PSF, 3 K Px float2), the twiddles of the two axes
// (Py and Px float2, a few unused), 4 sin^2 along y and x, the planar PSF.  block == nullptr: the size alone
struct IcsWnTables {
  float2 *Hr = nullptr, *twy = nullptr, *twx = nullptr;
  float *lamy = nullptr, *lamx = nullptr, *psf = nullptr;
  size_t bytes;
  IcsWnTables(void* block, int K, int Py, int Px) {
    bytes = ((size_t)3 * K * Px + Py + Px) * sizeof(float2) + ((size_t)Py + Px + (size_t)3 * K * K) * sizeof(float);
    if (!block) return;
    Hr = reinterpret_cast<float2*>(block); twy = Hr + (size_t)3 * K * Px; twx = twy + Py;
    lamy = reinterpret_cast<float*>(twx + Px); lamx = lamy + Py; psf = lamx + Px;
  }
};
// the passes its kernels do for the other units on this transform: the twiddle tables of the two axes with 4 sin^2 along y and x; the
// tiled transpose in[plane][R][C] -> out[plane][C][R] of three planes for the columns below clim; the K non-zero rows of the rolled PSF
// (planar, [3][K][K]) transformed -> Hr[c][r][:]; and the rows A[c][y][:], y < rows, inverse, the real part of their first n points ->
// dst[c * chan + y * pitch + j * step]
void ics_launch_img_wiener_tables(float2* twy, float2* twx, float* lamy, float* lamx, int Py, int Px, hipStream_t s);
void ics_launch_img_wiener_transpose(const float2* in, int R, int C, int clim, float2* out, hipStream_t s);
hipError_t ics_launch_img_wiener_psf_rows(const float* psf, int K, int Px, const float2* twx, float2* Hr, hipStream_t s);
hipError_t ics_launch_img_wiener_inv_rows(const float2* A, int rows, int Py, int Px, const float2* twx, float* dst, long chan, long pitch, int step, int n, hipStream_t s);

// ---- TV-regularised deconvolution of device-resident images (ics_img_tvdeconv.hip): split-Bregman iterations on the transform of
// ics_img_wiener.hip (its sizes, its extension, its tables), a shrinkage of the gradient per pixel and a solve that is diagonal under
// the transform.  workspace: ics_img_tvd_workspace_bytes, one block; ics_img_tvd_tables: the block of IcsWnTables inside it, its psf
// holding the PSF as [3][K][K] (every channel of sum 1) before the launch.
// coupling: 0 every channel by its own gradient magnitude, 1 the three by their common one.  One route; f is only read.
size_t ics_img_tvd_workspace_bytes(int K, int Py, int Px);
void* ics_img_tvd_tables(void* workspace, int Py, int Px);
hipError_t ics_launch_img_tv_deconvolve(const float* f, int H, int W, int K, float mu, float beta, int iterations, int coupling, int Py, int Px, void* workspace, float* out,
                                        hipStream_t s);
// its shrink pass, for ics_img_tvmdeconv.hip too: u, bx0, by0 -> bx1, by1, z on three Py x Px planes.  halves false: u and z planes
// [3][Py][Px]; true: u[c][y][:] the first and z[c][y][:] the second Px floats of row y of channel c of a spectrum frame (z = u + Px); the
// b planes contiguous
void ics_launch_img_tvd_shrink(int coupling, bool halves, const float* u, float* z, const float* bx0, const float* by0, float* bx1, float* by1, int Py, int Px, float thr,
                               hipStream_t s);

// ---- TV deconvolution with a masked data term (ics_img_tvmdeconv.hip): the iterations of ics_img_tvdeconv.hip with the extension of the
// frame, clipped and non-finite pixels and the caller's zeros declared unobserved, one more splitting variable keeping the solve
// diagonal.  workspace: ics_img_tvm_workspace_bytes, one block; ics_img_tvm_tables: the block of IcsWnTables inside it, its psf holding
// the PSF as [3][K][K] (every channel of sum 1) before the launch;
// ics_img_tvm_mask_slot: H W bytes of the caller's mask before the launch where observed is true; ics_img_tvm_total: the count of
// unobserved frame pixels after it.  clip: +inf for none.  coupling as above.  One route; f is only read.
size_t ics_img_tvm_workspace_bytes(int K, int Py, int Px);
void* ics_img_tvm_tables(void* workspace, int Py, int Px);
long long* ics_img_tvm_total(void* workspace, int Py, int Px);
unsigned char* ics_img_tvm_mask_slot(void* workspace, int K, int Py, int Px);
hipError_t ics_launch_img_tv_deconvolve_masked(const float* f, int H, int W, int K, bool observed, float clip, float mu, float beta, float gamma, int iterations, int coupling,
                                               int Py, int Px, void* workspace, float* out, hipStream_t s);

// ---- PSF from a sharp / blurred pair of device-resident images (ics_img_psfest.hip): the tapered derivatives of the two H x W windows
// through one transform of the sizes of ics_img_wiener.hip, the cross-spectrum solve, the K x K crop of its inverse.  sharp, blurred:
// the first pixel of the window in each frame, `pitch` floats a frame row.  workspace: ics_img_pe_workspace_bytes, one block;
// ics_img_pe_raw (3 K K floats, [i][j][c]) and ics_img_pe_energy (3 doubles) inside it hold the results after the launch.  coupling: 0 a
// PSF per channel, 1 one from the three.  One route; the frames are only read.
size_t ics_img_pe_workspace_bytes(int H, int W, int K, int Py, int Px);
float* ics_img_pe_raw(void* workspace, int H, int W, int K, int Py, int Px);
double* ics_img_pe_energy(void* workspace, int H, int W, int K, int Py, int Px);
hipError_t ics_launch_img_psf_estimate(const float* sharp, const float* blurred, long pitch, int H, int W, int K, float regularisation, int coupling, int Py, int Px,
                                       void* workspace, hipStream_t s);
// ... with the rows of the six planes formed by the caller's kernel: `rows` gets what k_img_pe_rows gets (tables already queued on s) and
// has to write every row of Za ([6][Py][Px], rows H .. Py - 1 zero) and every slot ([6][H], the row's sum of the sharp derivative's
// squares); grid (6, Py) of `lanes` lanes with `lds` bytes at launch is k_img_pe_rows's shape.  rows == nullptr: k_img_pe_rows.
// ics_launch_img_psf_estimate_masked (ics_img_edges.hip): the sharp frame's derivatives multiplied by mask[y][x] before the taper;
// mask: the window's first byte of the plane of channel 0, `mask_pitch` bytes a row, `mask_plane` bytes from a channel's plane to the
// next (0: one plane for all).
struct IcsPeRows {
  const float *sharp, *blurred; long pitch; int H, W, Py, Px, logPx;
  const float2* twx; const float *wy, *wx; float2* Za; float* slot; int lanes; size_t lds;
};
typedef hipError_t (*ics_pe_rows_fn)(const IcsPeRows& r, void* user, hipStream_t s);
hipError_t ics_launch_img_psf_estimate_rows(ics_pe_rows_fn rows, void* user, const float* sharp, const float* blurred, long pitch, int H, int W, int K,
                                            float regularisation, int coupling, int Py, int Px, void* workspace, hipStream_t s);
hipError_t ics_launch_img_psf_estimate_masked(const float* sharp, const float* blurred, long pitch, const unsigned char* mask, long mask_pitch, long mask_plane,
                                              int H, int W, int K, float regularisation, int coupling, int Py, int Px, void* workspace, hipStream_t s);

// ---- registration and warp of device-resident images (ics_img_align.hip): the luma plane of a window of an HWC frame (`pitch` floats a
// frame row), its 2 x 2 mean, one evaluation of the Gauss-Newton sums of a fixed plane T (H x W) against a moving plane I (Hm x Wm), and
// the projective warp of a frame.  model 0 translation, 1 affine, 2 homography; A: the 3 x 3 matrix between the planes' own frames
// (coordinates from the centre, divided by half the longer side).  slots: ics_img_al_tiles(H, W) * ics_img_al_slot_floats floats; out:
// that many doubles -- the upper triangle of J^T J row-major, J^T r, sum r^2, the count.  The planes and frames are only read.
int ics_img_al_params(int model, int photometric);
int ics_img_al_slot_floats(int model, int photometric);
long ics_img_al_tiles(int H, int W);
hipError_t ics_launch_img_al_luma(const float* f, long pitch, int H, int W, float* out, hipStream_t s);
hipError_t ics_launch_img_al_half(const float* in, int H, int W, float* out, hipStream_t s);
hipError_t ics_launch_img_al_sums(const float* T, int H, int W, const float* I, int Hm, int Wm, int model, int photometric, const double A[9], double gain, double bias,
                                  float* slots, double* out, hipStream_t s);
hipError_t ics_launch_img_al_warp(const float* src, int H, int W, const double M[9], float* out, int oh, int ow, hipStream_t s);
