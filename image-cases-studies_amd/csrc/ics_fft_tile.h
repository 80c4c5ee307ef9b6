// ics_fft_tile.h -- the PSF convolutions of one Richardson-Lucy inner iteration as LDS-resident overlap-save FFT tiles, gfx950: what every
// tile kernel shares (constants, buffer access, arguments, unit decode, loads, stages A-G, epilogues, the launch helper).  The kernels:
//   ics_conv_fft.hip      k_conv_fft<0|1|2, TV>, k_conv_fft_blk<0|1> (tap blocks, PSF sizes above ICS_FFT_MAX_K), k_fft_image_spectrum,
//                         k_fft_spectrum; ics_conv_fft_fill_args and the convolutions' launchers
//   ics_conv_fft_sel.hip  k_conv_fft<3, false>: mode 2 without the epilogue's operands (ics_maxg_select.h), compiled from ics_conv_fft.hip in a unit of its own
//   ics_gradk_fft.hip     k_gradk_fft, k_synth_gradk_fft, k_gradk_fft_reduce[_blk] and their launchers
//   (k_conv_fft_blk stays in the unit of k_conv_fft: compiled in a unit of its own, both families came out with other registers and
//    another instruction order -- the optimiser's result for a kernel depends on which other kernels share its module)
//   ics_fft_math.h        complex products, fft4 / fft8 / fft16, tw128
//   tools/bench_conv_fft.hip   includes both units; `emulate` is the host pass of the stage functions below (`make check-fft-emulate`)
//
//   mode 0 (A1+A2 / A11, lib/deconvolution.pyx:477-488, 555-565):  error = convolve(u, psf, "valid") - image
//   mode 1 (A3, pyx:490-491):  gradu = convolve(error, rot180(psf), "full")  (+ the reductions of A7, pyx:523-524)
//   mode 2 (A1+A2+A3 in one unit, round 6):  gradu straight from u and the image -- interior tiles never leave the frequency domain,
//                                             G = S1 (16384 S0 T - F) with F = the image windows' spectra (k_fft_image_spectrum); see tile_is_border.
//                                             Its tiles are 128 - 2 K + 2 pixels a side and cover the whole u-frame; the last tile of an axis also stores
//                                             the up to 2 pad rows / columns of the pad ring behind it where that saves a tile row / column (tile_rows;
//                                             4096^2 / 15: 41 x 41 tiles instead of 42 x 42, 2523 units = ten rounds on 256 workgroups instead of eleven)
//   k_synth_gradk_fft (A11+A12+A13 in one unit, round 6), k_gradk_fft (A12+A13), k_fft_spectrum (the weight spectra): see their units
//
// The reference computes both with scipy's complex64 FFT over the whole frame (pyx:478,491 -> scipy.signal.fftconvolve); here the frame is
// cut into tiles of V = 128 - K + 1 output pixels a side, each the valid part of a 128 x 128 circular correlation (overlap-save), fp32
// throughout.  The matrix-core kernels (ics_conv_mfma.hip) pay 3 split terms x 47..65 % Toeplitz fill -- at 31 x 31 a fifth of their
// MFMA flops is useful and the pass takes 0.9-1.0 ms at 6144^2; a 128 x 128 transform pair costs ~130 flop per output value whatever K is.
//
// In u-frame coordinates (ics_common.h) both modes are  out[y, x, c] = sum_{a,b<K} W[a, b, c] in[y + a - pad, x + b - pad, c]
// (W = rot180(psf) for mode 0, psf for mode 1).  With t = the 128 x 128 window of `in` that starts at (oy - pad, ox - pad),
//     out[oy + v, ox + h] = r[v][h],   r = IDFT( conj(DFT(W)) . DFT(t) ),   valid for v, h < V   (no wrap-around reaches them),
// and S = conj(DFT2(W zero-padded)) / 128^2 is built once per PSF by k_fft_spectrum.
//
// Work unit = (a PAIR of horizontally adjacent tiles, one channel): the two real tiles travel as real and imaginary part of one complex
// tile -- W is real, so IDFT(S . DFT(a + i b)) = corr(a) + i corr(b) with no separation step.  One 1024-thread workgroup per CU holds the
// complex tile in LDS (128 rows x 136 complex = 136 KB; pitch 272 dwords = 16 banks mod 64) and walks units n = r * grid + q, q chosen so that
// the three channel units of a tile pair run at the same time on three CUs of ONE XCD: the HWC lines a channel unit touches (4 of every
// 12 bytes) are the lines its two siblings touch, and they meet in that XCD's L2.
//
// 128 = 16 x 8 per dimension: n = j + 8 m, k = k1 + 16 k2,
//     X[k1 + 16 k2] = sum_j w8^(j k2) [ w128^(j k1) sum_m x[j + 8 m] w16^(m k1) ]            (forward; the inverse runs the same steps backwards)
// so a thread always holds 16 complex values: one radix-16 or two radix-8 transforms, and every exchange goes through LDS:
//   A  x-major (wave: j = w & 7, 64 columns)   global -> radix-16 over m -> twiddle -> LDS row 16 j + k1          | barrier
//   B  x-major (k1 = (w & 7) + 8 s)            radix-8 over j  -> row k1 + 16 k2 (= ky)                            | barrier
//   C  row-owner (wave: 8 rows; j = lane & 7)  radix-16 over m (x = j + 8 m) -> twiddle -> column 8 k1 + (j + k1) % 8
//   D  row-owner (k1 = (lane & 7) + 8 s)       radix-8 over j -> kx = k1 + 16 k2; x S[ky][kx]; inverse radix-8 over k2 -> same slots
//   E  row-owner                               conj twiddle, inverse radix-16 over k1 -> x = j + 8 m              | barrier
//   F  x-major                                 inverse radix-8 over k2 (rows k1 + 16 k2) -> row 16 j + k1         | barrier
//   G  x-major                                 conj twiddle, inverse radix-16 -> y = j + 8 m; epilogue straight from the registers
// C, D, E exchange data inside a wave's own 8 rows only (a wave's LDS operations execute in order): four workgroup barriers per unit.
// The column skew (j + k1) % 8 and the 16-bank pitch make every ds_read_b64 / ds_write_b64 of C, D, E conflict-free.
//
// Epilogues: the arithmetic of ics_conv.hip (mode 0: minus image on the M x N interior; mode 1: raw sums stored, maxima of
// |lambd g + (u - ut)/2| and u per channel; PAM kinds store G = T + lambd g).  Not bit-identical to the direct-sum kernels (an FFT
// rounds differently): held to the same float64 stage gates (tests/test_gpu_stages.py) and run-level goldens.
#pragma once
#include "ics_common.h"
#include "ics_kernels.h"
#include "ics_fft_math.h"
#include "ics_update.h"
#include <algorithm>
#include <cassert>

#define ICS_FFT_P 128
// largest PSF size ONE tile takes (44 valid pixels a side); above it the PSF is cut into tap blocks (k_conv_fft_blk), which measured ahead
// from about there: 4096^2 non-blind 85 one tile 1.68 ms, 97 one tile 2.85, 99 as 2 x 2 blocks 1.59
constexpr int ICS_FFT_MAX_K = 85;
#define ICS_FFT_PITCH 136
#define ICS_FFT_TWS 17         /* the twiddle table behind the tile: T[j][k1] = w^(j k1), j < 8, k1 < 16, rows of 17 entries (34 dwords: the eight j of a
                                  wave's lanes fall into different banks), so that a lane's fifteen reads are ONE address + immediate offsets */
#define ICS_FFT_TW_ENTRIES (8 * ICS_FFT_TWS)
#define ICS_FFT_LDS_BYTES (ICS_FFT_P * ICS_FFT_PITCH * 8 + ICS_FFT_TW_ENTRIES * 8)   /* the tile + the twiddle table */
#define ICS_FFT_THREADS 1024

#if defined(__HIP_DEVICE_COMPILE__)
#define ICS_FFT_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else   /* host pass: the CPU emulation of tools/bench_conv_fft.hip (single roundings there too: ICS_FSUB etc. of ics_update.h) */
#define ICS_FFT_UNIFORM(x) (x)
#endif

namespace icsfft {

// Global memory goes through buffer addressing on the device (SGPR resource + 32-bit lane offset + SGPR offset): with flat 64-bit pointers
// the compiler keeps one 64-bit VGPR address per access alive across the unit loop and spills them, and every access costs vector
// instructions for its address.  Here an access is  base + 4 * (lane index) + 4 * (wave-uniform index)  with the uniform part in a scalar
// register: the row walk of a tile costs no vector instruction at all.  Indices count floats from the START of the frame buffer (origin
// offset added: the apron in front of the origin has negative coordinates).
// Lane index ICS_FFT_NONE = "no access": its byte offset 2^31 lies beyond num_records, the hardware returns 0 for the load and drops the
// store.  Every access is issued unconditionally, so the number of memory operations in flight is static and the compiler's
// s_waitcnt vmcnt(n) for the register prefetch of the next unit does not degrade to vmcnt(0) behind the epilogue's stores.
// The host pass (CPU emulation, tools/bench_conv_fft.hip) indexes pointers.
#define ICS_FFT_NONE 0x20000000
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t gbuf;
__device__ __forceinline__ gbuf make_gbuf(const void* p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7FFFFFFF, 0x00020000); }
__device__ __forceinline__ float ld_f32(gbuf b, int vi, int si) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(b, 4 * vi, 4 * si, 0)); }
__device__ __forceinline__ void st_f32(gbuf b, int vi, int si, float v) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), b, 4 * vi, 4 * si, 0); }
__device__ __forceinline__ v2f ld_v2f(gbuf b, int vi, int si) { return __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(b, 8 * vi, 8 * si, 0)); }
template <int KIND = 0>   // (KIND: which class of access this is -- spectrum 1, operands 2 / 16, window 4)
__device__ __forceinline__ v4f ld_f32x4(gbuf b, int vi, int si) {
  return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(b, 4 * vi, 4 * si, 0));
}
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
// (the s_nop behind the store, with the data registers as its operands: a buffer store of more than 8 bytes reads its data registers for a
//  few cycles after it issues, and a vector instruction that rewrites one of them right behind it changes what is stored.  The compiler's
//  hazard table inserts wait states for that -- except when the store has an SGPR offset, which it takes to be safe.  On MI355X it is
//  not: `buffer_store_dwordx4 v[50:53], v58, s[20:23], s29 offen` followed by `v_mov_b32 v50, v0` stored the new v50 on some lanes
//  (tools/bench_conv_fft.hip found it: the first pixel of the quads of lanes 12-15 of every row group but the first).  Keeping the data
//  alive across two wait states costs nothing here: eight stores per thread and unit)
__device__ __forceinline__ void st_f32x4(gbuf b, int vi, int si, v4f v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, v), b, 4 * vi, 4 * si, 0);
  asm volatile("s_nop 2" :: "v"(v) : "memory");
}
#else
typedef const void* gbuf;
static inline gbuf make_gbuf(const void* p) { return p; }
static inline float ld_f32(gbuf b, int vi, int si) { return vi >= ICS_FFT_NONE ? 0.f : static_cast<const float*>(b)[vi + si]; }
static inline void st_f32(gbuf b, int vi, int si, float v) { if (vi < ICS_FFT_NONE) const_cast<float*>(static_cast<const float*>(b))[vi + si] = v; }
static inline v2f ld_v2f(gbuf b, int vi, int si) { return static_cast<const v2f*>(b)[vi + si]; }
template <int KIND = 0>
static inline v4f ld_f32x4(gbuf b, int vi, int si) {
  if (vi >= ICS_FFT_NONE) return (v4f){0.f, 0.f, 0.f, 0.f};
  const float* p = static_cast<const float*>(b) + vi + si;
  return (v4f){p[0], p[1], p[2], p[3]};
}
static inline void st_f32x4(gbuf b, int vi, int si, v4f v) {
  if (vi >= ICS_FFT_NONE) return;
  float* p = const_cast<float*>(static_cast<const float*>(b)) + vi + si;
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
#endif
// where pixel (Y, X, c) of a channel-planar frame lives: index = org + Y * pitch + X + c * cmul  (ics_common.h: ics_ppitch, ics_plane_floats)
struct Lay { int org, pitch, cmul; };
struct Mem {
  gbuf in, out, f, u, ut, tv, spec, spec1, fspec;
  Lay lay;   // (the same geometry: all frames of a job are)
};

}  // namespace icsfft

// ---- arguments ---------------------------------------------------------------------------------------------------------------------------
struct IcsFftArgs {
  IcsConvArgs c;        // frames, operands, reduction slots, geometry (c.w / c.bt / c.facc / c.sched unused)
  const v2f* spec;      // [3][128][128]: conj(DFT2(W_c)) / 128^2 of this orientation (k_fft_spectrum)
  const v2f* spec1;     // mode 2 (k_conv_fft<2>: A1 + A3 in one unit): `spec` = the convolution orientation's, `spec1` = the correlation orientation's
  int V;                // valid output pixels per tile ROW: 128 - K + 1 rounded down to whole quads
  int Vy;               // valid output ROWS per tile = 128 - K + 1: rows need no rounding to quads, and two more rows per tile save a whole round of
                        // units at some sizes (6144^2 / 31 x 31 back-projection: 65 x 65 tiles -> 63 x 65 = exactly 24 units per CU instead of 24.8)
  int tiles_x, ntiles, nunits;
  int ext_y, ext_x;     // mode 2: the LAST tile row / column stores this many output rows / columns beyond its Vy / V, up to 2 pad -- the strip of the
                        // pad ring that would otherwise take a tile row / column of its own (tile_rows).  0 everywhere else
  unsigned long long tiles_x_magic;   // floor(2^32 / tiles_x) + 1 (33 bits for tiles_x = 1): the unit decode divides by a multiply
  int oy0, ox0, oy1, ox1;   // output region in u-frame coordinates (mode 0: the M x N interior; mode 1: the whole u-frame)
  int gx0;                  // first column of the tile grid: ox0 rounded down to a multiple of 4, so that every 16-byte access of a plane row
                            // is 16-byte aligned (measured on MI355X: a buffer_store_dwordx4 at 12 mod 16 bytes lost its first dword on
                            // some lanes); the pixels in front of ox0 are stored as zeros, like those behind ox1
  alignas(8) int wpad;      // a tile's window starts wpad pixels up and left of its first output pixel: pad (one convolution), 2 pad (mode 2, k_conv_fft<2>: two in a row)
                            // (alignas: four bytes stay free behind gx0.  The compiler pairs the scalar loads of neighbouring fields by offset and
                            //  alignment, and with wpad and everything behind it packed 8 bytes lower all eleven tile kernels came out with other
                            //  registers -- k_conv_fft<1, false> with 17 SGPR spills instead of 16, k_conv_fft<2, true> with 36 instead of 34)
  float* fspec;             // mode 2: DFT of the image windows of every unit, [unit][8][1024] quads in load_spectrum's order (k_fft_image_spectrum)
  int blk_n, blk_k;         // tap blocks (PSF sizes above ICS_FFT_MAX_K, k_conv_fft_blk / k_gradk_fft with a lag block): blk_n x blk_n blocks of blk_k x blk_k taps;
                            // the tiles' valid part follows the BLOCK size, 128 - blk_k + 1 pixels a side.  0 = the whole PSF in one tile
  int lag_y, lag_x;         // k_gradk_fft with tap blocks: the block of lags [lag_y, lag_y + blk_k) x [lag_x, lag_x + blk_k) this launch evaluates
  int rot;                  // the walk starts `rot` units into the unit list and wraps around (mode 2: so that the last, partial round of units is
                            // not the bottom tile row, whose units are the outer ring's four-transform ones).  Order only: results do not change
  int wy0, wy1, wx0, wx1;   // k_synth_gradk_fft: the stop-test window in u-frame coordinates -- the residual is stored to its frame for the tiles
  int store_all;            // that touch it (pyx:600-601, 627 read nothing else of it), or for every tile (single stage)
};

namespace icsfft {

struct Unit {
  int c;            // channel
  int oy[2], ox[2]; // u-frame coordinates of output pixel (0, 0) of the two tiles
  bool has[2];
};

ICS_FFT_HD Unit decode_unit(const IcsFftArgs& a, int n) {
  Unit u;
  const int pair = n / 3;
  u.c = n - 3 * pair;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ti = 2 * pair + t;
    u.has[t] = ti < a.ntiles;
    const int ty = (int)(((unsigned long long)(unsigned)ti * a.tiles_x_magic) >> 32), tx = ti - ty * a.tiles_x;   // ti / tiles_x (fill_args: exact for ti * tiles_x < 2^32; the magic is 2^32 + 1 for one tile column)
    u.oy[t] = a.oy0 + ty * a.Vy; u.ox[t] = a.gx0 + tx * a.V;
  }
  return u;
}

// Output rows / columns tile (oy, ox) stores: Vy x V, cut at the region's far edge -- and, mode 2, the last tile of an axis goes on for
// ext more.  Such a tile is one of the outer ring (oy + Vy >= M: fill_args), it takes both transform pairs with residual_window between
// them, and then the second pair's outputs Vy .. Vy + ext - 1 are as good as the first Vy: they read the residual at buffer rows up to
// Vy + ext - 1 + 2 pad <= 127 -- no wrap-around -- and what they read beyond row Vy + 2 pad, where the first pair's wrap-around begins, lies
// at u-frame rows >= oy + Vy + pad >= pad + M, outside the interior, where residual_window has written the zeros that belong there.
ICS_FFT_HD int tile_rows(const IcsFftArgs& a, int oy) {
  const int rem = a.oy1 - oy;
  return rem <= a.Vy + a.ext_y ? rem : a.Vy;
}
ICS_FFT_HD int tile_cols(const IcsFftArgs& a, int ox) {
  const int rem = a.ox1 - ox;
  return rem <= a.V + a.ext_x ? rem : a.V;
}
// (wave-uniform) a tile of the unit reaches beyond the output region's columns, or stops short of a quad's end: per-pixel column tests.
// (EXT = false, here and in quad_lane: the kernels whose geometry never has an extension keep the plain Vy x V forms and do not read ext --
//  they are at the end of their registers as it is)
template <bool EXT> ICS_FFT_HD bool unit_is_edge(const IcsFftArgs& a, const Unit& u) {
  if (EXT) return u.ox[0] < a.ox0 || tile_cols(a, u.ox[0]) != a.V || u.ox[1] < a.ox0 || tile_cols(a, u.ox[1]) != a.V;
  return u.ox[0] < a.ox0 || u.ox[0] + a.V > a.ox1 || u.ox[1] < a.ox0 || u.ox[1] + a.V > a.ox1;
}

// walk position k -> unit (positions beyond the list stay beyond it: their accesses are dropped)
ICS_FFT_HD int walk_unit(const IcsFftArgs& a, int k) {
  if (k >= a.nunits) return k;
  const int n = k + a.rot;
  return n < a.nunits ? n : n - a.nunits;
}
ICS_FFT_HD Lay make_lay(const IcsGeom& g) {
  Lay l;
  l.pitch = ics_ppitch(g); l.org = g.ay * l.pitch + g.ax; l.cmul = g.rows * l.pitch;
  return l;
}
// (mode = 0 / 1: only the frames that mode touches get a resource of their own -- scalar registers are short in this kernel; -1: all)
ICS_FFT_HD Mem make_mem(const IcsFftArgs& a, int mode = -1) {
  Mem m;
  const IcsGeom& g = a.c.g;
  m.lay = make_lay(g);
  m.in = make_gbuf(a.c.in - m.lay.org); m.out = make_gbuf(a.c.out - m.lay.org);
  m.f = mode == 1 ? m.in : make_gbuf(a.c.f - m.lay.org);
  m.u = (mode == 0 || mode == 2) ? m.in : make_gbuf(a.c.u - m.lay.org);    // (mode 2 convolves u itself: the window's frame is the operand frame)
  m.ut = mode == 0 ? m.in : make_gbuf(a.c.ut - m.lay.org);
  m.tv = (a.c.tv && mode != 0) ? make_gbuf(a.c.tv - m.lay.org) : m.in;
  m.spec = make_gbuf(a.spec);
  m.spec1 = (mode == 2 || mode == -1) ? make_gbuf(a.spec1) : m.spec;
  m.fspec = (mode == 2 || mode == -1) ? make_gbuf(a.fspec) : m.spec;
  return m;
}

// LDS reads are volatile: left alone, the compiler pairs them into ds_read2_b64 / ds_read2st64_b64, which take 8 LDS cycles per wave
// instruction where two ds_read_b64 take 2 + 2 (MI355X_MICROARCH: 128 vs 256 B/clk)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ v2f lds_ld(const v2f* p) {   // (the low half of a generic address inside the LDS aperture is the LDS address)
  typedef const volatile __attribute__((address_space(3))) v2f* lds_vp;
  return *(lds_vp)(uint32_t)(uintptr_t)p;
}
#else
static inline v2f lds_ld(const v2f* p) { return *p; }
#endif

// "everything requested above is issued before anything below": keeps the scheduler from sinking LDS reads next to their first use, which
// turns fifteen twiddle reads into fifteen serial LDS round trips (seen in the ISA of stage E: ds_read / s_waitcnt lgkmcnt(0) / multiply, x 15)
#if defined(__HIP_DEVICE_COMPILE__)
#define ICS_FFT_ISSUE_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define ICS_FFT_ISSUE_FENCE() do { } while (0)
#endif

// Thread mappings.  x-major (stages A, B, F, G): wave w -> selector w & 7, columns 64 (w >> 3) + lane.  Row-owner (C, D, E): wave w -> rows
// 8 w + (lane >> 3), selector lane & 7.  Row-quad (the unit's boundaries, 16-byte global accesses): rows (tid >> 5) + 32 i, i < 4, pixels
// 4 (tid & 31) .. + 3 -- a half-wave covers one 512-byte row segment.
#define ICS_FFT_AT(row, col) lds[(row) * ICS_FFT_PITCH + (col)]

// The window of a unit, requested one unit ahead into registers: tile t, row group i -> 4 consecutive pixels (one dwordx4; a wave64 memory
// instruction costs the texture addresser ~16 cycles whether it moves 4 or 16 bytes per lane: as single floats the 64 loads per thread of
// a unit took 20 k of its 37 k shader clocks).  Rows and pixels beyond the frame's value range read as 0: rows as dropped accesses, pixels
// through the apron's zeros (a quad that starts inside [.., uN + pad) ends inside the apron, ax >= pad + 3; quads beyond it are dropped).
// (dy, dx: the window starts that much further down / right -- the tap blocks of wide PSFs)
ICS_FFT_HD void load_window(const IcsFftArgs& a, const Mem& mem, const Unit& u, int tid, v4f (&pw)[2][4], int t0 = 0, int t1 = 2, int dy = 0, int dx = 0) {
  const int r0 = tid >> 5, xq = tid & 31;
  const int pad = a.wpad, pitch = mem.lay.pitch, ylast = a.c.g.uM + pad - 1, xlast = a.c.g.uN + pad - 1;
#pragma unroll
  for (int t = t0; t < t1; ++t) {
    const int X = u.ox[t] - pad + dx + 4 * xq, Y0 = u.oy[t] - pad + dy + r0;       // both >= -pad by construction
    const int vo = (u.has[t] && X <= xlast) ? mem.lay.org + Y0 * pitch + X + mem.lay.cmul * u.c : ICS_FFT_NONE;
#pragma unroll
    for (int i = 0; i < 4; ++i) pw[t][i] = ld_f32x4<4>(mem.in, (Y0 + 32 * i <= ylast) ? vo : ICS_FFT_NONE, 32 * i * pitch);
  }
}
// ... and its way into the tile buffer: z = tile 0 + i tile 1, natural [row][pixel] layout (two 16-byte LDS stores per row group)
ICS_FFT_HD void store_window(const v4f (&pw)[2][4], v2f* lds, int tid) {
  const int r0 = tid >> 5, xq = tid & 31;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v4f* wp = reinterpret_cast<v4f*>(lds + (r0 + 32 * i) * ICS_FFT_PITCH + 4 * xq);
    wp[0] = (v4f){pw[0][i].x, pw[1][i].x, pw[0][i].y, pw[1][i].y};
    wp[1] = (v4f){pw[0][i].z, pw[1][i].z, pw[0][i].w, pw[1][i].w};
  }
}

// A: column x, rows j + 8 m -> radix-16 over m -> twiddle (wave-uniform: scalar registers) -> k1 to row j + 8 k1 (the slots it read)
ICS_FFT_HD void stage_a(v2f* lds, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, j = w & 7, x = 64 * (w >> 3) + lane;
  v2f* cp = lds + j * ICS_FFT_PITCH + x;
  v2f v[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) v[m] = lds_ld(cp + 8 * m * ICS_FFT_PITCH);
  fft16<1>(v);
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) cp[8 * k1 * ICS_FFT_PITCH] = k1 ? cmul_s(v[k1], tw128(j * k1)) : v[k1];
}

// B: radix-8 over j at fixed k1 (rows j + 8 k1) -> k2 to row 8 k1 + k2: frequency ky = k1 + 16 k2 lives in row 8 k1 + k2 from here on
// (in place again: the row stages do not care which row holds which ky, stage D asks ky_of_row).  F = the inverse, the same slots.
template <int DIR> ICS_FFT_HD void stage_b(v2f* lds, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, x = 64 * (w >> 3) + lane;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    v2f* bp = lds + 8 * ((w & 7) + 8 * s) * ICS_FFT_PITCH + x;
    v2f v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = lds_ld(bp + i * ICS_FFT_PITCH);
    if (DIR > 0) fft8<1>(v); else fft8<-1>(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) bp[i * ICS_FFT_PITCH] = v[i];
  }
}
ICS_FFT_HD int ky_of_row(int row) { return (row >> 3) + 16 * (row & 7); }

ICS_FFT_HD int skew_col(int j, int k1) { return 8 * k1 + ((j + k1) & 7); }

// C: one row, x = j + 8 m -> radix-16 over m -> twiddle -> column 8 k1 + (j + k1) % 8
// (`rd` = `lds` on the device -- the lanes of a wave run in lock step, every read is back before the first write; the CPU emulation, which
//  runs the threads one after the other, passes a snapshot)
// (`twl` = the 128 twiddles in LDS behind the tile: the lane-dependent ones of C and E are read from there, all fifteen requested ahead of
//  the transform; the skewed columns are eight base addresses (j + s) % 8, s = k1 % 8, plus compile-time offsets)
template <int TWB = 8>   // twiddles requested TWB at a time (8: two halves; 4: the PSF-gradient kernel, which holds 64 registers of spectra beside this stage)
ICS_FFT_HD void stage_c(const v2f* rd, v2f* lds, const v2f* twl, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), j = lane & 7;
  v2f v[16], tw[TWB];
  const v2f* rp = rd + row * ICS_FFT_PITCH + j;
#pragma unroll
  for (int m = 0; m < 16; ++m) v[m] = lds_ld(rp + 8 * m);
  if (TWB == 8) {
#pragma unroll
    for (int k1 = 1; k1 < 8; ++k1) tw[k1] = lds_ld(twl + j * ICS_FFT_TWS + k1);
    ICS_FFT_ISSUE_FENCE();
  }
  fft16<1>(v);
  v2f* const rowp = lds + row * ICS_FFT_PITCH;
  if (TWB == 8) {      // the second eight twiddles are requested before the first eight products: those cover their round trip
    v2f tw2[8];
#pragma unroll
    for (int k1 = 8; k1 < 16; ++k1) tw2[k1 - 8] = lds_ld(twl + j * ICS_FFT_TWS + k1);
    ICS_FFT_ISSUE_FENCE();
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) rowp[8 * k1 + ((j + k1) & 7)] = k1 ? cmul(v[k1], tw[k1]) : v[k1];
#pragma unroll
    for (int k1 = 8; k1 < 16; ++k1) rowp[8 * k1 + ((j + k1) & 7)] = cmul(v[k1], tw2[k1 - 8]);
    return;
  }
#pragma unroll
  for (int h = 0; h < 16 / TWB; ++h) {
    if (TWB != 8 || h > 0) {
#pragma unroll
      for (int k1 = TWB * h; k1 < TWB * h + TWB; ++k1) if (k1) tw[k1 - TWB * h] = lds_ld(twl + j * ICS_FFT_TWS + k1);
    }
#pragma unroll
    for (int k1 = TWB * h; k1 < TWB * h + TWB; ++k1) rowp[8 * k1 + ((j + k1) & 7)] = k1 ? cmul(v[k1], tw[k1 - TWB * h]) : v[k1];
  }
}

// The spectrum values a thread multiplies by in stage D: row -> ky, kx = q + 8 s + 16 k2 (from L2: 384 KB for the three channels).  Requested
// in front of stage C: requested inside stage D, in two batches of eight with a wait each, the last wave left stage D 17 k shader clocks
// after the first (per-wave timeline).  (Requested a whole unit ahead -- in front of the
// previous unit's stores, which vmcnt makes every later load wait for -- they took stage D to 2 k clocks, but 32 registers alive across
// stages A-C spilled the window prefetch: measured slower.)
// Layout (k_fft_spectrum writes it): the sixteen values of a thread as eight 16-byte pairs, [channel][pair l = 4 s + k2 / 2][thread] -- a wave's
// load is 1 KiB contiguous, eight loads per thread instead of sixteen 8-byte ones (the texture addresser's time goes by instructions).
ICS_FFT_HD int spec_index(int c, int ky, int kx) {   // position of S_c[ky][kx] in v2f units
  const int tid = 64 * (ky & 15) + 8 * (ky >> 4) + (kx & 7), s = (kx >> 3) & 1, k2 = kx >> 4;
  return (((c * 8 + 4 * s + (k2 >> 1)) * ICS_FFT_THREADS + tid) * 2) + (k2 & 1);
}
ICS_FFT_HD void load_spectrum(const Mem& mem, int c, int tid, v2f (&sp)[2][8]) {
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const v4f p = ld_f32x4<1>(mem.spec, 4 * tid, (c * 8 + l) * ICS_FFT_THREADS * 4);
    sp[l >> 2][2 * (l & 3)] = (v2f){p.x, p.y};
    sp[l >> 2][2 * (l & 3) + 1] = (v2f){p.z, p.w};
  }
}
// one half (s = 0 / 1: the eight values of one pass of stage D) of a thread's sixteen spectrum values, from a buffer in load_spectrum's layout
// whose block of 8 x 1024 quads starts at quad index `blk` (a channel of the weight spectra, a unit of the image spectra)
template <int KIND>
ICS_FFT_HD void load_spectrum_half(gbuf b, int blk, int tid, int s, v2f (&sp)[8]) {
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const v4f p = ld_f32x4<KIND>(b, 4 * tid, (blk + 4 * s + l) * ICS_FFT_THREADS * 4);
    sp[2 * l] = (v2f){p.x, p.y};
    sp[2 * l + 1] = (v2f){p.z, p.w};
  }
}
// ... and the way out: a thread's sixteen values as block `blk` of such a buffer (k_fft_image_spectrum)
ICS_FFT_HD void store_spectrum(gbuf b, int blk, int tid, const v2f (&z)[2][8]) {
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const v2f z0 = z[l >> 2][2 * (l & 3)], z1 = z[l >> 2][2 * (l & 3) + 1];
    st_f32x4(b, 4 * tid, (blk + l) * ICS_FFT_THREADS * 4, (v4f){z0.x, z0.y, z1.x, z1.y});
  }
}
// Stage D of the fused A1 + A3 unit (mode 2, k_conv_fft<2>), interior tiles: with T = the window's spectrum (after the radix-8 pass),
//     G = S1 . (16384 S0 T - F),     F = the UNNORMALISED transform of the image window (k_fft_image_spectrum),
// i.e. the spectrum of corr(conv(u) - image): both weight spectra carry the 1 / 128^2 of an inverse transform, the first one's is undone
// (a power of two: exact).  One forward and one inverse transform where k_conv_fft<0> + k_conv_fft<1> run two of each.
ICS_FFT_HD void stage_d2_half(const v2f (&s0)[8], const v2f (&s1)[8], const v2f (&fs)[8], v2f* lds, int tid, int s) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
  v2f v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = lds_ld(lds + row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s);
  fft8<1>(v);
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) {
    const v2f st = cmul(v[k2], s0[k2]);
    const v2f x = __builtin_elementwise_fma(st, (v2f){16384.f, 16384.f}, -fs[k2]);
    v[k2] = cmul(x, s1[k2]);
  }
  fft8<-1>(v);
#pragma unroll
  for (int j = 0; j < 8; ++j) lds[row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s] = v[j];
}

// D: radix-8 over j -> kx = k1 + 16 k2, multiply by the spectrum, inverse radix-8 over k2 -> j, same slots
ICS_FFT_HD void stage_d(const v2f (&sp)[2][8], v2f* lds, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
  v2f* db[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) db[j] = lds + row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7);   // column 8 k1 + (j + k1) % 8 with k1 = q + 8 s: + 64 s
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    v2f v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lds_ld(db[j] + 64 * s);
    fft8<1>(v);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) v[k2] = cmul(v[k2], sp[s][k2]);
    fft8<-1>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) db[j][64 * s] = v[j];
  }
}

// The two halves of stage D on their own (PSF gradient, k_gradk_fft): the 2-D spectrum of the tile in the thread's registers -- sixteen
// values, the same (ky, kx) in the same slot for every tile -- and the way back from such a set of values.
ICS_FFT_HD void stage_d_forward(const v2f* lds, int tid, v2f (&z)[2][8]) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    v2f v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lds_ld(lds + row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s);
    fft8<1>(v);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) z[s][k2] = v[k2];
  }
}
ICS_FFT_HD void stage_d_inverse(const v2f (&z)[2][8], v2f* lds, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    v2f v[8];
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) v[k2] = z[s][k2];
    fft8<-1>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s] = v[j];
  }
}

// Stage D of the fused A11 + A13 unit (k_synth_gradk_fft).  First use: as stage_d, and the window's 2-D spectrum stays behind in `zu`
// (the same (ky, kx) in the same slot for every tile: stage_d_forward's layout).  Second use, on the residual tile: its spectrum goes
// straight into the workgroup's sum  acc += DFT(t) conj(DFT(e'))  -- eight values at a time, the residual's spectrum is never whole in registers.
ICS_FFT_HD void stage_d_keep(const v2f (&sp)[2][8], v2f* lds, int tid, v2f (&zu)[2][8]) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    v2f v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lds_ld(lds + row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s);
    fft8<1>(v);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) { zu[s][k2] = v[k2]; v[k2] = cmul(v[k2], sp[s][k2]); }
    fft8<-1>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s] = v[j];
  }
}
ICS_FFT_HD void stage_d_acc(const v2f* lds, int tid, const v2f (&zu)[2][8], v2f (&acc)[2][8]) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    v2f v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lds_ld(lds + row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s);
    fft8<1>(v);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) acc[s][k2] += cmulc(zu[s][k2], v[k2]);
  }
}

// Tap blocks (k_conv_fft_blk): the window's spectrum times the block's weight spectrum, added to the unit's sum -- the products of all
// blocks meet in the frequency domain and share one inverse transform (stage_d_inverse)
ICS_FFT_HD void stage_d_mac_half(const v2f* lds, int tid, int s, const v2f (&sp)[8], v2f (&acc)[8]) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), q = lane & 7;
  v2f v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = lds_ld(lds + row * ICS_FFT_PITCH + 8 * q + ((j + q) & 7) + 64 * s);
  fft8<1>(v);
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) acc[k2] += cmul(v[k2], sp[k2]);
}
ICS_FFT_HD void stage_d_mac(const v2f* lds, int tid, const v2f (&sp)[2][8], v2f (&acc)[2][8]) {
  stage_d_mac_half(lds, tid, 0, sp[0], acc[0]);
  stage_d_mac_half(lds, tid, 1, sp[1], acc[1]);
}

// E with its twiddles requested four at a time (the fused unit holds 64 registers of spectra beside this stage: as stage_c<4>)
ICS_FFT_HD void stage_e_lean(const v2f* rd, v2f* lds, const v2f* twl, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), j = lane & 7;
  v2f v[16];
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) v[k1] = lds_ld(rd + row * ICS_FFT_PITCH + ((j + k1) & 7) + 8 * k1);
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    v2f tw[4];
#pragma unroll
    for (int k1 = 4 * h; k1 < 4 * h + 4; ++k1) if (k1) tw[k1 - 4 * h] = lds_ld(twl + j * ICS_FFT_TWS + k1);
    ICS_FFT_ISSUE_FENCE();
#pragma unroll
    for (int k1 = 4 * h; k1 < 4 * h + 4; ++k1) if (k1) v[k1] = cmulc(v[k1], tw[k1 - 4 * h]);
  }
  fft16<-1>(v);
  v2f* wp = lds + row * ICS_FFT_PITCH + j;
#pragma unroll
  for (int m = 0; m < 16; ++m) wp[8 * m] = v[m];
}

// E: conj twiddle, inverse radix-16 over k1 -> x = j + 8 m
ICS_FFT_HD void stage_e(const v2f* rd, v2f* lds, const v2f* twl, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, row = 8 * w + (lane >> 3), j = lane & 7;
  v2f v[16], tw[16];
  const v2f* cb[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) cb[s] = rd + row * ICS_FFT_PITCH + ((j + s) & 7);
  // all fifteen twiddles and the sixteen values requested in one go (the scheduler otherwise sinks each twiddle read next to its product:
  // fifteen serial LDS round trips per wave in a stage every wave of the CU is in at the same time)
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) tw[k1] = lds_ld(twl + j * ICS_FFT_TWS + k1);
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) v[k1] = lds_ld(cb[k1 & 7] + 8 * k1);
  ICS_FFT_ISSUE_FENCE();
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) v[k1] = cmulc(v[k1], tw[k1]);
  fft16<-1>(v);
  v2f* wp = lds + row * ICS_FFT_PITCH + j;
#pragma unroll
  for (int m = 0; m < 16; ++m) wp[8 * m] = v[m];
}

// G: rows j + 8 k1 of column x -> conj twiddle, inverse radix-16 over k1 -> the finished values of rows j + 8 m, back into the slots they
// came from: the tile buffer now holds r (tile 0 in .x, tile 1 in .y) in natural [row][pixel] layout for the row-quad epilogue
ICS_FFT_HD void stage_g(v2f* lds, int tid) {
  const int w = ICS_FFT_UNIFORM(tid >> 6), lane = tid & 63, j = w & 7, x = 64 * (w >> 3) + lane;
  v2f* cp = lds + j * ICS_FFT_PITCH + x;
  v2f v[16];
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) v[k1] = lds_ld(cp + 8 * k1 * ICS_FFT_PITCH);
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) v[k1] = cmulc_s(v[k1], tw128(j * k1));
  fft16<-1>(v);
#pragma unroll
  for (int m = 0; m < 16; ++m) cp[8 * m * ICS_FFT_PITCH] = v[m];
}

// Epilogue (row-quad ownership): the arithmetic of ics_conv.hip on 4 consecutive pixels of a row at a time, operands and results as
// dwordx4.  On gfx9 vmcnt counts loads and stores alike and retires them in order: a load issued behind a store waits out the store's round
// trip to L2.  So within a unit every operand load is issued before the first store: mode 0 requests the image quads of both tiles before
// stage F; mode 1 walks its operands (u, ut[, T]) row group by row group, group i + 1 requested before the maxima of group i are taken, and
// stores the values it kept at the end.  A quad's lane address says "this row group of this tile is mine" or is a dropped access; pixels
// of a valid quad beyond the output region are stored as zeros (they land in the frame's border ring / slack, which holds zeros).
struct Ops { v4f a[2][4], b[2][4]; };   // [tile][row group].  mode 1: a = u, b = ut -- or, for the PAM kinds (TV kernel, tv_kind >= 2), b = the T frame
// The maxima of A6 / A7 over a unit's valid pixels, in a form that costs two or three vector operations per pixel and no lane masks:
//   ag  = max over pixels of (bits of g) & 0x7FFFFFFF as an unsigned integer: the bits of |g| order like |g| itself and every NaN lies above
//         +inf (0x7F800000), so one integer maximum carries both max |g| and "a NaN was seen";
//   mu  = float maximum of u (v_max_f32 drops NaNs), au = the same integer maximum of |u| bits, kept only for its NaN test;
//   any = a valid pixel was seen (row groups outside the tile / region contribute nothing).
struct Maxima { uint32_t ag, au, any; float mu; };
ICS_FFT_HD void maxima_init(Maxima& mx) { mx.ag = 0u; mx.au = 0u; mx.any = 0u; mx.mu = -__builtin_inff(); }
ICS_FFT_HD uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
// the unit's two keys (0 = nothing seen, canonical NaN key = largest: a NaN propagates like np.amax)
ICS_FFT_HD void maxima_keys(const Maxima& mx, uint32_t& kg, uint32_t& ku) {
  kg = mx.ag > 0x7F800000u ? 0xFFC00000u : (mx.any ? ics_f2key(__builtin_bit_cast(float, mx.ag)) : 0u);
  ku = mx.au > 0x7F800000u ? 0xFFC00000u : (mx.any ? ics_f2key(mx.mu) : 0u);
}

// lane address of row group 0 of tile t in frame layout L, or ICS_FFT_NONE; `rows` = number of this lane's row groups inside the tile (0..4)
template <bool EXT = false>
ICS_FFT_HD int quad_lane(const IcsFftArgs& a, const Unit& u, const Lay& L, int tid, int t, int& rows, int& X) {
  const int r0 = tid >> 5, xq = tid & 31;
  const int lim = EXT ? tile_rows(a, u.oy[t]) : (a.oy1 - u.oy[t] < a.Vy ? a.oy1 - u.oy[t] : a.Vy);      // output rows of this tile
  X = u.ox[t] + 4 * xq;
  const bool ok = EXT ? (u.has[t] && 4 * xq < tile_cols(a, u.ox[t]) && r0 < lim) : (u.has[t] && 4 * xq < a.V && X < a.ox1 && r0 < lim);
  rows = ok ? (lim - r0 + 31) >> 5 : 0;                                // row groups i with r0 + 32 i < lim
  return ok ? L.org + (u.oy[t] + r0) * L.pitch + X + L.cmul * u.c : ICS_FFT_NONE;
}

ICS_FFT_HD void load_image(const IcsFftArgs& a, const Mem& mem, const Unit& u, int tid, v4f (&f)[2][4], int t0 = 0, int t1 = 2) {
#pragma unroll
  for (int t = t0; t < t1; ++t) {
    int rows, X;
    const int vo = quad_lane(a, u, mem.lay, tid, t, rows, X);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[t][i] = ld_f32x4<2>(mem.f, i < rows ? vo : ICS_FFT_NONE, 32 * i * mem.lay.pitch);
  }
}
// (row groups [i0, i1) of both tiles only)
ICS_FFT_HD void load_image_rows(const IcsFftArgs& a, const Mem& mem, const Unit& u, int tid, v4f (&f)[2][4], int i0, int i1) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    int rows, X;
    const int vo = quad_lane(a, u, mem.lay, tid, t, rows, X);
#pragma unroll
    for (int i = i0; i < i1; ++i) f[t][i] = ld_f32x4<2>(mem.f, i < rows ? vo : ICS_FFT_NONE, 32 * i * mem.lay.pitch);
  }
}
// mode 1: the operands under tile t.  The PAM kinds (build-defined tv_mode 2 / 3; ics_conv.hip's epilogue for them) need u and the TV
// term T = -div(p) instead of u and ut: two operand frames either way (a third does not fit 128 registers).
template <bool TV, bool EXT = false>
ICS_FFT_HD void load_ops(const IcsFftArgs& a, const Mem& mem, const Unit& u, int tid, int t, Ops& o, int i0 = 0, int i1 = 4) {
  int rows, X;
  const int va = quad_lane<EXT>(a, u, mem.lay, tid, t, rows, X);
  const bool pam = TV && a.c.tv_kind >= 2;
#pragma unroll
  for (int i = i0; i < i1; ++i) {
    const int vo = i < rows ? va : ICS_FFT_NONE;
    if (t == 0) {
      o.a[t][i] = ld_f32x4<2>(mem.u, vo, 32 * i * mem.lay.pitch);
      o.b[t][i] = pam ? ld_f32x4<2>(mem.tv, vo, 32 * i * mem.lay.pitch) : ld_f32x4<2>(mem.ut, vo, 32 * i * mem.lay.pitch);
    } else {
      o.a[t][i] = ld_f32x4<16>(mem.u, vo, 32 * i * mem.lay.pitch);
      o.b[t][i] = pam ? ld_f32x4<16>(mem.tv, vo, 32 * i * mem.lay.pitch) : ld_f32x4<16>(mem.ut, vo, 32 * i * mem.lay.pitch);
    }
  }
}
// the finished values of row group i: r[t] = 4 pixels of tile t
ICS_FFT_HD void read_quads(const v2f* lds, int tid, int i, v4f (&r)[2]) {
  const int r0 = tid >> 5, xq = tid & 31;
  const v4f* rp = reinterpret_cast<const v4f*>(lds + (r0 + 32 * i) * ICS_FFT_PITCH + 4 * xq);
  const v4f z0 = rp[0], z1 = rp[1];
  r[0] = (v4f){z0.x, z0.z, z1.x, z1.z};
  r[1] = (v4f){z0.y, z0.w, z1.y, z1.w};
}
// mode 0 takes the lane address and the pixel masks of a tile ONCE per unit (as eight store_quad calls the address arithmetic of the
// epilogue was 300 of a unit's 1310 vector instructions); `edge` (wave-uniform) = the tile reaches beyond the output region's columns
struct QuadOut { int vo, rows, X; };
ICS_FFT_HD void store_quad_at(const IcsFftArgs& a, const Mem& mem, const QuadOut& q, bool edge, int i, v4f val) {
  if (edge) {
    const int X = q.X;
    val = (v4f){X >= a.ox0 ? val.x : 0.f, (X + 1 >= a.ox0 && X + 1 < a.ox1) ? val.y : 0.f, (X + 2 >= a.ox0 && X + 2 < a.ox1) ? val.z : 0.f, X + 3 < a.ox1 ? val.w : 0.f};
  }
  st_f32x4(mem.out, i < q.rows ? q.vo : ICS_FFT_NONE, 32 * i * mem.lay.pitch, val);
}
// k_conv_fft<3>: `acc` raised to the largest |.| bits among the pixels of row group i that store_quad_at stores as they are (a pixel it stores as
// zero, or a dropped row group, counts as nothing).  The integer maximum of the bits is Maxima::ag's: a NaN ranks above inf.
ICS_FFT_HD uint32_t quad_absmax(const IcsFftArgs& a, const QuadOut& q, bool edge, int i, v4f val, uint32_t acc) {
  if (edge) {
    const int X = q.X;
    val = (v4f){X >= a.ox0 ? val.x : 0.f, (X + 1 >= a.ox0 && X + 1 < a.ox1) ? val.y : 0.f, (X + 2 >= a.ox0 && X + 2 < a.ox1) ? val.z : 0.f, X + 3 < a.ox1 ? val.w : 0.f};
  }
  uint32_t m = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) m = __builtin_elementwise_max(m, fbits(val[e]) & 0x7FFFFFFFu);
  return __builtin_elementwise_max(acc, i < q.rows ? m : 0u);
}
// ... and word `idx` of the launch's array of wave maxima (ICS_FFT_NONE: no access), unconditionally issued like every access of the unit loop
ICS_FFT_HD void store_wave_key(uint32_t* keys, int idx, uint32_t v) { st_f32(make_gbuf(keys), idx, 0, __builtin_bit_cast(float, v)); }
// Fused A11 + A13 unit: the residual of row group i, e' = r - image (pyx:563-565) on the tile's valid pixels inside the M x N interior and
// exact zeros everywhere else of the 128 x 128 tile (what k_gradk_fft reads back from the residual frame), goes back into the slots it
// was read from -- the operand of the second forward transform -- and, for tiles under the stop-test window, to the residual frame.
ICS_FFT_HD void residual_quads(const IcsFftArgs& a, const Mem& mem, const QuadOut (&qo)[2], bool edge, bool store, v2f* lds, int tid, int i, const v4f (&fimg)[2][4]) {
  v4f r[2];
  read_quads(lds, tid, i, r);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bool row_ok = i < qo[t].rows;
    const int X = qo[t].X;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = ICS_FSUB(r[t][e], fimg[t][i][e]);        // pyx:565
      const bool ok = edge ? (row_ok && X + e >= a.ox0 && X + e < a.ox1) : row_ok;
      r[t][e] = ok ? d : 0.f;
    }
  }
  const int r0 = tid >> 5, xq = tid & 31;
  v4f* wp = reinterpret_cast<v4f*>(lds + (r0 + 32 * i) * ICS_FFT_PITCH + 4 * xq);
  wp[0] = (v4f){r[0].x, r[1].x, r[0].y, r[1].y};
  wp[1] = (v4f){r[0].z, r[1].z, r[0].w, r[1].w};
  if (store) {
#pragma unroll
    for (int t = 0; t < 2; ++t) st_f32x4(mem.out, i < qo[t].rows ? qo[t].vo : ICS_FFT_NONE, 32 * i * mem.lay.pitch, r[t]);
  }
}

// ---- mode 2 (k_conv_fft<2>): A1 + A2 + A3 of a tile pair in one unit -----------------------------------------------------------------------
// The residual a back-projection tile reads is the M x N interior's (zero outside, pyx:482-491).  A tile whose residual window -- the
// V2 + 2 pad pixels a side around it -- lies inside the interior needs no mask and runs in the frequency domain alone (stage_d2_half); the
// tiles of the outer ring take both transforms pairs, with the mask in between (`border`).  u-frame coordinates.
ICS_FFT_HD bool tile_is_border(const IcsFftArgs& a, int oy, int ox) {
  const IcsGeom& g = a.c.g;
  return oy - g.pad < g.pad || oy + tile_rows(a, oy) + g.pad > g.pad + g.M || ox - g.pad < g.pad || ox + tile_cols(a, ox) + g.pad > g.pad + g.N;
}
ICS_FFT_HD bool unit_is_border(const IcsFftArgs& a, const Unit& u) {
  return tile_is_border(a, u.oy[0], u.ox[0]) || (u.has[1] && tile_is_border(a, u.oy[1], u.ox[1]));
}
// border units, between the two transform pairs: the tile buffer holds conv(u) of the window that starts (pad, pad) before the output
// tile; e = conv - image inside the interior, 0 outside it (pyx:488 and the zero extension of mode "full", pyx:491), back into the slots
// it was read from.  Row-quad ownership; the image quads of all four row groups are requested first.
ICS_FFT_HD void residual_window(const IcsFftArgs& a, const Mem& mem, const Unit& u, v2f* lds, int tid) {
  const IcsGeom& g = a.c.g;
  const int r0 = tid >> 5, xq = tid & 31, pad = g.pad;
  v4f f[2][4];
  int X[2], Y0[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    X[t] = u.ox[t] - pad + 4 * xq; Y0[t] = u.oy[t] - pad + r0;
    const int vo = (u.has[t] && X[t] + 3 >= pad && X[t] < pad + g.N) ? mem.lay.org + Y0[t] * mem.lay.pitch + X[t] + mem.lay.cmul * u.c : ICS_FFT_NONE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int Y = Y0[t] + 32 * i;
      f[t][i] = ld_f32x4<2>(mem.f, (Y >= pad && Y < pad + g.M) ? vo : ICS_FFT_NONE, 32 * i * mem.lay.pitch);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v4f r[2];
    read_quads(lds, tid, i, r);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int Y = Y0[t] + 32 * i;
      const bool row_ok = u.has[t] && Y >= pad && Y < pad + g.M;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = ICS_FSUB(r[t][e], f[t][i][e]);                 // pyx:488
        r[t][e] = (row_ok && X[t] + e >= pad && X[t] + e < pad + g.N) ? d : 0.f;
      }
    }
    v4f* wp = reinterpret_cast<v4f*>(lds + (r0 + 32 * i) * ICS_FFT_PITCH + 4 * xq);
    wp[0] = (v4f){r[0].x, r[1].x, r[0].y, r[1].y};
    wp[1] = (v4f){r[0].z, r[1].z, r[0].w, r[1].w};
  }
}

// mode 1: g = lambd gradu + (u - ut)/2 (pyx:519) for the maxima of A7 on row group i of tile t; the PAM kinds replace the stored value by G
template <bool TV>
ICS_FFT_HD void maxima_quad(const IcsFftArgs& a, const Unit& u, int tid, int t, int i, v4f& r, const Ops& o, Maxima& mx, const QuadOut& q, bool edge) {
  const float lambd = a.c.lambd;
  const int X0 = q.X;
  const bool row_ok = i < q.rows;         // (quad_lane: tile present, quad inside the tile's valid columns and the region, row group inside)
  uint32_t qg = 0u, qu = 0u, qany = 0u;
  float qm = -__builtin_inff();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float rv = r[e], uv = o.a[t][i][e], tv = o.b[t][i][e];
    const int X = X0 + e;
    float g;
    if (TV && a.c.tv_kind >= 2) { g = (float)((double)tv + (double)ICS_FMUL(lambd, rv)); r[e] = g; }     // PAM: G = T + lambd*gradu, stored (o.b holds T)
    else
      g = ics_mm_g(lambd, rv, uv, tv);
    if (edge) {                                        // (wave-uniform) first / last tile of a tile row: per-pixel column test
      const bool ok = row_ok && X >= a.ox0 && X < a.ox1;
      qg = __builtin_elementwise_max(qg, ok ? (fbits(g) & 0x7FFFFFFFu) : 0u);
      qu = __builtin_elementwise_max(qu, ok ? (fbits(uv) & 0x7FFFFFFFu) : 0u);
      qm = __builtin_fmaxf(qm, ok ? uv : -__builtin_inff());
      qany |= ok ? 1u : 0u;
    } else {
      qg = __builtin_elementwise_max(qg, fbits(g) & 0x7FFFFFFFu);
      qu = __builtin_elementwise_max(qu, fbits(uv) & 0x7FFFFFFFu);
      qm = __builtin_fmaxf(qm, uv);
    }
  }
  if (edge) { mx.ag = __builtin_elementwise_max(mx.ag, qg); mx.au = __builtin_elementwise_max(mx.au, qu); mx.mu = __builtin_fmaxf(mx.mu, qm); mx.any |= qany; }
  else {
    mx.ag = __builtin_elementwise_max(mx.ag, row_ok ? qg : 0u); mx.au = __builtin_elementwise_max(mx.au, row_ok ? qu : 0u);
    mx.mu = __builtin_fmaxf(mx.mu, row_ok ? qm : -__builtin_inff()); mx.any |= row_ok ? 1u : 0u;
  }
}

__device__ __forceinline__ void wave_sync() {
  // stages C, D, E exchange data between the lanes of ONE wave through LDS: a wave's DS operations execute in order, the compiler must
  // keep them in program order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a copy of `x` the optimiser cannot trace back: lane constants derived from it (LDS addresses, frame offsets) are recomputed in the stage that
// uses them instead of being hoisted out of the unit loop and kept alive -- and spilled -- across it (as in ics_conv_mfma.hip)
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }

// workgroup barrier that waits for this wave's LDS traffic only (__syncthreads() also waits for the global loads and stores in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace icsfft

// ---- host side: arguments, grid, launch ------------------------------------------------------------------------------------------------------
// the region and valid part of `mode`, then ics_fft_tile_grid (ics_conv_fft.hip)
void ics_conv_fft_fill_args(int mode, const IcsConvArgs& c, const float* spec, IcsFftArgs* a, int blk_n = 0, int blk_k = 0);
hipError_t ics_launch_conv_fft_sel(const IcsFftArgs& a, hipStream_t s);   // k_conv_fft<3, false> (ics_conv_fft_sel.hip); `a` as ics_launch_conv2_fft fills it
// One persistent workgroup per CU, capped by the max_wgs debug switch and by the number of units.  triples: the PSF-gradient kernels, whose
// workgroups keep one channel each (blockIdx % 3) -- a multiple of three, three at least.
static inline int ics_fft_grid(int cus, int nunits, bool triples = false) {
  int grid = cus;
  if (const int mw = ics_debug().max_wgs.load(std::memory_order_relaxed); mw > 0 && grid > mw) grid = mw;
  if (triples) grid = grid < 3 ? 3 : grid / 3 * 3;
  return grid > nunits ? nunits : grid;
}
// `configured` = one flag per device, static in the launcher, one array per kernel instantiation (ics_configure_lds)
template <typename Kern, typename... Args>
static inline hipError_t ics_fft_launch(std::atomic<bool>* configured, Kern kern, int grid, hipStream_t s, Args... args) {
  if (hipError_t e = ics_configure_lds(configured, ics_current_device(), kern, ICS_FFT_LDS_BYTES); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(ICS_FFT_THREADS), ICS_FFT_LDS_BYTES, s, args...);
  return hipGetLastError();
}
