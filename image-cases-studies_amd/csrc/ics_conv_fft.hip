// ics_conv_fft.hip -- transform tiles (ics_fft_tile.h): the convolutions k_conv_fft<0|1|2> (and, built by ics_conv_fft_sel.hip from this file, the
// operand-free mode-2 instance k_conv_fft<3>) and, for wide PSFs, k_conv_fft_blk<0|1>, the image
// spectra of mode 2, the weight spectra (k_fft_spectrum; with the PSF step in front of them: k_psf_spectra), and the arguments every tile kernel is launched with (ics_conv_fft_fill_args).
#include "ics_fft_tile.h"
#include "ics_psf_step.h"
#include "ics_maxg_select.h"
#include <algorithm>
#include <cassert>
#include <mutex>
#include <vector>

namespace icsfft {

// MODE 3 = mode 2 without the epilogue's operands (ics_maxg_select.h; instantiated in ics_conv_fft_sel.hip alone): the same units and the same
// stored values; instead of the maxima of A6 / A7 it records max |gradu| per tile and wave (a.c.dofkeys: [unit][tile][wave]) and per channel
// (a.c.sched: three words) -- two pointers of IcsConvArgs no tile kernel reads otherwise, so that IcsFftArgs keeps its layout.
template <int MODE, bool TV>
__global__ __launch_bounds__(ICS_FFT_THREADS) void k_conv_fft(IcsFftArgs a) {
  constexpr bool M2 = MODE >= 2, SEL = MODE == 3;
  extern __shared__ __attribute__((aligned(16))) v2f lds[];
  v2f* const twl = lds + ICS_FFT_P * ICS_FFT_PITCH;
  const int tid = threadIdx.x;
  const int G = gridDim.x;
  if (tid < ICS_FFT_TW_ENTRIES) twl[tid] = tw128((tid / ICS_FFT_TWS) * (tid % ICS_FFT_TWS));
  const Mem mem = make_mem(a, M2 ? 2 : MODE);
  // workgroup b runs on XCD b % 8 (observed dispatch): consecutive unit slots q go to one XCD, so the three channel units of a tile pair
  // (n = 3 pair + c) share that XCD's L2.  Affects speed only.
  const int q = (G & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3);
  uint32_t accg[3] = {0u, 0u, 0u}, accu[3] = {0u, 0u, 0u};   // the workgroup's maxima as order-preserving keys (0 = nothing seen, NaN = largest)
  // A unit's window is requested one unit ahead (registers).  It enters the tile buffer -- and runs its stage A -- at the END of the unit
  // before it, behind that unit's stores: there the compiler knows exactly what is in flight (the window loads, then the stores) and waits
  // with vmcnt(n_stores).  (Consumed at the top of the loop the wait became vmcnt(0): the loop header merges the first entry, where
  // nothing follows the loads.)
  v4f pw[2][4];
  if (q < a.nunits) {
    load_window(a, mem, decode_unit(a, walk_unit(a, q)), opaque(tid), pw);
    store_window(pw, lds, opaque(tid));
    lds_barrier();
    stage_a(lds, opaque(tid));
  }
  for (int k = q; k < a.nunits; k += G) {
    const int n = walk_unit(a, k);
    const Unit u = decode_unit(a, n);
    lds_barrier();
    stage_b<1>(lds, opaque(tid));
    lds_barrier();
    if (M2) {
      // A1 + A3 in one unit (see stage_d2_half): interior tiles stay in the frequency domain between the two convolutions
      if (!unit_is_border(a, u)) {
        v2f fs[2][8], s0[8], s1[8];
        load_spectrum_half<1>(mem.fspec, 8 * n, opaque(tid), 0, fs[0]);       // the image windows' spectrum of this unit: from HBM, requested first
        load_spectrum_half<1>(mem.fspec, 8 * n, opaque(tid), 1, fs[1]);
        load_spectrum_half<1>(mem.spec, 8 * u.c, opaque(tid), 0, s0);
        load_spectrum_half<1>(mem.spec1, 8 * u.c, opaque(tid), 0, s1);
        stage_c<4>(lds, lds, twl, opaque(tid));
        wave_sync();
        stage_d2_half(s0, s1, fs[0], lds, opaque(tid), 0);
        load_spectrum_half<1>(mem.spec, 8 * u.c, opaque(tid), 1, s0);         // the second halves of the weight spectra behind the first pass
        load_spectrum_half<1>(mem.spec1, 8 * u.c, opaque(tid), 1, s1);
        stage_d2_half(s0, s1, fs[1], lds, opaque(tid), 1);
        wave_sync();
      } else {
        // the outer ring: conv, residual with its mask in the tile buffer, then the correlation (four transforms, as the two kernels)
        {
          v2f sp[2][8];
          load_spectrum(mem, u.c, opaque(tid), sp);
          stage_c(lds, lds, twl, opaque(tid));
          wave_sync();
          stage_d(sp, lds, opaque(tid));
        }
        wave_sync();
        stage_e(lds, lds, twl, opaque(tid));
        lds_barrier();
        stage_b<-1>(lds, opaque(tid));
        lds_barrier();
        stage_g(lds, opaque(tid));
        lds_barrier();
        residual_window(a, mem, u, lds, opaque(tid));
        lds_barrier();
        stage_a(lds, opaque(tid));
        lds_barrier();
        stage_b<1>(lds, opaque(tid));
        lds_barrier();
        {
          v2f sp[2][8];
#pragma unroll
          for (int h = 0; h < 2; ++h) load_spectrum_half<1>(mem.spec1, 8 * u.c, opaque(tid), h, sp[h]);
          stage_c(lds, lds, twl, opaque(tid));
          wave_sync();
          stage_d(sp, lds, opaque(tid));
        }
        wave_sync();
      }
    } else {
    v2f sp[2][8];
    load_spectrum(mem, u.c, opaque(tid), sp);      // (stage C's arithmetic covers their trip to L2; inside stage D the waves queued up on it)
    stage_c(lds, lds, twl, opaque(tid));
    wave_sync();
    stage_d(sp, lds, opaque(tid));
    wave_sync();
    }
    load_window(a, mem, decode_unit(a, walk_unit(a, k + G)), opaque(tid), pw, 0, (MODE == 0 || SEL) ? 2 : 1);   // next unit (beyond the last one: dropped accesses); mode 1 holds 64 operand registers through stage G and requests the second tile behind it
    stage_e(lds, lds, twl, opaque(tid));
    v4f fimg[2][4];
    Ops ops;
    if (MODE == 0) load_image(a, mem, u, opaque(tid), fimg);
    else if (!SEL) {
      load_ops<TV, M2>(a, mem, u, opaque(tid), 0, ops);
      load_ops<TV, M2>(a, mem, u, opaque(tid), 1, ops, 0, 1);   // (stages F and G leave registers for the first row group of tile 1's operands)
    }
    lds_barrier();
    stage_b<-1>(lds, opaque(tid));
    lds_barrier();
    stage_g(lds, opaque(tid));
    lds_barrier();
    // row-quad epilogue, row group by row group (at most one group's raw values alive beside the operands).  Mode 1 has two operand
    // frames: it requests those of the second tile here and takes its maxima in a second pass, and the second tile of the next unit's
    // window goes out between the passes (registers: 128 per thread with 1024 of them).
    if (MODE >= 1 && !SEL) load_ops<TV, M2>(a, mem, u, opaque(tid), 1, ops, 1, 4);
    Maxima mx; maxima_init(mx);
    v4f res[4][2];
    // lane address and row-group count of the two tiles ONCE per unit (as eight store_quad calls the address arithmetic of the epilogue
    // was 300 of a unit's 1310 vector instructions).  u.ox is wave-uniform: interior tiles -- all but the first and last of a tile row --
    // need no per-pixel column tests.
    QuadOut qo[2];
    const int te = opaque(tid);
#pragma unroll
    for (int t = 0; t < 2; ++t) qo[t].vo = quad_lane<M2>(a, u, mem.lay, te, t, qo[t].rows, qo[t].X);
    const bool edge = unit_is_edge<M2>(a, u);
    uint32_t tg[2] = {0u, 0u};   // (SEL) bits of max |gradu| over this thread's valid pixels of the two tiles
    if (SEL) {
      // no operands: a row group leaves as soon as its maximum is taken -- of the value that is stored, so a pixel outside the region counts as the 0 it is stored as
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        read_quads(lds, opaque(tid), i, res[i]);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (edge) { tg[t] = quad_absmax(a, qo[t], true, i, res[i][t], tg[t]); store_quad_at(a, mem, qo[t], true, i, res[i][t]); }
          else { tg[t] = quad_absmax(a, qo[t], false, i, res[i][t], tg[t]); store_quad_at(a, mem, qo[t], false, i, res[i][t]); }
        }
        asm volatile("" ::: "memory");
      }
    } else if (MODE == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        read_quads(lds, opaque(tid), i, res[i]);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) res[i][t][e] = ICS_FSUB(res[i][t][e], fimg[t][i][e]);        // pyx:488
        asm volatile("" ::: "memory");
      }
      if (edge) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t) store_quad_at(a, mem, qo[t], true, i, res[i][t]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t) store_quad_at(a, mem, qo[t], false, i, res[i][t]);
      }
    } else {
      // first pass: tile 0 leaves as soon as its maxima are taken (its operands' registers are free for the second window then), tile 1's
      // values wait in res[.][1] for their operands
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        read_quads(lds, opaque(tid), i, res[i]);
        if (edge) { maxima_quad<TV>(a, u, te, 0, i, res[i][0], ops, mx, qo[0], true); store_quad_at(a, mem, qo[0], true, i, res[i][0]); }
        else { maxima_quad<TV>(a, u, te, 0, i, res[i][0], ops, mx, qo[0], false); store_quad_at(a, mem, qo[0], false, i, res[i][0]); }
        asm volatile("" ::: "memory");
      }
      load_window(a, mem, decode_unit(a, walk_unit(a, k + G)), opaque(tid), pw, 1, 2);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (edge) { maxima_quad<TV>(a, u, te, 1, i, res[i][1], ops, mx, qo[1], true); store_quad_at(a, mem, qo[1], true, i, res[i][1]); }
        else { maxima_quad<TV>(a, u, te, 1, i, res[i][1], ops, mx, qo[1], false); store_quad_at(a, mem, qo[1], false, i, res[i][1]); }
      }
    }
    if (k + G < a.nunits) {
      store_window(pw, lds, opaque(tid));      // (the slots this thread just read)
      lds_barrier();
      stage_a(lds, opaque(tid));
    }
    if (SEL) {   // the tile maxima of this wave: lane 0 stores them (no atomic inside the loop), the workgroup keeps the channel's
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint32_t wg = ics_wave_max_u32(tg[t]);
        store_wave_key(a.c.dofkeys, (tid & 63) == 0 ? (n * 2 + t) * (ICS_FFT_THREADS / 64) + (tid >> 6) : ICS_FFT_NONE, wg);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (u.c == c) accg[c] = accg[c] > wg ? accg[c] : wg;
      }
    } else if (MODE >= 1) {   // (u.c is uniform)
      uint32_t kg, ku;
      maxima_keys(mx, kg, ku);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (u.c == c) { accg[c] = accg[c] > kg ? accg[c] : kg; accu[c] = accu[c] > ku ? accu[c] : ku; }
    }
  }
  if (SEL) {   // (accg is wave-uniform already)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if ((tid & 63) == 0 && accg[c] > a.c.sched[c]) atomicMax(a.c.sched + c, accg[c]);
  } else if (MODE >= 1) {
    // the workgroup's maxima: wave maxima -> one conditional atomic per wave, channel and value at the END of the kernel (inside the loop
    // the read of the running maximum waited for every store in flight)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t kg = ics_wave_max_u32(accg[c]), ku = ics_wave_max_u32(accu[c]);
      if ((tid & 63) == 0) {
        if (kg > a.c.red[ICS_RED_MAXG + c]) atomicMax(a.c.red + ICS_RED_MAXG + c, kg);
        if (ku > a.c.red[ICS_RED_MAXU + c]) atomicMax(a.c.red + ICS_RED_MAXU + c, ku);
      }
    }
  }
}

#ifdef ICS_FFT_SEL_UNIT
// ics_conv_fft_sel.hip: this unit builds k_conv_fft<3, false> and its launcher, and nothing else.  An instance more in the unit of the
// others moves their register allocation (ics_fft_tile.h, head), so the operand-free instance lives alone.
}  // namespace icsfft
hipError_t ics_launch_conv_fft_sel(const IcsFftArgs& a, hipStream_t s) {
  static std::atomic<bool> configured[ICS_MAX_DEVICES];
  if (!a.spec1 || !a.fspec || !a.c.dofkeys || !a.c.sched || a.c.tv) return hipErrorInvalidValue;
  return ics_fft_launch(configured, icsfft::k_conv_fft<3, false>, ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits), s, a);
}
#else
// ---- PSF sizes above ICS_FFT_MAX_K: tap blocks on the tiles -----------------------------------------------------------------------------------
// A tile keeps 128 - K + 1 of its 128 pixels a side: 32 at 97, nothing at 129.  A convolution is linear in its taps, so the K x K PSF is cut
// into blk_n x blk_n blocks of blk_k x blk_k taps (blk_k <= 65) and block (qa, qb) is the blk_k x blk_k kernel on the window that starts
// (qa blk_k, qb blk_k) further down / right:
//     out = sum_q IDFT( S_q . DFT(window_q) ) = IDFT( sum_q S_q . DFT(window_q) )
// -- blk_n^2 forward transforms whose products meet in the frequency domain (sixteen complex values per thread), ONE inverse transform and
// one epilogue per unit, with tiles of 128 - blk_k + 1 valid pixels a side.  The epilogues are those of modes 0 and 1 (shipped loop).
template <int MODE>
__global__ __launch_bounds__(ICS_FFT_THREADS) void k_conv_fft_blk(IcsFftArgs a) {
  extern __shared__ __attribute__((aligned(16))) v2f lds[];
  v2f* const twl = lds + ICS_FFT_P * ICS_FFT_PITCH;
  const int tid = threadIdx.x;
  const int G = gridDim.x;
  if (tid < ICS_FFT_TW_ENTRIES) twl[tid] = tw128((tid / ICS_FFT_TWS) * (tid % ICS_FFT_TWS));
  const Mem mem = make_mem(a, MODE);
  const int q = (G & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3);
  uint32_t accg[3] = {0u, 0u, 0u}, accu[3] = {0u, 0u, 0u};
  const int nblk = a.blk_n * a.blk_n;
  // (the blocks' windows are NOT requested a block ahead: the running sum, the block's spectrum and a window in flight through the runtime
  //  loop over the blocks spill 40 registers; every block waits out its window's round trip -- measured 5-10 x ahead of the matrix cores' tap
  //  blocks as it is)
  for (int n = q; n < a.nunits; n += G) {
    const Unit u = decode_unit(a, n);
    v2f acc[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[s][k] = (v2f){0.f, 0.f};
    for (int b = 0; b < nblk; ++b) {
      const int qa = b / a.blk_n, qb = b - qa * a.blk_n;
      {
        v4f pw[2][4];
        load_window(a, mem, u, opaque(tid), pw, 0, 2, qa * a.blk_k, qb * a.blk_k);
        lds_barrier();                            // (the previous block's stage D / the previous unit's epilogue has read the tile)
        store_window(pw, lds, opaque(tid));
      }
      lds_barrier();
      stage_a(lds, opaque(tid));
      lds_barrier();
      stage_b<1>(lds, opaque(tid));
      lds_barrier();
      v2f sp[2][8];
#pragma unroll
      for (int h = 0; h < 2; ++h) load_spectrum_half<1>(mem.spec, 8 * (3 * b + u.c), opaque(tid), h, sp[h]);
      stage_c<4>(lds, lds, twl, opaque(tid));
      wave_sync();
      stage_d_mac(lds, opaque(tid), sp, acc);
    }
    lds_barrier();
    stage_d_inverse(acc, lds, opaque(tid));
    wave_sync();
    stage_e(lds, lds, twl, opaque(tid));
    lds_barrier();
    stage_b<-1>(lds, opaque(tid));
    lds_barrier();
    stage_g(lds, opaque(tid));
    QuadOut qo[2];
    const int te = opaque(tid);
#pragma unroll
    for (int t = 0; t < 2; ++t) qo[t].vo = quad_lane(a, u, mem.lay, te, t, qo[t].rows, qo[t].X);
    const bool edge = u.ox[0] < a.ox0 || u.ox[0] + a.V > a.ox1 || u.ox[1] < a.ox0 || u.ox[1] + a.V > a.ox1;
    if (MODE == 0) {
      v4f fimg[2][4];
      load_image(a, mem, u, opaque(tid), fimg);
      lds_barrier();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v4f r[2];
        read_quads(lds, te, i, r);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int e = 0; e < 4; ++e) r[t][e] = ICS_FSUB(r[t][e], fimg[t][i][e]);        // pyx:488
          store_quad_at(a, mem, qo[t], edge, i, r[t]);
        }
      }
    } else {
      Ops ops;
      load_ops<false>(a, mem, u, opaque(tid), 0, ops);
      load_ops<false>(a, mem, u, opaque(tid), 1, ops);
      lds_barrier();
      Maxima mx; maxima_init(mx);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v4f r[2];
        read_quads(lds, te, i, r);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          maxima_quad<false>(a, u, te, t, i, r[t], ops, mx, qo[t], edge);
          store_quad_at(a, mem, qo[t], edge, i, r[t]);
        }
      }
      uint32_t kg, ku;
      maxima_keys(mx, kg, ku);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (u.c == c) { accg[c] = accg[c] > kg ? accg[c] : kg; accu[c] = accu[c] > ku ? accu[c] : ku; }
    }
  }
  if (MODE == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t kg = ics_wave_max_u32(accg[c]), ku = ics_wave_max_u32(accu[c]);
      if ((tid & 63) == 0) {
        if (kg > a.c.red[ICS_RED_MAXG + c]) atomicMax(a.c.red + ICS_RED_MAXG + c, kg);
        if (ku > a.c.red[ICS_RED_MAXU + c]) atomicMax(a.c.red + ICS_RED_MAXU + c, ku);
      }
    }
  }
}

// ---- the image side of mode 2: F = DFT of the two image windows of every unit (unnormalised), once per image ----------------------------------
// k_conv_fft<2> subtracts it from 16384 S0 T in stage D -- the "- image" of pyx:488 in the frequency domain.  The window of a unit's tile
// starts (pad, pad) before the tile's first output pixel (where the residual window of the back-projection starts); the image frame is zero
// outside the M x N interior.  Stored in load_spectrum's order, one block of 8 x 1024 quads per unit: 128 KB per unit, read once per inner
// iteration (HBM), written once per upload of the image.  `a` = the mode-2 geometry with in = the image's planar mirror and wpad = pad.
template <int DUMMY>
__global__ __launch_bounds__(ICS_FFT_THREADS) void k_fft_image_spectrum(IcsFftArgs a) {
  extern __shared__ __attribute__((aligned(16))) v2f lds[];
  v2f* const twl = lds + ICS_FFT_P * ICS_FFT_PITCH;
  const int tid = threadIdx.x;
  if (tid < ICS_FFT_TW_ENTRIES) twl[tid] = tw128((tid / ICS_FFT_TWS) * (tid % ICS_FFT_TWS));
  const Mem mem = make_mem(a, 2);
  for (int n = blockIdx.x; n < a.nunits; n += gridDim.x) {
    const Unit u = decode_unit(a, n);
    v4f pw[2][4];
    load_window(a, mem, u, opaque(tid), pw);
    lds_barrier();                                // (the previous unit's stage D has read the tile)
    store_window(pw, lds, opaque(tid));
    lds_barrier();
    stage_a(lds, opaque(tid));
    lds_barrier();
    stage_b<1>(lds, opaque(tid));
    lds_barrier();
    stage_c(lds, lds, twl, opaque(tid));
    wave_sync();
    v2f z[2][8];
    stage_d_forward(lds, opaque(tid), z);
    store_spectrum(mem.fspec, 8 * n, opaque(tid), z);
  }
}

// ---- spectrum: S_o,c[ky][kx] = conj( sum_{a,b} W_o[a][b][c] w^(a ky + b kx) ) / 128^2,  w = exp(-2 pi i / 128), stored at spec_index(c, ky, kx) ----
// W_0 = rot180(psf) (mode 0), W_1 = psf (mode 1).  Double accumulation (a PSF value enters with its float32 value, the twiddles from a
// double table built on the device); one workgroup per (orientation, channel, 32 columns kx): G[a][kx] = sum_b W[a][b] w^(b kx) in LDS,
// then S[ky][kx] = conj(sum_a G[a][kx] w^(a ky)).
// (tap blocks: blockIdx.y = block q = qa * nb + qb of Kb x Kb taps starting at W_o[qa Kb][qb Kb], taps beyond K are zero; its spectra go to
//  spec + q * 3 * 128 * 128.  nb = 1, Kb = K: the whole PSF.)
__global__ __launch_bounds__(256) void k_fft_spectrum(const float* __restrict__ psf, int K, v2f* __restrict__ spec0, v2f* __restrict__ spec1, int nb, int Kb) {
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [128][2] twiddles, then [K][32][2] G
  double* twd = sm;
  double* Gs = sm + 256;
  const int tid = threadIdx.x;
  // one workgroup per (orientation, channel, 32 columns kx, 32 rows ky): 96 of them; each builds the G of its columns itself (K^2 x 32
  // products) and then its 32 x 32 values of S (K each).  (24 workgroups with all 128 rows each took 30 us at 31 x 31, 65 us at 63 x 63 --
  // per inner iteration of a blind run.)
  const int o = blockIdx.x / 48, c = (blockIdx.x / 16) % 3, kx0 = ((blockIdx.x >> 2) & 3) * 32, ky0 = (blockIdx.x & 3) * 32;
  const int qa = (int)blockIdx.y / nb, qb = (int)blockIdx.y - qa * nb, a0 = qa * Kb, b0 = qb * Kb;
  spec0 += (size_t)blockIdx.y * 3 * ICS_FFT_P * ICS_FFT_P; spec1 += (size_t)blockIdx.y * 3 * ICS_FFT_P * ICS_FFT_P;
  if (tid < 128) {
    double sn, cs;
    sincospi((double)tid / 64.0, &sn, &cs);
    twd[2 * tid] = cs; twd[2 * tid + 1] = -sn;
  }
  __syncthreads();
  for (int i = tid; i < Kb * 32; i += 256) {
    const int aa = i >> 5, kx = kx0 + (i & 31);
    double re = 0.0, im = 0.0;
    for (int b = 0; b < Kb; ++b) {
      const int ta = a0 + aa, tb = b0 + b;           // the tap of W_o this is
      double wv = 0.0;
      if (ta < K && tb < K) wv = o == 0 ? (double)psf[((K - 1 - ta) * K + (K - 1 - tb)) * 3 + c] : (double)psf[(ta * K + tb) * 3 + c];
      const int t = (b * kx) & 127;
      re += wv * twd[2 * t]; im += wv * twd[2 * t + 1];
    }
    Gs[2 * i] = re; Gs[2 * i + 1] = im;
  }
  __syncthreads();
  for (int i = tid; i < 32 * 32; i += 256) {
    const int ky = ky0 + (i >> 5), kxl = i & 31;
    double re = 0.0, im = 0.0;
    for (int aa = 0; aa < Kb; ++aa) {
      const double gr = Gs[2 * (aa * 32 + kxl)], gi = Gs[2 * (aa * 32 + kxl) + 1];
      const int t = (aa * ky) & 127;
      const double wr = twd[2 * t], wi = twd[2 * t + 1];
      re += gr * wr - gi * wi; im += gr * wi + gi * wr;
    }
    const double sc = 1.0 / (128.0 * 128.0);
    (o == 0 ? spec0 : spec1)[spec_index(c, ky, kx0 + kxl)] = (v2f){(float)(re * sc), (float)(-im * sc)};
  }
}

// ---- A14 ... A17 + both spectra in one launch (blind runs on the tiles, PSF sizes <= ICS_FFT_MAX_K) ---------------------------------------------
// k_psf and k_fft_spectrum were two dependent launches of 1 and 96 workgroups in every blind inner iteration, with nothing to run beside
// them and 6 ... 7 us of idle device between them.  Here the 96 workgroups of the spectrum launch each redo the small step on a private
// LDS copy of the PSF -- the same instructions on the same inputs, hence the same bits in every workgroup, and no workgroup waits for
// another -- and then transform their share of it exactly as k_fft_spectrum does.  Workgroup 0 alone stores psf_next, psf_caller, dtpsf
// and the `frozen` flag, and alone reads that flag.  The PSF is read from a.psf and written to a.psf_next: workgroup 0 may finish before
// another workgroup has started.  Neither the row-pair tables nor the fp16 Toeplitz tables are packed: no tile kernel reads them.
// (Also summing the gradient's blocks here, every workgroup for itself in the order of k_gradk_fft_reduce, was built and measured:
//  bit-identical and slower at every size -- 4096^2 blind, ms per inner iteration, folded / k_gradk_fft_reduce as a launch:
//  15 x 15 0.6704 / 0.6612, 25 x 25 0.8565 / 0.8005, 31 x 31 0.9466 / 0.8670; the launch it saves costs 5.3 us + a kernel boundary, the
//  redundant sums 25 us at 15 x 15 -- 3 K^2 values x 255 blocks per workgroup from L2 in dependent batches.  NOTES_r07.md.)

// GR = gradient values per thread at the largest PSF of the instance (value i = tid + r * 1024, as the PSF's own copy loop)
template <int GR>
__global__ __launch_bounds__(1024) void k_psf_spectra(IcsPsfSpectraArgs a) {
  constexpr int NTHR = 1024;
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [128][2] twiddles, [K][32][2] G, then the PSF: [K][K][3] floats
  __shared__ uint32_t sred[2];
  __shared__ float ssum[3];
  const int K = a.K, KK = K * K, n = 3 * KK, tid = threadIdx.x;
  double* twd = sm;
  double* Gs = sm + 256;
  float* p = reinterpret_cast<float*>(Gs + 64 * K);
  const bool first = blockIdx.x == 0;
  const int frozen = first ? *a.frozen : 1;
  if (tid < 128) {
    double sn, cs;
    sincospi((double)tid / 64.0, &sn, &cs);
    twd[2 * tid] = cs; twd[2 * tid + 1] = -sn;
  }
  if (tid < 2) sred[tid] = 0u;
  for (int i = tid; i < n; i += NTHR) p[i] = a.psf[i];
  // ---- phase 1: the gradient (everything the step needs from global memory is requested up front) ----
  float gk[GR];
#pragma unroll
  for (int r = 0; r < GR; ++r) { const int i = tid + r * NTHR; gk[r] = i < n ? a.gradk[i] : 0.f; }
  __syncthreads();
  // ---- phase 2: A14 ... A17 (ics_psf_step.h) ----
  uint32_t kp = 0u, kg = 0u;
#pragma unroll
  for (int r = 0; r < GR; ++r) {
    const int i = tid + r * NTHR;
    if (i < n) {
      const uint32_t k1 = ics_key_of(p[i]), k2 = ics_key_of(__builtin_fabsf(gk[r]));
      kp = kp > k1 ? kp : k1; kg = kg > k2 ? kg : k2;
    }
  }
  kp = ics_shfl_max_u32(kp); kg = ics_shfl_max_u32(kg);
  if ((tid & 63) == 0) { atomicMax(&sred[0], kp); atomicMax(&sred[1], kg); }
  __syncthreads();
  const float dtpsf = ics_psf_dt(a.step, K, ics_key2f(sred[0]), ics_key2f(sred[1]));
  if (first && tid == 0) a.scal[ICS_SC_DTPSF] = dtpsf;
#pragma unroll
  for (int r = 0; r < GR; ++r) {
    const int i = tid + r * NTHR;
    if (i < n) {
      p[i] = ics_psf_step_px(p[i], dtpsf, gk[r]);
      if (!frozen) a.psf_caller[i] = p[i];
    }
  }
  __syncthreads();
  if (a.correlation) {
    for (int i = tid; i < KK; i += NTHR) {
      const float mval = ics_psf_mean3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
      p[3 * i] = mval; p[3 * i + 1] = mval; p[3 * i + 2] = mval;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += NTHR) p[i] = ics_psf_clamp(p[i]);
  __syncthreads();
  if (tid < 3) ssum[tid] = ics_psf_channel_sum(p, KK, tid);
  __syncthreads();
  const bool detach = a.correlation != 0;
  for (int i = tid; i < n; i += NTHR) {
    p[i] = ics_psf_norm(p[i], ssum[i % 3]);
    if (first) a.psf_next[i] = p[i];
    if (!frozen && !detach) a.psf_caller[i] = p[i];
  }
  if (first && tid == 0 && detach) *a.frozen = 1;
  __syncthreads();
  // ---- phase 3: the two loops of k_fft_spectrum (whole PSF: one block of K x K taps), fed from the LDS copy ----
  const int o = blockIdx.x / 48, c = (blockIdx.x / 16) % 3, kx0 = ((blockIdx.x >> 2) & 3) * 32, ky0 = (blockIdx.x & 3) * 32;
  for (int i = tid; i < K * 32; i += NTHR) {
    const int aa = i >> 5, kx = kx0 + (i & 31);
    double re = 0.0, im = 0.0;
    for (int b = 0; b < K; ++b) {
      const double wv = o == 0 ? (double)p[((K - 1 - aa) * K + (K - 1 - b)) * 3 + c] : (double)p[(aa * K + b) * 3 + c];
      const int t = (b * kx) & 127;
      re += wv * twd[2 * t]; im += wv * twd[2 * t + 1];
    }
    Gs[2 * i] = re; Gs[2 * i + 1] = im;
  }
  __syncthreads();
  for (int i = tid; i < 32 * 32; i += NTHR) {
    const int ky = ky0 + (i >> 5), kxl = i & 31;
    double re = 0.0, im = 0.0;
    for (int aa = 0; aa < K; ++aa) {
      const double gr = Gs[2 * (aa * 32 + kxl)], gi = Gs[2 * (aa * 32 + kxl) + 1];
      const int t = (aa * ky) & 127;
      const double wr = twd[2 * t], wi = twd[2 * t + 1];
      re += gr * wr - gi * wi; im += gr * wi + gi * wr;
    }
    const double sc = 1.0 / (128.0 * 128.0);
    reinterpret_cast<v2f*>(o == 0 ? a.spec_conv : a.spec_corr)[spec_index(c, ky, kx0 + kxl)] = (v2f){(float)(re * sc), (float)(-im * sc)};
  }
}

}  // namespace icsfft

// ---- launchers -----------------------------------------------------------------------------------------------------------------------------
// (the stage functions are exact for any K <= 125; what bounds the range is the valid part of a tile, 128 - K + 1 pixels a side: 44 at 85)
bool ics_conv_fft_supported(int K) { return K >= 3 && K <= ICS_FFT_MAX_K && (K & 1); }
size_t ics_conv_fft_spectrum_floats() { return (size_t)3 * ICS_FFT_P * ICS_FFT_P * 2; }   // per orientation (and per tap block)
hipError_t ics_launch_fft_spectrum(const float* psf, int K, float* spec_conv, float* spec_corr, hipStream_t s, int blk_n, int blk_k) {
  const int nb = blk_n > 0 ? blk_n : 1, Kb = blk_n > 0 ? blk_k : K;
  const size_t lds = (256 + (size_t)Kb * 32 * 2) * sizeof(double);   // 35 KB at 65, 46 KB at 85
  hipLaunchKernelGGL(icsfft::k_fft_spectrum, dim3(96, nb * nb), dim3(256), lds, s, psf, K, reinterpret_cast<v2f*>(spec_conv), reinterpret_cast<v2f*>(spec_corr), nb, Kb);
  return hipGetLastError();
}

// (dynamic LDS: twiddles + G + the PSF = 15 KB at 15 x 15, 130 KB at 85 x 85 of the CU's 160)
hipError_t ics_launch_psf_spectra(const IcsPsfSpectraArgs& a, hipStream_t s) {
  if (a.K < 3 || a.K > ICS_FFT_MAX_K) return hipErrorInvalidValue;
  auto bytes = [](int K) { return (256 + (size_t)K * 64) * sizeof(double) + (size_t)3 * K * K * sizeof(float); };
  // two instances: the sizes mode 2 of the tiles serves keep three gradient values a thread, the others up to 22
  constexpr int K_FEW = 31, GR_FEW = (3 * K_FEW * K_FEW + 1023) / 1024, GR_ALL = (3 * ICS_FFT_MAX_K * ICS_FFT_MAX_K + 1023) / 1024;
  static std::atomic<bool> cfg_few[ICS_MAX_DEVICES], cfg_all[ICS_MAX_DEVICES];
  if (a.K <= K_FEW) {
    if (hipError_t e = ics_configure_lds(cfg_few, ics_current_device(), icsfft::k_psf_spectra<GR_FEW>, bytes(K_FEW)); e != hipSuccess) return e;
    hipLaunchKernelGGL((icsfft::k_psf_spectra<GR_FEW>), dim3(96), dim3(1024), bytes(a.K), s, a);
  } else {
    if (hipError_t e = ics_configure_lds(cfg_all, ics_current_device(), icsfft::k_psf_spectra<GR_ALL>, bytes(ICS_FFT_MAX_K)); e != hipSuccess) return e;
    hipLaunchKernelGGL((icsfft::k_psf_spectra<GR_ALL>), dim3(96), dim3(1024), bytes(a.K), s, a);
  }
  return hipGetLastError();
}

// the tile grid over the output region [oy0, oy1) x [ox0, ox1) of `a` with its valid part Vy x V
static void ics_fft_tile_grid(int mode, IcsFftArgs* a) {
  const IcsGeom& g = a->c.g;
  a->gx0 = a->ox0 & ~3;
  a->tiles_x = (a->ox1 - a->gx0 + a->V - 1) / a->V;
  int tiles_y = (a->oy1 - a->oy0 + a->Vy - 1) / a->Vy;
  a->ext_y = a->ext_x = 0;
  if (mode == 2) {
    // The far edge (tile_rows): where the tiles that cover the M interior rows end within 2 pad of the u-frame's last row, the last of them
    // stores the rest of the pad ring as well and the tile row behind it is not run -- 42 -> 41 tile rows and columns at 4096 / 15, 2646 ->
    // 2523 units = ten rounds on 256 workgroups instead of eleven.  An axis that loses no tile this way keeps ext = 0.
    const int ny = (g.M + a->Vy - 1) / a->Vy, nx = (g.N + a->V - 1) / a->V;
    if (ny < tiles_y) { a->ext_y = g.uM - ny * a->Vy; tiles_y = ny; }
    if (nx < a->tiles_x) { a->ext_x = g.uN - nx * a->V; a->tiles_x = nx; }
    // (0 < ext <= 2 pad follows from n V >= M and n < ceil(uM / V); an extended tile ends at or behind the interior's last row / column
    //  -- what tile_rows' derivation rests on -- and is one of the outer ring)
    assert(a->ext_y >= 0 && a->ext_y <= 2 * g.pad && a->ext_x >= 0 && a->ext_x <= 2 * g.pad);
    assert(!a->ext_y || (ny * a->Vy >= g.M && (ny - 1) * a->Vy + icsfft::tile_rows(*a, (ny - 1) * a->Vy) == g.uM));      // (> M: tile_is_border's row test)
    assert(!a->ext_x || (nx * a->V >= g.N && (nx - 1) * a->V + icsfft::tile_cols(*a, (nx - 1) * a->V) == g.uN));
  }
  a->ntiles = a->tiles_x * tiles_y;
  a->tiles_x_magic = 0x100000000ull / (unsigned)a->tiles_x + 1ull;
  a->nunits = 3 * ((a->ntiles + 1) / 2);
}

void ics_conv_fft_fill_args(int mode, const IcsConvArgs& c, const float* spec, IcsFftArgs* a, int blk_n, int blk_k) {
  a->c = c;
  a->wy0 = a->wy1 = a->wx0 = a->wx1 = 0; a->store_all = 0;
  a->wpad = c.g.pad; a->fspec = nullptr; a->spec1 = nullptr; a->lag_y = a->lag_x = 0; a->rot = 0;
  a->spec = reinterpret_cast<const v2f*>(spec);
  const IcsGeom& g = c.g;
  a->blk_n = blk_n; a->blk_k = blk_k;
  a->Vy = ICS_FFT_P - (blk_k ? blk_k : g.K) + 1;   // valid rows per tile: all of them (tap blocks: of the block's size)
  a->V = a->Vy & ~3;                     // valid pixels per tile row, whole quads (16-byte stores never straddle two tiles)
  if (mode == 2) { a->Vy = ICS_FFT_P - 2 * g.K + 2; a->V = a->Vy & ~3; a->wpad = 2 * g.pad; }   // A1 + A3 in one unit: the valid part of two convolutions in a row
  if (mode == 0) { a->oy0 = g.pad; a->ox0 = g.pad; a->oy1 = g.pad + g.M; a->ox1 = g.pad + g.N; }
  else { a->oy0 = 0; a->ox0 = 0; a->oy1 = g.uM; a->ox1 = g.uN; }
  ics_fft_tile_grid(mode, a);
}

hipError_t ics_launch_conv_fft_args(int mode, const IcsFftArgs& a, hipStream_t s) {
  static std::atomic<bool> configured[5][ICS_MAX_DEVICES];
  // (mode 1 with the T frame: the PAM kinds, whose epilogue takes u and T where the shipped loop takes u and ut.  The active MM-TV kind
  //  needs all three and does not fit 128 registers: not built)
  if (a.c.tv && a.c.tv_kind == 1) return hipErrorInvalidValue;
  const bool pam = mode == 1 && a.c.tv && a.c.tv_kind >= 2;
  auto k0 = icsfft::k_conv_fft<0, false>;
  auto k1 = icsfft::k_conv_fft<1, false>;
  auto k1t = icsfft::k_conv_fft<1, true>;
  auto k2 = icsfft::k_conv_fft<2, false>;
  auto k2t = icsfft::k_conv_fft<2, true>;
  const bool pam2 = mode == 2 && a.c.tv && a.c.tv_kind >= 2;      // (the PAM kinds' epilogue on mode 2's units: operands u and T, G = T + lambd gradu stored)
  if (mode == 2 && (!a.spec1 || !a.fspec)) return hipErrorInvalidValue;
  auto kern = mode == 2 ? (pam2 ? k2t : k2) : (mode == 0 ? k0 : (pam ? k1t : k1));
  const int slot = mode == 2 ? (pam2 ? 4 : 3) : (pam ? 2 : mode);
  return ics_fft_launch(configured[slot], kern, ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits), s, a);
}
hipError_t ics_launch_conv_fft(int mode, const IcsConvArgs& c, const float* spec, hipStream_t s) {
  if (mode != 0 && mode != 1) return hipErrorInvalidValue;   // (mode 2: ics_launch_conv2_fft)
  IcsFftArgs a;
  ics_conv_fft_fill_args(mode, c, spec, &a);
  return ics_launch_conv_fft_args(mode, a, s);
}
// mode 0 over a part of the interior only: the tiles that cover output rows [oy0, oy1) x columns [ox0, ox1) of the u-frame (a window of the
// residual; what lies outside the region inside a stored quad is written as zero, the rest of the frame is not touched)
hipError_t ics_launch_conv_fft_region(const IcsConvArgs& c, const float* spec, int oy0, int ox0, int oy1, int ox1, hipStream_t s) {
  IcsFftArgs a;
  ics_conv_fft_fill_args(0, c, spec, &a);
  a.oy0 = oy0; a.ox0 = ox0; a.oy1 = oy1; a.ox1 = ox1;
  ics_fft_tile_grid(0, &a);
  return ics_launch_conv_fft_args(0, a, s);
}
// ---- mode 2: A1 + A2 + A3 in one unit per tile pair (k_conv_fft<2>) ---------------------------------------------------------------------------
// valid output per tile: 128 - 2 K + 2 pixels a side; the per-unit image spectra must stay addressable with 32-bit byte offsets
size_t ics_conv2_fft_fspec_floats(const IcsGeom& g) {
  IcsConvArgs c; memset(&c, 0, sizeof c); c.g = g;
  IcsFftArgs a;
  ics_conv_fft_fill_args(2, c, nullptr, &a);
  return (size_t)a.nunits * 8 * ICS_FFT_THREADS * 4;
}
bool ics_conv2_fft_supported(const IcsGeom& g) {
  if (!ics_conv_fft_supported(g.K) || ICS_FFT_P - 2 * g.K + 2 < 16) return false;
  return ics_conv2_fft_fspec_floats(g) * sizeof(float) < 0x7FFFFFFFull;
}
// f = origin of the image's planar mirror; fspec = ics_conv2_fft_fspec_floats(g) floats
hipError_t ics_launch_fft_image_spectrum(const float* f, const IcsGeom& g, float* fspec, hipStream_t s) {
  IcsConvArgs c;
  memset(&c, 0, sizeof c);
  c.g = g; c.in = f; c.f = f; c.out = const_cast<float*>(f); c.u = f; c.ut = f;
  IcsFftArgs a;
  ics_conv_fft_fill_args(2, c, nullptr, &a);
  a.wpad = g.pad; a.fspec = fspec; a.spec = reinterpret_cast<const v2f*>(fspec); a.spec1 = a.spec;
  static std::atomic<bool> configured[ICS_MAX_DEVICES];
  return ics_fft_launch(configured, icsfft::k_fft_image_spectrum<0>, ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits), s, a);
}
// c: in = u = the u mirror's origin, out = the back-projection's, f = the image's, ut, red, lambd as for mode 1; spec_conv / spec_corr = the two
// weight spectra; fspec = the image spectra of THIS image and geometry
// wkeys + gmax (both or neither): the operand-free instance k_conv_fft<3> (ics_conv_fft_sel.hip; shipped loop), which takes no maxima of g and u
// but leaves max |gradu| per (unit, tile, wave) in wkeys -- ics_conv2_fft_units(g) * 2 * 16 words -- and raises the three words of gmax
hipError_t ics_launch_conv2_fft(const IcsConvArgs& c, const float* spec_conv, const float* spec_corr, const float* fspec, hipStream_t s, uint32_t* wkeys, uint32_t* gmax) {
  IcsFftArgs a;
  ics_conv_fft_fill_args(2, c, spec_conv, &a);
  if ((wkeys != nullptr) != (gmax != nullptr)) return hipErrorInvalidValue;
  a.spec1 = reinterpret_cast<const v2f*>(spec_corr); a.fspec = const_cast<float*>(fspec);
  // Where the static walk starts: the units of the outer ring take four transforms instead of two (about 1.6 of a unit's time), and a walk from
  // the first tile row ends on the last one -- the final, partial round of units is then made of the heaviest units (4096^2 / 15: 86 units of
  // the bottom row on 86 workgroups while 170 idle: 0.293 -> 0.281 ms with the walk started half way).  Of eight starting points the one with
  // the lightest most-loaded workgroup is taken (workgroup of walk position k = k mod grid); the choice depends on the geometry and the grid
  // only and is kept for the next launch.  Order only: results do not change.
  // The kept choice is one record (geometry, grid and rot together) read and written under a mutex: jobs of other geometries run
  // concurrently from several host threads (lib/banded.py: one per band), and a rot read apart from its own key could lie beyond this
  // launch's unit list, where walk_unit would send positions past the end and drop their units.
  if (ics_debug().fft_rot.load(std::memory_order_relaxed)) {
    struct RotCache { int M = -1, N = -1, K = -1, grid = -1, rot = 0; };
    static std::mutex cache_mu;
    static RotCache cache;
    const int grid = ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits);   // (what ics_launch_conv_fft_args launches)
    RotCache hit;
    {
      std::lock_guard<std::mutex> lk(cache_mu);
      hit = cache;
    }
    if (hit.M == c.g.M && hit.N == c.g.N && hit.K == c.g.K && hit.grid == grid) a.rot = hit.rot;
    else {
      std::vector<unsigned char> ring((size_t)a.nunits);
      for (int n = 0; n < a.nunits; ++n) ring[n] = icsfft::unit_is_border(a, icsfft::decode_unit(a, n)) ? 1 : 0;
      std::vector<int> load((size_t)grid);
      int best = 0; long best_cost = -1;
      static const int order[8] = {4, 0, 2, 6, 1, 3, 5, 7};      // (ties: the walk started half way first -- the form that was measured)
      for (int ci = 0; ci < 8; ++ci) {
        const int cand = order[ci];
        a.rot = (int)((long long)a.nunits * cand / 8);
        std::fill(load.begin(), load.end(), 0);
        for (int k = 0; k < a.nunits; ++k) load[k % grid] += ring[icsfft::walk_unit(a, k)] ? 16 : 10;      // (tenths of a two-transform unit)
        const long cost = *std::max_element(load.begin(), load.end());
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = a.rot; }
      }
      a.rot = best;
      RotCache fresh;
      fresh.M = c.g.M; fresh.N = c.g.N; fresh.K = c.g.K; fresh.grid = grid; fresh.rot = best;
      std::lock_guard<std::mutex> lk(cache_mu);
      cache = fresh;
    }
  }
  if (a.rot < 0 || a.rot >= a.nunits) a.rot = 0;   // (a start point outside the list would drop units; any inside it only reorders the walk)
  if (wkeys) { a.c.dofkeys = wkeys; a.c.sched = gmax; return ics_launch_conv_fft_sel(a, s); }
  return ics_launch_conv_fft_args(2, a, s);
}
// the tile grid of mode 2 on this geometry, for the selection kernel behind the operand-free instance (ics_maxg_select.h)
void ics_conv2_fft_select_grid(const IcsGeom& g, IcsMaxgSelectArgs* m) {
  IcsConvArgs c; memset(&c, 0, sizeof c); c.g = g;
  IcsFftArgs a;
  ics_conv_fft_fill_args(2, c, nullptr, &a);
  m->ntiles = a.ntiles; m->tiles_x = a.tiles_x; m->Vy = a.Vy; m->V = a.V; m->ext_y = a.ext_y; m->ext_x = a.ext_x;
  m->uM = g.uM; m->uN = g.uN; m->ppitch = ics_ppitch(g); m->plane = ics_plane_floats(g);
}
int ics_conv2_fft_units(const IcsGeom& g) { return (int)(ics_conv2_fft_fspec_floats(g) / ((size_t)8 * ICS_FFT_THREADS * 4)); }
// ---- tap blocks (PSF sizes above ICS_FFT_MAX_K) ------------------------------------------------------------------------------------------------
// the fewest blocks per axis whose size stays at 65 or below (2 to 129, 3 to 193, 4 to 255)
bool ics_conv_fft_blk_supported(int K) { return K > ICS_FFT_MAX_K && K <= 255 && (K & 1); }
void ics_conv_fft_blk_shape(int K, int* blk_n, int* blk_k) {
  int n = (K + 64) / 65;
  int k = (K + n - 1) / n;
  *blk_n = n; *blk_k = k;
}
// spec = this orientation's block spectra, blk_n^2 x [3][128][128] (ics_launch_fft_spectrum with blk_n, blk_k)
hipError_t ics_launch_conv_fft_blk(int mode, const IcsConvArgs& c, const float* spec, int blk_n, int blk_k, hipStream_t s) {
  if ((mode != 0 && mode != 1) || blk_n < 2 || blk_k < 3 || blk_k > 65 || (c.tv && c.tv_kind)) return hipErrorInvalidValue;   // (shipped loop)
  IcsFftArgs a;
  ics_conv_fft_fill_args(mode, c, spec, &a, blk_n, blk_k);
  static std::atomic<bool> configured[2][ICS_MAX_DEVICES];
  auto k0 = icsfft::k_conv_fft_blk<0>;
  auto k1 = icsfft::k_conv_fft_blk<1>;
  return ics_fft_launch(configured[mode], mode == 0 ? k0 : k1, ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits), s, a);
}
#endif   // ICS_FFT_SEL_UNIT
