// ics_img_noise.hip -- noise estimate of device-resident images (ics_img_noise_estimate, include/ics_hip.h): H x W x 3 float32, HWC,
// contiguous.  The exact lower median of the finest starlet detail scale, from which the host derives the noise level.
//
//   w_0      = c_0 - c_1, c_1 = V_0(H_0(c_0)): wv_pass along x, then along y, at d = 1, indices folded by wv_fold (ics_img_px.h; the
//              arithmetic of ics_img_wavelet.hip, no FMA)
//   key      "channel": |w_0| of every channel, three populations of n = H W values; "vector": m = sqrt((s0 + s1) + s2), the squares
//              of the three channels added smallest first, one population (ns_keys)
//   median   the value of rank k = (n - 1) / 2 of the sorted population.  The keys are non-negative floats, so they order like their
//              bit patterns read as unsigned integers: a radix select over the 31 bits below the sign.
//
// Three histogram passes of 11 + 10 + 10 bits, the most significant first.  A pass counts, per population, the keys whose bits above
// the pass's field equal the prefix found so far, by the value of the field.  Between two passes k_img_ns_select (one workgroup) scans
// the bins, finds the bin that holds the rank, appends it to the prefix, lowers the rank by the count below the bin, and leaves the
// histogram zeroed: prefix and rank live in a state block behind the histograms, nothing returns to the host between the passes.
// After the third pass the prefix is the median's bit pattern.  Counts are 32-bit integers (a frame has fewer than 2^31 values), so
// the result does not depend on the order in which the atomics arrive.
//
// 11 bits first: the field then holds the exponent and three mantissa bits, eight bins per octave; |w_0| of a noisy picture spreads
// over two to three octaves, so the fullest bin takes about 6 % of the keys, four lanes of a wave.  With 8 bits (the exponent alone)
// a third of a wave would meet at one address.  Two further measures against lanes at one LDS address (ns_count): every bin has two
// counters, for even and odd lanes, in neighbouring banks; and a wave whose counted lanes all carry one bin (flat or clipped areas,
// where w_0 = 0) adds its lane count once.  The later passes count only the keys of one bin of the pass before.
//
// A workgroup keeps its histograms in LDS (2048 bins x 2 counters x 4 B = 16 KB per population; 1024 bins, 8 KB, in k_img_ns_hist,
// which only serves the 10-bit passes), walks over its share of the tiles, and at the end adds its non-empty bins to the global
// histogram with integer atomics.
//
// Route 1 (k_img_ns_recompute): every pass recomputes w_0 from the frame, a lane per pixel, the 5 x 5 neighbourhood read directly
// as in k_img_wv_scale.  No temporaries but the histogram and state block.
// Route 2 (k_img_ns_keys, then k_img_ns_hist twice): the first pass stages a 64 x 16 tile plus 2 pixels per side in LDS, in planes,
// through wv_fold (a position outside the picture holds the symmetric extension; a row outside it is then the row pass of the
// extension, which is what route 1 reads), runs the row pass into a fourth plane and the column pass into registers, channel by
// channel, writes the keys to a planar buffer (12 B per pixel "channel", 4 B "vector") and counts them.  The later passes read the
// keys.  LDS: 4 planes of 68 x 20 floats = 21 760 B and the histograms, 70 912 B "channel" (two workgroups per CU), 38 144 B "vector".
// Both routes form every key with the same inline functions in the same order: identical histograms, identical bits.
#include "ics_img_px.h"

namespace {

#define NSB0 11                                // bits of the first pass
#define NSB1 10                                // bits of the second and third
#define NSBINS (1 << NSB0)                     // bins of a population's histogram
#define NSLANES 256
#define NSTW 64                                // tile of route 2's first pass
#define NSTH 16
#define NSSW (NSTW + 4)                        // staged: 68 x 20
#define NSSH (NSTH + 4)
#define NSN (NSSW * NSSH)
#define NSPX (NSTW * NSTH / NSLANES)           // pixels per lane: 4
#define NSHK 4                                 // keys per lane and step of route 2's later passes
#define NSSTATE (3 * NSBINS)                   // state block behind the histograms: prefix[3], rank[3]

static_assert(NSTW == 64 && NSTH % (NSLANES / 64) == 0 && NSB0 + 2 * NSB1 == 31 && NSB1 <= NSB0 && NSBINS % NSLANES == 0 && (1 << NSB1) % NSLANES == 0, "bit split");

template <bool VEC>
__device__ __forceinline__ void ns_keys(const float cur[3], const float nxt[3], unsigned key[3]) {
  float w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = __fsub_rn(cur[c], nxt[c]);
  if (VEC) {   // as wv_detail<true>: the squares summed in ascending order, but an IEEE square root
    const float q0 = __fmul_rn(w[0], w[0]), q1 = __fmul_rn(w[1], w[1]), q2 = __fmul_rn(w[2], w[2]);
    const float lo = fminf(q0, q1), hi = fmaxf(q0, q1);
    // sqrtf is the correctly rounded root (the compiler's default for HIP code); __fsqrt_rn is the bare instruction here, within 1 ulp,
    // and a median that has to equal its restatement bit for bit cannot take that
    key[0] = __float_as_uint(sqrtf(__fadd_rn(__fadd_rn(fminf(lo, q2), fmaxf(lo, fminf(hi, q2))), fmaxf(hi, q2))));
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) key[c] = __float_as_uint(fabsf(w[c]));
  }
}

// one key into the LDS histogram h[NSBINS][2] of its population, if `on` and its bits above the field equal the prefix.  Called by
// all lanes of a wave together.
__device__ __forceinline__ void ns_count(unsigned* h, unsigned key, bool on, unsigned prefix, int shift, int bits) {
  on = on && (key >> (shift + bits)) == prefix;
  const unsigned bin = (key >> shift) & ((1u << bits) - 1u);
  const unsigned long long act = __ballot(on);
  if (!act) return;
  const int lane = threadIdx.x & 63, first = __ffsll((long long)act) - 1;
  const unsigned b0 = __shfl(bin, first);
  if (__ballot(on && bin == b0) == act) {
    if (lane == first) atomicAdd(&h[2 * b0], (unsigned)__popcll(act));
  } else if (on) {
    atomicAdd(&h[2 * bin + (lane & 1)], 1u);
  }
}

__device__ __forceinline__ void ns_zero(unsigned* h, int words) {
  for (int i = threadIdx.x; i < words; i += NSLANES) h[i] = 0u;
}

// the workgroup's non-empty bins, h[npop][hbins][2], into the global histograms g[npop][NSBINS]
__device__ __forceinline__ void ns_merge(const unsigned* h, int hbins, unsigned* g, int npop, int bits) {
  for (int i = threadIdx.x; i < (npop << bits); i += NSLANES) {
    const int p = i >> bits, b = i - (p << bits), k = p * hbins + b;
    const unsigned v = h[2 * k] + h[2 * k + 1];
    if (v) atomicAdd(&g[p * NSBINS + b], v);
  }
}

// ---- route 1, every pass: w_0 from the frame -----------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(NSLANES) void k_img_ns_recompute(const float* __restrict__ f, int H, int W, int shift, int bits, unsigned* __restrict__ blk) {
  constexpr int NPOP = VEC ? 1 : 3;
  __shared__ unsigned h[NPOP * NSBINS * 2];
  unsigned prefix[NPOP];
#pragma unroll
  for (int p = 0; p < NPOP; ++p) prefix[p] = blk[NSSTATE + p];
  ns_zero(h, NPOP * NSBINS * 2);
  __syncthreads();
  const int tx = (W + 63) / 64, tiles = tx * ((H + 3) / 4);
  const long L = 3L * W;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t / tx, x = (t - ty * tx) * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
    const bool on = x < W && y < H;
    unsigned key[3] = {0u, 0u, 0u};
    if (on) {
      int xs[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) xs[k] = 3 * wv_fold(x + k - 2, W);
      float hr[5][3], cur[3], nxt[3];
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const float* row = f + (long)wv_fold(y + r - 2, H) * L;
        float a[5][3];
#pragma unroll
        for (int k = 0; k < 5; ++k) ld3(row + xs[k], a[k]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          hr[r][c] = wv_pass(a[0][c], a[1][c], a[2][c], a[3][c], a[4][c]);
          if (r == 2) cur[c] = a[2][c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) nxt[c] = wv_pass(hr[0][c], hr[1][c], hr[2][c], hr[3][c], hr[4][c]);
      ns_keys<VEC>(cur, nxt, key);
    }
#pragma unroll
    for (int p = 0; p < NPOP; ++p) ns_count(h + p * NSBINS * 2, key[p], on, prefix[p], shift, bits);
  }
  __syncthreads();
  ns_merge(h, NSBINS, blk, NPOP, bits);
}

// ---- route 2, first pass: keys from an LDS tile, written to keys[NPOP][H W] and counted by their top NSB0 bits ---------------------------
template <bool VEC>
__global__ __launch_bounds__(NSLANES) void k_img_ns_keys(const float* __restrict__ f, int H, int W, unsigned* __restrict__ keys, unsigned* __restrict__ blk) {
  constexpr int NPOP = VEC ? 1 : 3;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sc = lds, *sh = lds + 3 * NSN;                                     // planes c[3][NSSH][NSSW], row pass [NSSH][NSSW]
  unsigned* h = reinterpret_cast<unsigned*>(lds + 4 * NSN);
  ns_zero(h, NPOP * NSBINS * 2);
  const int tx = (W + NSTW - 1) / NSTW, tiles = tx * ((H + NSTH - 1) / NSTH);
  const long L = 3L * W, n = (long)H * W;
  const int col = threadIdx.x & 63, row0 = threadIdx.x >> 6;                 // the lane's pixels: column col, rows row0 + 4 k of the tile
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t / tx, by = ty * NSTH, bx = (t - ty * tx) * NSTW;
    __syncthreads();                                                         // the histogram is zeroed; the tile before is done with
    for (int e = threadIdx.x; e < NSN; e += NSLANES) {
      const int ly = e / NSSW, lx = e - ly * NSSW;
      float v[3];
      ld3(f + (long)wv_fold(by - 2 + ly, H) * L + 3L * wv_fold(bx - 2 + lx, W), v);
#pragma unroll
      for (int c = 0; c < 3; ++c) sc[c * NSN + e] = v[c];
    }
    __syncthreads();
    float cur[NSPX][3], nxt[NSPX][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = sc + c * NSN;
      for (int e = threadIdx.x; e < NSSH * NSTW; e += NSLANES) {             // every staged row, the tile's columns
        const int i = (e >> 6) * NSSW + 2 + (e & 63);
        sh[i] = wv_pass(p[i - 2], p[i - 1], p[i], p[i + 1], p[i + 2]);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NSPX; ++k) {
        const int i = (2 + row0 + 4 * k) * NSSW + 2 + col;
        cur[k][c] = p[i];
        nxt[k][c] = wv_pass(sh[i - 2 * NSSW], sh[i - NSSW], sh[i], sh[i + NSSW], sh[i + 2 * NSSW]);
      }
      if (c < 2) __syncthreads();                                            // (after the last channel: the barrier at the loop's top)
    }
#pragma unroll
    for (int k = 0; k < NSPX; ++k) {
      const int y = by + row0 + 4 * k, x = bx + col;
      const bool on = y < H && x < W;
      unsigned key[3] = {0u, 0u, 0u};
      ns_keys<VEC>(cur[k], nxt[k], key);
#pragma unroll
      for (int p = 0; p < NPOP; ++p) {
        if (on) keys[p * n + (long)y * W + x] = key[p];
        ns_count(h + p * NSBINS * 2, key[p], on, 0u, 31 - NSB0, NSB0);
      }
    }
  }
  __syncthreads();
  ns_merge(h, NSBINS, blk, NPOP, NSB0);
}

// ---- route 2, later passes: the stored keys, NSHK per lane and step (independent loads in flight), histograms of 2^NSB1 bins ---------
template <bool VEC>
__global__ __launch_bounds__(NSLANES) void k_img_ns_hist(const unsigned* __restrict__ keys, long n, int shift, unsigned* __restrict__ blk) {
  constexpr int NPOP = VEC ? 1 : 3, NB = 1 << NSB1;
  __shared__ unsigned h[NPOP * NB * 2];
  unsigned prefix[NPOP];
#pragma unroll
  for (int p = 0; p < NPOP; ++p) prefix[p] = blk[NSSTATE + p];
  ns_zero(h, NPOP * NB * 2);
  __syncthreads();
  for (long i0 = (long)blockIdx.x * (NSLANES * NSHK); i0 < n; i0 += (long)gridDim.x * (NSLANES * NSHK)) {
    unsigned key[NSHK][NPOP];
#pragma unroll
    for (int k = 0; k < NSHK; ++k) {
      const long i = i0 + k * NSLANES + threadIdx.x;
#pragma unroll
      for (int p = 0; p < NPOP; ++p) key[k][p] = i < n ? keys[p * n + i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < NSHK; ++k) {
      const bool on = i0 + k * NSLANES + threadIdx.x < n;
#pragma unroll
      for (int p = 0; p < NPOP; ++p) ns_count(h + p * NB * 2, key[k][p], on, prefix[p], shift, NSB1);
    }
  }
  __syncthreads();
  ns_merge(h, NB, blk, NPOP, NSB1);
}

// ---- between the passes, one workgroup: the bin that holds the rank joins the prefix, the rank drops by the count below that bin, the
// histogram is left zeroed.  first: the rank is rank0 (the state block starts zeroed: prefix 0, which is what the first pass matches)
__global__ __launch_bounds__(NSLANES) void k_img_ns_select(unsigned* __restrict__ blk, int npop, int bits, unsigned rank0, int first) {
  __shared__ unsigned wsum[NSLANES / 64];
  const int per = (1 << bits) / NSLANES, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;      // 8 or 4 bins per lane
  for (int p = 0; p < npop; ++p) {
    unsigned* g = blk + p * NSBINS + threadIdx.x * per;
    const unsigned rank = first ? rank0 : blk[NSSTATE + 3 + p], prefix = blk[NSSTATE + p];
    unsigned v[NSBINS / NSLANES], s = 0u;
#pragma unroll
    for (int i = 0; i < NSBINS / NSLANES; ++i) {
      v[i] = 0u;
      if (i < per) { v[i] = g[i]; g[i] = 0u; }
      s += v[i];
    }
    unsigned incl = s;                                                       // inclusive scan of the lanes' sums: in the wave, then over the waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned below = incl - s;
    for (int w = 0; w < wave; ++w) below += wsum[w];
    if (below <= rank && rank - below < s) {                                 // exactly one lane: the counts sum to more than the rank
      unsigned c = below;
#pragma unroll
      for (int i = 0; i < NSBINS / NSLANES; ++i) {
        if (i < per && c <= rank && rank - c < v[i]) {
          blk[NSSTATE + p] = (prefix << bits) | (unsigned)(threadIdx.x * per + i);
          blk[NSSTATE + 3 + p] = rank - c;
        }
        c += v[i];
      }
    }
    __syncthreads();                                                         // wsum is reused by the next population
  }
}

}  // namespace

size_t ics_img_noise_block_words() { return NSSTATE + 6; }
size_t ics_img_noise_result_word() { return NSSTATE; }
size_t ics_img_noise_key_words(int H, int W, int coupling, int route) { return route == 2 ? (size_t)(coupling ? 1 : 3) * H * W : 0; }
size_t ics_img_noise_keys_lds(int coupling) { return (size_t)4 * NSN * sizeof(float) + (size_t)(coupling ? 1 : 3) * NSBINS * 2 * sizeof(unsigned); }

hipError_t ics_launch_img_noise(const float* f, int H, int W, int coupling, int route, int cus, unsigned* blk, unsigned* keys, hipStream_t s) {
  if ((route != 1 && route != 2) || !blk || (route == 2 && !keys) || H < 1 || W < 1) return hipErrorInvalidValue;
  const int npop = coupling ? 1 : 3;
  const long n = (long)H * W;
  const unsigned rank0 = (unsigned)((n - 1) / 2);
  // persistent workgroups, as many per CU as fit beside each other with their histograms: 49 152 B "channel" in k_img_ns_recompute,
  // 70 912 B in k_img_ns_keys, 24 576 B in k_img_ns_hist; no kernel needs more than 128 registers, four workgroups per CU
  const int rec_per_cu = coupling ? 4 : 3, keys_per_cu = coupling ? 4 : 2, hist_per_cu = 4;
  auto wgs = [&](long units, int per_cu) {
    long grid = (long)(cus > 0 ? cus : 256) * per_cu;
    if (units < grid) grid = units;
    if (const int m = ics_debug().max_wgs.load(std::memory_order_relaxed); m > 0 && grid > m) grid = m;   // test hook: several tiles per workgroup on small frames
    return dim3((unsigned)grid);
  };
  hipError_t e = hipMemsetAsync(blk, 0, ics_img_noise_block_words() * sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  const int shift[3] = {NSB1 + NSB1, NSB1, 0}, bits[3] = {NSB0, NSB1, NSB1};
  for (int pass = 0; pass < 3; ++pass) {
    if (route == 1) {
      const long tiles = (long)((W + 63) / 64) * ((H + 3) / 4);
      ICS_LAUNCH_VEC(coupling, k_img_ns_recompute, wgs(tiles, rec_per_cu), dim3(NSLANES), 0, s, f, H, W, shift[pass], bits[pass], blk);
    } else if (pass == 0) {
      const size_t lds = ics_img_noise_keys_lds(coupling);
      e = coupling ? set_dynamic_lds(k_img_ns_keys<true>, lds) : set_dynamic_lds(k_img_ns_keys<false>, lds);
      if (e != hipSuccess) return e;
      const long tiles = (long)((W + NSTW - 1) / NSTW) * ((H + NSTH - 1) / NSTH);
      ICS_LAUNCH_VEC(coupling, k_img_ns_keys, wgs(tiles, keys_per_cu), dim3(NSLANES), lds, s, f, H, W, keys, blk);
    } else {
      ICS_LAUNCH_VEC(coupling, k_img_ns_hist, wgs((n + NSLANES * NSHK - 1) / (NSLANES * NSHK), hist_per_cu), dim3(NSLANES), 0, s, keys, n, shift[pass], blk);
    }
    hipLaunchKernelGGL(k_img_ns_select, dim3(1), dim3(NSLANES), 0, s, blk, npop, bits[pass], rank0, pass == 0);
  }
  return hipGetLastError();
}
