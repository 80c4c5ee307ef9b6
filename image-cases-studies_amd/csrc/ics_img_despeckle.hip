// ics_img_despeckle.hip -- thresholded median ("despeckle") of device-resident images (ics_img_despeckle, include/ics_hip.h): H x W x 3
// float32, HWC, contiguous.  Removes impulses (hot and dead pixels, salt and pepper, NaN / inf) and nothing else; threshold 0 is the
// plain median filter.
//
//   key      of a value with bits b: b ^ 0xFFFFFFFF if the sign bit is set, else b | 0x80000000 (ds_key): unsigned integers that order
//            like the floats, -0 below +0, NaNs at the two ends by sign.  Every selection is made on the keys, never by a float compare.
//   window   of (y, x): the (2 r + 1)^2 pixels at (clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)), r = 1 or 2: n = 9 or 25 values
//   med_c    the key of rank (n - 1) / 2 of channel c of the window: one of the input values, bit for bit
//   d_c      = |I_c - med_c| (one float32 subtraction), hit_c = !(d_c <= t_c): a NaN difference is a hit
//   channel  out_c = hit_c ? med_c : I_c; replaced[c] counts hit_c
//   vector   hit = hit_0 || hit_1 || hit_2 with the one threshold t_0; all three channels of a hit pixel become their medians;
//            replaced[0] counts the hit pixels                                                                            (ds_strip)
//
// Selection (registers only, fully unrolled exchanges min / max on the keys, static indices).  A lane forms DSP = 4 vertically
// neighbouring outputs of one column, in strips of Q = 4 (r = 1), 2 (r = 2, route 2) or 1 (r = 2, route 1): 4 at a time at r = 2
// would need 164 to 170 registers.  The windows of a strip share rows, so each of its Q + 2 r window rows is sorted once (3 or 9
// exchanges: ds_sort) and serves up to Q outputs.
//   r = 1  from three sorted rows (lo, mid, hi each): med3(max of the lo, med3 of the mid, min of the hi).
//   r = 2  the five sorted rows of a window are sorted along the columns too (5 x 9 exchanges): the 5 x 5 block then ascends both
//          ways, the entry (a, b) (from 1) has at least a b - 1 entries that precede it and (6 - a)(6 - b) - 1 that follow it (ties
//          broken by position), so an entry with a b >= 14 or (6 - a)(6 - b) >= 14 is not the one of rank 12.  Six are excluded
//          on either side; the median of the 25 is the median of the 13 that remain, found by forgetful selection (ds_forget: of
//          8 values drop the smallest and the largest, take in the next, ... until 3 remain).
//
// Route 1 (k_img_ds_direct): a workgroup is one wave, 64 columns x DSP rows; a lane reads its window rows from the frame itself
// through the caches, a channel at a time.  No LDS; the counts are reduced in the wave by ballots.
// Route 2 (k_img_ds_tile): a workgroup of 256 lanes stages the keys of its DST x DST = 32 x 32 output tile plus an r halo once in
// LDS, at the clamped coordinates (an edge needs nothing special afterwards), in three planes of (DST + 2 r)^2 words; lane
// (lx, gy) reads rows 4 gy .. 4 gy + 3 + 2 r at columns lx .. lx + 2 r: the 32 lanes of a half-wave read 32 consecutive words,
// whatever the row stride, so no read has a bank conflict.  Static LDS 4 (3 (DST + 2 r)^2 + 3) bytes: 13 884 at r = 1, 15 564 at
// r = 2 (the last three words: the workgroup's counters).
// Both routes call ds_lane with another reader: identical bits.  Counts: per wave by ballots, per workgroup in LDS (route 2), then
// one atomicAdd on unsigned per workgroup and non-zero counter into the three words `cnt`, which the caller has zeroed: integer sums, any order.
// Registers: capped at 128 by __launch_bounds__(.., DSWGS = 4) (four waves per SIMD: four workgroups of 256 lanes per CU); no scratch.
#include "ics_img_px.h"

namespace {

#define DST 32                         // output tile edge of route 2
#define DSP 4                          // vertically neighbouring outputs of a lane
#define DSLANES 256                    // DST * (DST / DSP)
#define DSWAVE 64                      // route 1: one wave per workgroup, DSWAVE columns x DSP rows
#define DSWGS 4                        // waves per SIMD the register budget leaves room for (128 registers)

static_assert(DST * (DST / DSP) == DSLANES && DST % DSP == 0 && ICS_IMG_DESPECKLE_MAX_RADIUS == 2, "tile");

// (__host__ as well: tools/check_despeckle_select.hip runs the key order and the networks below on the CPU, on every 0-1 input)
__host__ __device__ __forceinline__ unsigned ds_key(unsigned b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__host__ __device__ __forceinline__ unsigned ds_bits(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

__host__ __device__ __forceinline__ unsigned ds_lo(unsigned a, unsigned b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ unsigned ds_hi(unsigned a, unsigned b) { return a < b ? b : a; }
__host__ __device__ __forceinline__ unsigned ds_med3(unsigned a, unsigned b, unsigned c) { return ds_hi(ds_lo(a, b), ds_lo(ds_hi(a, b), c)); }
__host__ __device__ __forceinline__ void ds_cx(unsigned& a, unsigned& b) {
  const unsigned lo = ds_lo(a, b);
  b = ds_hi(a, b);
  a = lo;
}

// ascending, 3 (D = 3) or 9 (D = 5) exchanges
template <int D>
__host__ __device__ __forceinline__ void ds_sort(unsigned* v) {
  if constexpr (D == 3) {
    ds_cx(v[0], v[1]); ds_cx(v[1], v[2]); ds_cx(v[0], v[1]);
  } else {
    static_assert(D == 5, "window edge");
    ds_cx(v[0], v[1]); ds_cx(v[3], v[4]); ds_cx(v[2], v[4]); ds_cx(v[2], v[3]); ds_cx(v[1], v[4]);
    ds_cx(v[0], v[3]); ds_cx(v[0], v[2]); ds_cx(v[1], v[3]); ds_cx(v[1], v[2]);
  }
}

// the smallest of w[0 .. M) to w[0], the largest to w[M - 1]
template <int M>
__host__ __device__ __forceinline__ void ds_minmax(unsigned* w) {
#pragma unroll
  for (int i = 0; i < M / 2; ++i) ds_cx(w[i], w[M - 1 - i]);
#pragma unroll
  for (int i = 1; i <= (M - 1) / 2; ++i) ds_cx(w[0], w[i]);
#pragma unroll
  for (int i = M / 2; i < M - 1; ++i) ds_cx(w[i], w[M - 1]);
}

// forgetful selection: the median of the M values in w and the LEFT values in rest, M = LEFT + 3: neither the smallest nor the
// largest of w can be it, both are dropped and the next value taken in
template <int M, int LEFT>
__host__ __device__ __forceinline__ unsigned ds_forget(unsigned* w, const unsigned* rest) {
  static_assert(M == LEFT + 3, "working set");
  ds_minmax<M>(w);
  if constexpr (LEFT == 0) {
    return w[1];
  } else {
    w[0] = rest[0];
    return ds_forget<M - 1, LEFT - 1>(w, rest + 1);
  }
}

// the key of rank (n - 1) / 2 of the window whose 2 R + 1 rows, each sorted, start at w
template <int R>
__host__ __device__ __forceinline__ unsigned ds_median(const unsigned (*w)[2 * R + 1]) {
  if constexpr (R == 1) {
    return ds_med3(ds_hi(ds_hi(w[0][0], w[1][0]), w[2][0]), ds_med3(w[0][1], w[1][1], w[2][1]), ds_lo(ds_lo(w[0][2], w[1][2]), w[2][2]));
  } else {
    unsigned m[5][5];
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      unsigned col[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) col[a] = w[a][b];
      ds_sort<5>(col);
#pragma unroll
      for (int a = 0; a < 5; ++a) m[a][b] = col[a];
    }
    // (a + 1)(b + 1) <= 13 and (5 - a)(5 - b) <= 13
    unsigned v[8] = {m[0][3], m[0][4], m[1][2], m[1][3], m[1][4], m[2][1], m[2][2], m[2][3]};
    const unsigned rest[5] = {m[3][0], m[3][1], m[3][2], m[4][0], m[4][1]};
    return ds_forget<8, 5>(v, rest);
  }
}

// Q neighbouring outputs of a lane.  key(c, j, k): the key of channel c at row j (0 .. Q + 2 R) and column k (0 .. 2 R + 1) of their
// block of window rows; output i has its centre at (i + R, R).  outb: the result's bits; hit: what `replaced` counts.
template <int R, bool VEC, int Q, typename Key>
__device__ __forceinline__ void ds_strip(Key key, const float t[3], unsigned outb[Q][3], bool hit[Q][3]) {
  constexpr int D = 2 * R + 1;
  unsigned ctr[Q][3], med[Q][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    unsigned row[Q + 2 * R][D];
    auto take = [&](int j) {                                             // window row j: read, its centre kept, sorted
#pragma unroll
      for (int k = 0; k < D; ++k) row[j][k] = key(c, j, k);
      if (j >= R && j < R + Q) ctr[j - R][c] = row[j][R];
      ds_sort<D>(row[j]);
    };
#pragma unroll
    for (int j = 0; j < 2 * R; ++j) take(j);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      take(i + 2 * R);
      med[i][c] = ds_median<R>(row + i);
      if (R == 2) __builtin_amdgcn_sched_barrier(0);                     // one 5 x 5 selection at a time
    }
  }
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    bool h[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float I = __uint_as_float(ds_bits(ctr[i][c])), m = __uint_as_float(ds_bits(med[i][c]));
      h[c] = !(fabsf(__fsub_rn(I, m)) <= t[VEC ? 0 : c]);
    }
    if (VEC) h[0] = h[1] = h[2] = h[0] || h[1] || h[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      outb[i][c] = ds_bits(h[c] ? med[i][c] : ctr[i][c]);
      hit[i][c] = h[c];
    }
  }
}

// outputs of a strip: DSP at r = 1; at r = 2 a strip of 4 would need 164 to 170 registers: route 2 takes two strips of 2 one after the
// other (122), route 1, which also holds its addresses, four of 1
template <int R, int ROUTE> struct ds_q { static constexpr int Q = R == 1 ? DSP : ROUTE; };

// The DSP outputs of a lane at column x, rows y0 .. y0 + DSP - 1, key(c, j, k) over the lane's DSP + 2 R window rows: the results
// inside the picture written, n[c] = this wave's count of counter c (the same in all lanes)
template <int R, bool VEC, int Q, typename Key>
__device__ __forceinline__ void ds_lane(Key key, const float t[3], float* __restrict__ out, int H, int W, int x, int y0, unsigned n[3]) {
  static_assert(DSP % Q == 0, "strips");
  n[0] = n[1] = n[2] = 0u;
  auto strip = [&](int q) {
    unsigned outb[Q][3];
    bool hit[Q][3];
    ds_strip<R, VEC, Q>([&](int c, int j, int k) { return key(c, q + j, k); }, t, outb, hit);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const int y = y0 + q + i;
      const bool on = x < W && y < H;
      if (on) {
        const float o[3] = {__uint_as_float(outb[i][0]), __uint_as_float(outb[i][1]), __uint_as_float(outb[i][2])};
        st3(out + ((long)y * W + x) * 3, o);
      }
#pragma unroll
      for (int c = 0; c < (VEC ? 1 : 3); ++c) n[c] += (unsigned)__popcll(__ballot(on && hit[i][c]));
    }
  };
  if constexpr (Q == 1) {                                                // a loop the compiler keeps: one output's registers
#pragma unroll 1
    for (int q = 0; q < DSP; ++q) strip(q);
  } else {
#pragma unroll
    for (int q = 0; q < DSP; q += Q) {
      strip(q);
      if (Q < DSP) __builtin_amdgcn_sched_barrier(0);
    }
  }
}

__device__ __forceinline__ int ds_clamp(int i, int n) { return min(max(i, 0), n - 1); }

// ---- route 1: the window rows from the frame ------------------------------------------------------------------------------------------
template <int R, bool VEC>
__global__ __launch_bounds__(DSWAVE, DSWGS) void k_img_ds_direct(const float* __restrict__ src, float* __restrict__ out, int H, int W, float t0, float t1,
                                                                 float t2, unsigned* __restrict__ cnt) {
  constexpr int D = 2 * R + 1;
  const int tx = (W + DSWAVE - 1) / DSWAVE, ty = blockIdx.x / tx;
  const int x = (blockIdx.x - ty * tx) * DSWAVE + threadIdx.x, y0 = ty * DSP;
  const long L = 3L * W;
  unsigned xo[D];                                                        // a row's address is the same in all lanes: one 32-bit offset per column
#pragma unroll
  for (int k = 0; k < D; ++k) xo[k] = 3u * (unsigned)ds_clamp(x - R + k, W);       // (a lane past the last column reads that column and writes nothing)
  auto key = [&](int c, int j, int k) {
    const float* row = src + (long)ds_clamp(y0 - R + j, H) * L;
    return ds_key(__float_as_uint(row[xo[k] + (unsigned)c]));
  };
  const float t[3] = {t0, t1, t2};
  unsigned n[3];
  ds_lane<R, VEC, ds_q<R, 1>::Q>(key, t, out, H, W, x, y0, n);
  const unsigned mine = threadIdx.x == 0 ? n[0] : threadIdx.x == 1 ? n[1] : n[2];
  if (threadIdx.x < (VEC ? 1 : 3) && mine) atomicAdd(&cnt[threadIdx.x], mine);
}

// ---- route 2: the keys of the tile and its halo staged in LDS -------------------------------------------------------------------------
template <int R, bool VEC>
__global__ __launch_bounds__(DSLANES, DSWGS) void k_img_ds_tile(const float* __restrict__ src, float* __restrict__ out, int H, int W, float t0, float t1,
                                                                float t2, unsigned* __restrict__ cnt) {
  constexpr int S = DST + 2 * R, NS = S * S;
  __shared__ unsigned lds[3 * NS + 3];
  unsigned* wc = lds + 3 * NS;
  const int tx = (W + DST - 1) / DST, ty = blockIdx.x / tx;
  const int ty0 = ty * DST, tx0 = (blockIdx.x - ty * tx) * DST;
  const long L = 3L * W;
  if (threadIdx.x < 3) wc[threadIdx.x] = 0u;
  for (int e = threadIdx.x; e < NS; e += DSLANES) {
    const int ly = e / S, lx = e - ly * S;
    float v[3];
    ld3(src + (long)ds_clamp(ty0 - R + ly, H) * L + 3L * ds_clamp(tx0 - R + lx, W), v);
#pragma unroll
    for (int c = 0; c < 3; ++c) lds[c * NS + e] = ds_key(__float_as_uint(v[c]));
  }
  __syncthreads();
  const int lx = threadIdx.x & (DST - 1), gy = threadIdx.x / DST;
  const unsigned* base = lds + gy * DSP * S + lx;
  auto key = [&](int c, int j, int k) { return base[c * NS + j * S + k]; };
  const float t[3] = {t0, t1, t2};
  unsigned n[3];
  ds_lane<R, VEC, ds_q<R, 2>::Q>(key, t, out, H, W, tx0 + lx, ty0 + gy * DSP, n);
  const int lane = threadIdx.x & 63;
  const unsigned mine = lane == 0 ? n[0] : lane == 1 ? n[1] : n[2];
  if (lane < (VEC ? 1 : 3) && mine) atomicAdd(&wc[lane], mine);
  __syncthreads();
  if (threadIdx.x < (VEC ? 1 : 3) && wc[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], wc[threadIdx.x]);
}

template <int R, bool VEC>
void ds_launch(int route, const float* src, float* out, int H, int W, const float t[3], unsigned* cnt, hipStream_t s) {
  if (route == 1) {
    const long wgs = (long)((W + DSWAVE - 1) / DSWAVE) * ((H + DSP - 1) / DSP);
    hipLaunchKernelGGL((k_img_ds_direct<R, VEC>), dim3((unsigned)wgs), dim3(DSWAVE), 0, s, src, out, H, W, t[0], t[1], t[2], cnt);
  } else {
    const long wgs = (long)((W + DST - 1) / DST) * ((H + DST - 1) / DST);
    hipLaunchKernelGGL((k_img_ds_tile<R, VEC>), dim3((unsigned)wgs), dim3(DSLANES), 0, s, src, out, H, W, t[0], t[1], t[2], cnt);
  }
}

}  // namespace

hipError_t ics_launch_img_despeckle(const float* src, int H, int W, int radius, const float t[3], int coupling, int route, float* out, unsigned* cnt,
                                    hipStream_t s) {
  if (radius < 1 || radius > ICS_IMG_DESPECKLE_MAX_RADIUS || (route != 1 && route != 2) || !cnt || H < 1 || W < 1 || W > (1 << 28)) return hipErrorInvalidValue;
  if ((long)((W + DSWAVE - 1) / DSWAVE) * ((H + DSP - 1) / DSP) > 0x7fffffffL) return hipErrorInvalidValue;      // (one-dimensional grids)
  if (radius == 1) {
    if (coupling) ds_launch<1, true>(route, src, out, H, W, t, cnt, s); else ds_launch<1, false>(route, src, out, H, W, t, cnt, s);
  } else {
    if (coupling) ds_launch<2, true>(route, src, out, H, W, t, cnt, s); else ds_launch<2, false>(route, src, out, H, W, t, cnt, s);
  }
  return hipGetLastError();
}
