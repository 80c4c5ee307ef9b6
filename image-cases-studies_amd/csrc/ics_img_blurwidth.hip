// ics_img_blurwidth.hip -- derivative autocorrelation of device-resident images (ics_img_blur_profile, include/ics_hip.h): H x W x 3
// float32, HWC, contiguous.  The two profiles from which the host reads the blur width (lib/_native.py blur_extent).
//
//   Y        = (R + G + B) * (1 / 3), every operation rounded once (no FMA)
//   dx[y,x]  = Y[y,x+1] - Y[y,x], dy[y,x] = Y[y+1,x] - Y[y,x], both pixels inside the window [y0, y1) x [x0, x1)
//   Sx(l)    = sum over the window of dx[y,x] dx[y,x+l], Sy(l) = sum of dy[y,x] dy[y+l,x], l = 0 .. L, every pair inside the window
//   Ax(l)    = Sx(l) / nx(l), nx(l) = (y1 - y0) max(x1 - x0 - 1 - l, 0); Ay, ny likewise; 0 where the count is 0
//
// k_img_bw_partial: persistent workgroups of 256 lanes walk the ACTH x ACTW tiles of the window's pixel grid (position (y, x) carries
// dx[y,x] and dy[y,x]).  A tile stages the luma twice in LDS, each plane at one pitch: the x plane, ACTH rows of ACTW + L + 1 columns at the pitch of the largest lag
// (the tile and what lies right of it), and the y plane, ACTH + L + 1 rows of ACTW columns (the tile and what lies below it).  The
// coordinates are clamped to the window, so a difference whose second pixel lies outside the window is Y - Y = 0 and a pair that
// reaches outside contributes nothing without a test per product; what clamping repeats across the axis (rows below the window in
// the x plane, columns right of it in the y plane) is cut by zeroing the lane's own differences there.  A lane owns column tid % 64
// and the rows tid / 64 + 4 k, k < 8: a wave reads 64 consecutive floats of one LDS row at every step.  It keeps its eight own
// differences in registers and slides over the lags in chunks of ACTCH: per lag and value one LDS read, one subtraction (the read
// before it is the other operand), one product, one sum.  The ACTCH sums of a chunk are reduced over the wave by a halving exchange
// (at every step a lane hands half of its sums to its partner and adds what it receives to the other half: 4 + 2 + 1 + 1 + 1 + 1
// exchanges), the four waves' sums wait in LDS, and after both axes lane o adds the four in wave order and stores partial o of the
// tile: float32 in one fixed order, no atomics.  partial[tile][axis][lag].
// k_img_bw_reduce: one workgroup, a lane per (axis, lag): the tile partials summed in tile order in double, divided by the pair count.
#include "ics_img_px.h"

namespace {

#define ACTW 64                                // tile: difference values per row ...
#define ACTH 32                                // ... and rows
#define ACTLANES 256
#define ACTPX (ACTW * ACTH / ACTLANES)         // values per lane: 8
#define ACTCH 8                                // lags per chunk: the sums a lane holds at once
#define ACTWAVES (ACTLANES / 64)
#define ACTSX (ACTW + ICS_IMG_BLURWIDTH_MAX_LAG + 1)   // pitch of the x plane: a constant, so that every LDS offset of a lane is an immediate

static_assert(ACTW == 64 && ACTH % ACTWAVES == 0 && ACTPX * ACTWAVES == ACTH && ACTCH == 8, "lane layout");

__device__ __forceinline__ float bw_luma(const float* __restrict__ p) {
  float v[3];
  ld3(p, v);
  return px_luma(v);
}

// the halving exchange: ACTCH sums per lane in, the sum over the wave of sum number bw_wave_slot(lane) out, in every lane
__device__ __forceinline__ float bw_wave_sum(const float a[ACTCH], int lane) {
  float b[4], c[2];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = __fadd_rn(h5 ? a[i + 4] : a[i], __shfl_xor(h5 ? a[i] : a[i + 4], 32));
#pragma unroll
  for (int i = 0; i < 2; ++i) c[i] = __fadd_rn(h4 ? b[i + 2] : b[i], __shfl_xor(h4 ? b[i] : b[i + 2], 16));
  float e = __fadd_rn(h3 ? c[1] : c[0], __shfl_xor(h3 ? c[0] : c[1], 8));
  e = __fadd_rn(e, __shfl_xor(e, 4));
  e = __fadd_rn(e, __shfl_xor(e, 2));
  return __fadd_rn(e, __shfl_xor(e, 1));
}
__device__ __forceinline__ int bw_wave_slot(int lane) { return ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1); }

// the sums of lags l0 .. l0 + ACTCH - 1 over the lane's values (TAIL: of those up to L, 0 beyond); prev: the luma read last per value
template <bool TAIL>
__device__ __forceinline__ void bw_chunk(const float* p, int kstep, int lstep, const float own[ACTPX], float prev[ACTPX], int l0, int L, float acc[ACTCH]) {
#pragma unroll
  for (int j = 0; j < ACTCH; ++j) {
    acc[j] = 0.f;
    if (!TAIL || l0 + j <= L) {
#pragma unroll
      for (int k = 0; k < ACTPX; ++k) {
        const float cur = p[k * kstep + (l0 + j + 1) * lstep];
        acc[j] = __fadd_rn(acc[j], __fmul_rn(own[k], __fsub_rn(cur, prev[k])));
        prev[k] = cur;
      }
    }
    // the ACTCH * ACTPX reads are independent of each other: left alone the scheduler hoists all of them and the kernel needs more
    // than 128 registers.  Two lags' reads in flight are enough beside three other waves per SIMD.
    if (j & 1) __builtin_amdgcn_sched_barrier(0);
  }
}

// one axis of one tile: p = the lane's first value in the plane, kstep = floats between its values, lstep = floats per lag; on[k]: the
// value counts.  ws[lag][wave] receives the wave's sums.
__device__ __forceinline__ void bw_axis(const float* p, int kstep, int lstep, const bool on[ACTPX], int L, float* ws, int lane, int wave) {
  float own[ACTPX], prev[ACTPX];
#pragma unroll
  for (int k = 0; k < ACTPX; ++k) {
    prev[k] = p[k * kstep];
    own[k] = on[k] ? __fsub_rn(p[k * kstep + lstep], prev[k]) : 0.f;
  }
  for (int l0 = 0; l0 <= L; l0 += ACTCH) {
    float acc[ACTCH];
    if (l0 + ACTCH - 1 <= L) {
      bw_chunk<false>(p, kstep, lstep, own, prev, l0, L, acc);
    } else {
      bw_chunk<true>(p, kstep, lstep, own, prev, l0, L, acc);                // (the planes end at lag L)
    }
    const float s = bw_wave_sum(acc, lane);
    const int l = l0 + bw_wave_slot(lane);
    if ((lane & 7) == 0 && l <= L) ws[l * ACTWAVES + wave] = s;
  }
}

// (four workgroups per CU at small lags: 128 registers)
__global__ __launch_bounds__(ACTLANES) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_img_bw_partial(const float* __restrict__ f, int W, int y0, int y1, int x0, int x1, int L,
                                                            float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int SX = ACTW + L + 1, RY = ACTH + L + 1;                           // columns of the x plane in use, rows of the y plane
  float *px = lds, *py = lds + ACTH * ACTSX, *ws = py + RY * ACTW;          // x plane [ACTH][ACTSX], y plane [RY][ACTW], wave sums [2][L + 1][ACTWAVES]
  const int tx = (x1 - x0 + ACTW - 1) / ACTW, tiles = tx * ((y1 - y0 + ACTH - 1) / ACTH);
  const long pitch = 3L * W;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    // what a lane derives from its number is derived again for every tile, and once more for the stores: kept across the lag loops
    // these values are what pushes the kernel over 128 registers
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int col = tid & 63, row0 = tid >> 6;
    const int ty = t / tx, by = y0 + ty * ACTH, bx = x0 + (t - ty * tx) * ACTW;
    __syncthreads();                                                         // the tile before is done with
    // (loops of a fixed inner count, ACTPX or four loads in flight, and no unrolling beyond that: the remainders of the compiler's own
    //  unrolling cost more registers than the kernel has to spare at four workgroups per CU)
#pragma nounroll
    for (int c = col; c < SX; c += 64) {
      const long xo = 3L * min(bx + c, x1 - 1);
#pragma unroll
      for (int k = 0; k < ACTPX; ++k) {
        const int r = row0 + ACTWAVES * k;
        px[r * ACTSX + c] = bw_luma(f + (long)min(by + r, y1 - 1) * pitch + xo);
      }
    }
    const long xc = 3L * min(bx + col, x1 - 1);
#pragma nounroll
    for (int rb = row0; rb < RY; rb += 4 * ACTWAVES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = rb + ACTWAVES * i;
        if (r < RY) py[r * ACTW + col] = bw_luma(f + (long)min(by + r, y1 - 1) * pitch + xc);
      }
    }
    __syncthreads();
    bool onx[ACTPX], ony[ACTPX];
#pragma unroll
    for (int k = 0; k < ACTPX; ++k) {
      onx[k] = by + row0 + ACTWAVES * k < y1;
      ony[k] = bx + col < x1;
    }
    bw_axis(px + row0 * ACTSX + col, ACTWAVES * ACTSX, 1, onx, L, ws, col, row0);
    bw_axis(py + row0 * ACTW + col, ACTWAVES * ACTW, ACTW, ony, L, ws + (L + 1) * ACTWAVES, col, row0);
    __syncthreads();
    float* out = partial + (long)t * (2 * (L + 1));
    int o0 = threadIdx.x;
    asm volatile("" : "+v"(o0));
#pragma nounroll
    for (int o = o0; o < 2 * (L + 1); o += ACTLANES) {
      const float* w = ws + o * ACTWAVES;
      out[o] = __fadd_rn(__fadd_rn(__fadd_rn(w[0], w[1]), w[2]), w[3]);
    }
  }
}

// a lane per (axis, lag): result[axis][lag] = (sum over the tiles in tile order, double) / pairs
__global__ __launch_bounds__(512) void k_img_bw_reduce(const float* __restrict__ partial, int tiles, int hw, int ww, int L, double* __restrict__ result) {
  const int o = threadIdx.x, n = 2 * (L + 1);
  if (o >= n) return;
  const int axis = o > L, l = axis ? o - (L + 1) : o;
  double s = 0.0;
  int t = 0;
  for (; t + 8 <= tiles; t += 8) {                                          // eight loads in flight, added in tile order
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = partial[(long)(t + i) * n + o];
#pragma unroll
    for (int i = 0; i < 8; ++i) s = __dadd_rn(s, (double)v[i]);
  }
  for (; t < tiles; ++t) s = __dadd_rn(s, (double)partial[(long)t * n + o]);
  const long along = (axis ? hw : ww) - 1 - l, pairs = along > 0 ? along * (axis ? ww : hw) : 0;
  result[o] = pairs > 0 ? __ddiv_rn(s, (double)pairs) : 0.0;
}

}  // namespace

size_t ics_img_blurwidth_lds(int L) { return ((size_t)ACTH * ACTSX + (size_t)(ACTH + L + 1) * ACTW + (size_t)2 * (L + 1) * ACTWAVES) * sizeof(float); }
long ics_img_blurwidth_tiles(int hw, int ww) { return (long)((ww + ACTW - 1) / ACTW) * ((hw + ACTH - 1) / ACTH); }
size_t ics_img_blurwidth_partial_floats(int hw, int ww, int L) { return (size_t)ics_img_blurwidth_tiles(hw, ww) * 2 * (L + 1); }

hipError_t ics_launch_img_blurwidth(const float* f, int H, int W, int y0, int y1, int x0, int x1, int L, int cus, float* partial, double* result, hipStream_t s) {
  if (!f || !partial || !result || y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1 || L < 0 || L > ICS_IMG_BLURWIDTH_MAX_LAG) return hipErrorInvalidValue;
  const long tiles = ics_img_blurwidth_tiles(y1 - y0, x1 - x0);
  if (tiles > 0x7fffffffL / (2 * (L + 1))) return hipErrorInvalidValue;
  const size_t lds = ics_img_blurwidth_lds(L);
  // persistent workgroups, as many per CU as their LDS lets stand beside each other (160 KB; two at L = 128), four at most: the
  // kernel stays below 128 registers
  int per_cu = (int)((size_t)160 * 1024 / lds);
  per_cu = per_cu > 4 ? 4 : per_cu;
  long grid = (long)(cus > 0 ? cus : 256) * per_cu;
  if (const int m = ics_debug().max_wgs.load(std::memory_order_relaxed); m > 0 && grid > m) grid = m;   // test hook: several tiles per workgroup on small frames
  if (grid > tiles) grid = tiles;
  hipError_t e = set_dynamic_lds(k_img_bw_partial, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_bw_partial, dim3((unsigned)grid), dim3(ACTLANES), lds, s, f, W, y0, y1, x0, x1, L, partial);
  hipLaunchKernelGGL(k_img_bw_reduce, dim3(1), dim3((unsigned)((2 * (L + 1) + 63) / 64 * 64)), 0, s, partial, (int)tiles, y1 - y0, x1 - x0, L, result);
  return hipGetLastError();
}
