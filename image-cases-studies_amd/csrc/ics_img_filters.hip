// ics_img_filters.hip -- the lib/utils.py filters (Gaussian / Bessel blur, USM, bilateral) on device-resident images
// (ics_img_convolve / ics_img_usm / ics_img_bilateral, include/ics_hip.h): H x W x 3 float32, HWC, contiguous.  Same semantics as
// the float64 per-channel kernels of ics_filters.hip (k_conv2d_tile, k_bilateral_tile); float32 arithmetic, FMA accumulation in
// a fixed order, so two runs give identical bits.
//
// Layout: the channels are filtered independently, so a row is treated as ONE flat axis of L = 3 W floats on which a horizontal
// tap is a stride of 3 floats and a vertical tap a stride of L.  A 256-thread workgroup owns 256 flat floats (one wave-wide
// row of 16-byte accesses) x 16 or 32 rows; the tile plus its halo is staged once in LDS with the symmetric extension
// (... x1 x0 | x0 x1 ...) resolved at load time: interior quads by one 16-byte global load (4-byte aligned: a row of 3 W floats
// starts on a 16-byte boundary only when W % 4 == 0) and one ds_write_b128, border quads element by element through symf().
// Every lane then produces 4 consecutive flat outputs and stores them with one 16-byte store.
//
// LDS traffic: the row taps of a lane are the floats [4t + 3u, 4t + 3u + 3] of its LDS row, u = 0 .. KW-1.  Four taps span 13
// floats = the quad carried over from the previous group + 3 new ALIGNED quads, so a lane issues 3 ds_read_b128 per 16 FMAs,
// lanes 16 bytes apart (conflict-free), instead of 16 stride-4 ds_read_b32 (4-way bank conflicts).  The column taps read one
// aligned quad per tap.  The bilateral filter needs the unaligned floats 4t + 3j + i one at a time; its tile is stored with one
// pad float per 32 (position i + i / 32), which spreads the stride-4 lanes of a ds_read_b32 group over all 32 banks.
//
// Occupancy against LDS (160 KB per CU): 15 taps -> row pass 16 x 308 x 4 = 19 KB (8 workgroups = 32 waves per CU), column pass
// 46 x 256 x 4 = 46 KB (3 workgroups); bilateral radius 5 -> 26 x 296 x 4 = 30 KB (5 workgroups).
#include "ics_img_px.h"

namespace {

#define FT 256   // flat floats per tile row: 64 lanes x 4
#define RT 16    // tile rows of the row / 2-D pass and of the bilateral filter
#define VT 32    // tile rows of the column pass

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };   // 16-byte access at 4-byte alignment

// flat index 3 x + c of the symmetric extension of a W-pixel row
__device__ __forceinline__ int symf(int g, int W) {
  const int px = g >= 0 ? g / 3 : -((2 - g) / 3);
  return 3 * symm(px, W) + (g - 3 * px);
}
__device__ __forceinline__ int swz(int i) { return i + (i >> 5); }

// LDS row r, position p  <-  ext[ys + r][fb + p], p < 4 nq
template <bool SWZ>
__device__ __forceinline__ void stage_tile(float* tile, int stride, const float* __restrict__ src, int H, int W, int ys, int fb, int rows, int nq) {
  const int L = 3 * W;
  for (int e = threadIdx.x; e < rows * nq; e += 256) {
    const int r = e / nq, v = e - r * nq;
    const float* g = src + (long)symm(ys + r, H) * L;
    const int f = fb + 4 * v;
    float4 x;
    if (f >= 0 && f + 3 < L) {
      const f4u q = *reinterpret_cast<const f4u*>(g + f);
      x = make_float4(q.x, q.y, q.z, q.w);
    } else {
      x = make_float4(g[symf(f, W)], g[symf(f + 1, W)], g[symf(f + 2, W)], g[symf(f + 3, W)]);
    }
    float* d = tile + r * stride;
    if (SWZ) {
      const int p = swz(4 * v);     // (a quad never straddles a group of 32)
      d[p] = x.x; d[p + 1] = x.y; d[p + 2] = x.z; d[p + 3] = x.w;
    } else {
      *reinterpret_cast<float4*>(d + 4 * v) = x;
    }
  }
}

// acc[i] += sum_u w[u] * lp[3 u + i], u ascending; lp = LDS row + 4 * lane (16-byte aligned)
__device__ __forceinline__ void row_taps(const float* lp, const float* __restrict__ w, int KW, float acc[4]) {
  float4 c = *reinterpret_cast<const float4*>(lp);
  for (int u0 = 0; u0 < KW; u0 += 4) {
    const float4 n1 = *reinterpret_cast<const float4*>(lp + 4), n2 = *reinterpret_cast<const float4*>(lp + 8),
                 n3 = *reinterpret_cast<const float4*>(lp + 12);
    const float e[13] = {c.x, c.y, c.z, c.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, n3.x};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (u0 + k < KW) {            // uniform
        const float wk = w[u0 + k];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(wk, e[3 * k + i], acc[i]);
      }
    }
    c = n3; lp += 12;
  }
}

// out[ro + f .. f + 3] = a, or the USM epilogue src0 + (src0 - a) * amount (lib/utils.py:275)
__device__ __forceinline__ void store4(float* __restrict__ out, const float* __restrict__ src0, int usm, float amount, long ro, int f, int L, const float a[4]) {
  if (f + 3 < L) {
    f4u o = {a[0], a[1], a[2], a[3]};
    if (usm) {
      const f4u s = *reinterpret_cast<const f4u*>(src0 + ro + f);
      o.x = fmaf(s.x - a[0], amount, s.x); o.y = fmaf(s.y - a[1], amount, s.y);
      o.z = fmaf(s.z - a[2], amount, s.z); o.w = fmaf(s.w - a[3], amount, s.w);
    }
    *reinterpret_cast<f4u*>(out + ro + f) = o;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (f + i < L) {
        const float s = usm ? src0[ro + f + i] : 0.f;
        out[ro + f + i] = usm ? fmaf(s - a[i], amount, s) : a[i];
      }
  }
}

// ---- scipy.signal.convolve2d(channel, kern, mode="same", boundary="symm") on the three channels: KH x KW taps --------------
// `wr` is the kernel reversed on both axes (wr[v][u] = kern[KH-1-v][KW-1-u]), so that out[y][f] = sum_v sum_u wr[v][u] *
// ext[y + cy - (KH-1) + v][f + 3 (cx - (KW-1) + u)], cy = (KH-1)/2, cx = (KW-1)/2; v slow, u fast, both ascending.
// KH = 1 is the row pass of a rank-1 kernel; KH > 1 the fallback for kernels that are not outer products.
__global__ __launch_bounds__(256) void k_img_conv_rows(const float* __restrict__ src, int H, int W, const float* __restrict__ wr, int KH, int KW,
                                                      float* __restrict__ out, const float* __restrict__ src0, int usm, float amount) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int L = 3 * W, S = FT + 12 * ((KW + 3) / 4) + 4;      // floats per LDS row: what the last lane's last group of 4 taps reads
  const int f0 = blockIdx.x * FT, y0 = blockIdx.y * RT;
  const int cy = (KH - 1) / 2, cx = (KW - 1) / 2;
  stage_tile<false>(tile, S, src, H, W, y0 + cy - (KH - 1), f0 + 3 * (cx - (KW - 1)), RT + KH - 1, S / 4);
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int m = 0; m < RT / 4; ++m) {
    const int r = wv + 4 * m, y = y0 + r;
    if (y >= H) break;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < KH; ++v) row_taps(tile + (r + v) * S + 4 * lane, wr + v * KW, KW, acc);
    store4(out, src0, usm, amount, (long)y * L, f0 + 4 * lane, L, acc);
  }
}

// ---- column pass of a rank-1 kernel: out[y][f] = sum_v wr[v] * ext[y + cy - (KH-1) + v][f], v ascending; optional USM ----
__global__ __launch_bounds__(256) void k_img_conv_cols(const float* __restrict__ src, int H, int W, const float* __restrict__ wr, int KH,
                                                      float* __restrict__ out, const float* __restrict__ src0, int usm, float amount) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int L = 3 * W;
  const int f0 = blockIdx.x * FT, y0 = blockIdx.y * VT;
  const int cy = (KH - 1) / 2;
  stage_tile<false>(tile, FT, src, H, W, y0 + cy - (KH - 1), f0, VT + KH - 1, FT / 4);
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int m = 0; m < VT / 4; ++m) {
    const int r = wv + 4 * m, y = y0 + r;
    if (y >= H) break;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* lp = tile + r * FT + 4 * lane;
    for (int v = 0; v < KH; ++v) {
      const float4 x = *reinterpret_cast<const float4*>(lp + v * FT);
      const float wk = wr[v];
      acc[0] = fmaf(wk, x.x, acc[0]); acc[1] = fmaf(wk, x.y, acc[1]); acc[2] = fmaf(wk, x.z, acc[2]); acc[3] = fmaf(wk, x.w, acc[3]);
    }
    store4(out, src0, usm, amount, (long)y * L, f0 + 4 * lane, L, acc);
  }
}

// ---- bilateral filter (lib/utils.py:173-234) on the three channels ------------------------------------------------------------
// Symmetric padding by `radius`; w = expf((nb - centre)^2 * ki) * ws[j][i], ki = -1 / (2 std_i^2), ws = the spatial weights
// exp(-(i^2 + j^2) / 2 std_s^2) precomputed once per call; sums in the reference's offset order (x offset j slow, y offset i
// fast), one division at the end.  A weighted mean lies between the smallest and the largest value it averages; rounding of the
// two float32 sums can miss that by an ulp, so the quotient is clamped to the window's range (a constant frame is a fixed point).
__global__ __launch_bounds__(256) void k_img_bilateral(const float* __restrict__ src, int H, int W, int R, float ki, const float* __restrict__ ws,
                                                      float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int L = 3 * W, D = 2 * R + 1;
  const int nq = (FT + 6 * R + 3) / 4, SW = swz(4 * nq) + 1;
  const int f0 = blockIdx.x * FT, y0 = blockIdx.y * RT;
  stage_tile<true>(tile, SW, src, H, W, y0 - R, f0 - 3 * R, RT + 2 * R, nq);
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int m = 0; m < RT / 4; ++m) {
    const int r = wv + 4 * m, y = y0 + r;
    if (y >= H) break;
    float cen[4], lo[4], hi[4], acc[4] = {0.f, 0.f, 0.f, 0.f}, wsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) lo[i] = hi[i] = cen[i] = tile[(r + R) * SW + swz(4 * lane + 3 * R + i)];
    for (int j = 0; j < D; ++j) {
      int p[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = swz(4 * lane + 3 * j + i);
      const float* row = tile + r * SW;
      for (int i2 = 0; i2 < D; ++i2, row += SW) {
        const float wsp = ws[j * D + i2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float nb = row[p[i]], d = nb - cen[i];
          const float w = expf(d * d * ki) * wsp;
          acc[i] = fmaf(nb, w, acc[i]); wsum[i] += w;
          lo[i] = fminf(lo[i], nb); hi[i] = fmaxf(hi[i], nb);
        }
      }
    }
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fminf(fmaxf(__fdiv_rn(acc[i], wsum[i]), lo[i]), hi[i]);
    store4(out, nullptr, 0, 0.f, (long)y * L, f0 + 4 * lane, L, o);
  }
}

}  // namespace

size_t ics_img_conv_rows_lds(int KH, int KW) { return (size_t)(RT + KH - 1) * (FT + 12 * ((KW + 3) / 4) + 4) * sizeof(float); }
size_t ics_img_conv_cols_lds(int KH) { return (size_t)(VT + KH - 1) * FT * sizeof(float); }
size_t ics_img_bilateral_lds(int radius) {
  const int nq = (FT + 6 * radius + 3) / 4;
  return (size_t)(RT + 2 * radius) * (4 * nq + (4 * nq >> 5) + 1) * sizeof(float);
}

hipError_t ics_launch_img_conv_rows(const float* src, int H, int W, const float* wr, int KH, int KW, float* out, const float* src0, int usm,
                                    float amount, hipStream_t s) {
  const size_t lds = ics_img_conv_rows_lds(KH, KW);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = set_dynamic_lds(k_img_conv_rows, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_conv_rows, dim3((3 * W + FT - 1) / FT, (H + RT - 1) / RT), dim3(256), lds, s, src, H, W, wr, KH, KW, out, src0, usm, amount);
  return hipGetLastError();
}

hipError_t ics_launch_img_conv_cols(const float* src, int H, int W, const float* wr, int KH, float* out, const float* src0, int usm, float amount,
                                    hipStream_t s) {
  const size_t lds = ics_img_conv_cols_lds(KH);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = set_dynamic_lds(k_img_conv_cols, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_conv_cols, dim3((3 * W + FT - 1) / FT, (H + VT - 1) / VT), dim3(256), lds, s, src, H, W, wr, KH, out, src0, usm, amount);
  return hipGetLastError();
}

hipError_t ics_launch_img_bilateral(const float* src, int H, int W, int radius, float ki, const float* ws, float* out, hipStream_t s) {
  const size_t lds = ics_img_bilateral_lds(radius);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = set_dynamic_lds(k_img_bilateral, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_bilateral, dim3((3 * W + FT - 1) / FT, (H + RT - 1) / RT), dim3(256), lds, s, src, H, W, radius, ki, ws, out);
  return hipGetLastError();
}
