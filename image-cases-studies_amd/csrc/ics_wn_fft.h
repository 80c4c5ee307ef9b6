// ics_wn_fft.h -- for ics_img_wiener.hip, ics_img_tvdeconv.hip, ics_img_tvmdeconv.hip and ics_img_psfest.hip only (everything here is local to the unit that includes it): the
// line transform of the frame-sized fp32 transforms, a Stockham autosort transform of one line of N = 2^n points in LDS, and the
// layout of its twiddle table (ics_img_wiener.hip describes both).  Device functions only; the kernels stay in their units.
#pragma once
#include "ics_kernels.h"

namespace {

__device__ __forceinline__ float2 wn_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 wn_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 wn_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// the line in x (written by the whole workgroup, a barrier passed since) -> its transform, unscaled, in the returned buffer (x or y), a
// barrier passed.  tw: the table of this N (wn_table)
template <bool INV>
__device__ __forceinline__ float2* wn_fft(float2* x, float2* y, int N, int logN, const float2* __restrict__ tw) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  int p = 1;
  if (logN & 1) {
    const int t = N >> 1;
    for (int b = tid; b < t; b += nthr) {
      const float2 u0 = x[b], u1 = x[b + t];
      y[2 * b] = wn_add(u0, u1);
      y[2 * b + 1] = wn_sub(u0, u1);
    }
    __syncthreads();
    float2* tmp = x; x = y; y = tmp;
    p = 2;
  }
  const int t = N >> 2, p0 = p;
  for (; p < N; p <<= 2) {
    const float2* __restrict__ ws = tw + (p - p0);
    for (int b0 = tid; b0 < t; b0 += 2 * nthr) {
      float2 u[2][4], w[2][3];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int b = b0 + h * nthr;
        if (b < t) {
          const int k = b & (p - 1);
#pragma unroll
          for (int q = 0; q < 4; ++q) u[h][q] = x[b + q * t];
#pragma unroll
          for (int q = 0; q < 3; ++q) w[h][q] = ws[3 * k + q];
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int b = b0 + h * nthr;
        if (b < t) {
          const int k = b & (p - 1), j = ((b - k) << 2) + k;
          if (INV) { w[h][0].y = -w[h][0].y; w[h][1].y = -w[h][1].y; w[h][2].y = -w[h][2].y; }
          const float2 u0 = u[h][0], u1 = wn_mul(u[h][1], w[h][0]), u2 = wn_mul(u[h][2], w[h][1]), u3 = wn_mul(u[h][3], w[h][2]);
          const float2 v0 = wn_add(u0, u2), v1 = wn_sub(u0, u2), v2 = wn_add(u1, u3), d = wn_sub(u1, u3);
          const float2 v3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);   // -+ i d
          y[j] = wn_add(v0, v2);
          y[j + p] = wn_add(v1, v3);
          y[j + 2 * p] = wn_sub(v0, v2);
          y[j + 3 * p] = wn_sub(v1, v3);
        }
      }
    }
    __syncthreads();
    float2* tmp = x; x = y; y = tmp;
  }
  return x;
}

// entry i of the table of an N-point line (N - p0 entries): stage p = p0, 4 p0, ... holds {w, w^2, w^3}(k), k < p, from offset p - p0
__device__ __forceinline__ float2 wn_table(int i, int logN) {
  int p = (logN & 1) ? 2 : 1, off = 0;
  while (i >= off + 3 * p) { off += 3 * p; p <<= 2; }
  const int r = i - off, k = r / 3, m = r - 3 * k + 1;
  const double a = (double)(k * m) / (double)(2 * p);            // exp(-2 pi i k m / 4p)
  return make_float2((float)cospi(a), (float)-sinpi(a));
}

}  // namespace
