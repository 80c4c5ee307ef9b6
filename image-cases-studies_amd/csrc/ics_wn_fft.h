// ics_wn_fft.h -- for ics_img_wiener.hip, ics_img_tvdeconv.hip, ics_img_tvmdeconv.hip, ics_img_psfest.hip and ics_img_edges.hip (the rows of the masked pair solve) only (everything here is local to the unit that includes it): what
// the operators on the frame-sized fp32 2-D transform share.  Device side: the line transform, a Stockham autosort transform of one line
// of N = 2^n points in LDS, and the layout of its twiddle table (ics_img_wiener.hip describes both); a line into LDS and out of it; the
// K values of a PSF at their rolled places in a line; a pixel of the frame extended to the transform size.  Host side: the lanes of a
// line's workgroup, the shape check and the dynamic-LDS limit of the line kernels.  The kernels stay in their units.
#pragma once
#include "ics_kernels.h"

namespace {

#define WN_MAX ICS_IMG_WIENER_MAX              // longest line: two buffers of it are 128 KB of the 160 KB of LDS
#define WN_LANES 1024                          // lanes of a line's workgroup at most (N / 4 below 4096 points, 64 at least)

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

// the line l of n points -> sm, a barrier passed (a real line: its values as the real parts)
__device__ __forceinline__ void wn_load(float2* sm, const float2* l, int n) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int j = tid; j < n; j += nthr) sm[j] = l[j];
  __syncthreads();
}
__device__ __forceinline__ void wn_load(float2* sm, const float* l, int n) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int j = tid; j < n; j += nthr) sm[j] = make_float2(l[j], 0.f);
  __syncthreads();
}
// the first n points of the line r in LDS -> l
__device__ __forceinline__ void wn_store(float2* l, const float2* r, int n) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int j = tid; j < n; j += nthr) l[j] = r[j];
}

// a line of P points of a PSF, its K values v(0) .. v(K - 1) zero padded, tap K / 2 rolled to point 0 -> its transform (sm or sm + P)
template <typename V>
__device__ __forceinline__ const float2* wn_psf_line(float2* sm, int P, int logP, int K, const float2* __restrict__ tw, V v) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int j = tid; j < P; j += nthr) {
    int t = j + K / 2;
    if (t >= P) t -= P;
    sm[j] = t < K ? v(t) : make_float2(0.f, 0.f);
  }
  __syncthreads();
  return wn_fft<false>(sm, sm + P, P, logP, tw);
}

// pixel (y, x) of channel c of the H x W frame f (HWC) extended to Py x Px so that the wrap-around carries no step: along y, for every
// column, rows H .. Py - 1 are (1 - t / g) f[H - 1] + (t / g) f[0], g = Py - H + 1, t = 1 .. g - 1; then the same along x on all Py rows.
// ZERO_NONFINITE: a non-finite value of f counts as 0
template <bool ZERO_NONFINITE>
__device__ __forceinline__ float wn_ext(const float* __restrict__ f, int c, int y, int x, int H, int W, int Py, int Px) {
  const bool below = y >= H;
  const float* r0 = f + (long)(below ? H - 1 : y) * (3L * W) + c;   // the row itself, or the last one
  const float* r1 = f + c;                                          // the first one
  const float ty = below ? (float)(y - H + 1) / (float)(Py - H + 1) : 0.f;
  const auto at = [&](const float* r, int i) { const float v = r[3L * i]; return ZERO_NONFINITE && !isfinite(v) ? 0.f : v; };
  const auto px = [&](int i) { return below ? (1.f - ty) * at(r0, i) + ty * at(r1, i) : at(r0, i); };
  const float last = px(W - 1), first = px(0);                      // (read on every path: uniform over a row's workgroup, scalar loads in the gfx950 code)
  if (x < W) return px(x);
  const float t = (float)(x - W + 1) / (float)(Px - W + 1);
  return (1.f - t) * last + t * first;
}

inline int wn_log2(int v) { int k = 0; while ((1 << k) < v) ++k; return k; }
inline int wn_lanes(int P) { const int t = P / 4; return t < 64 ? 64 : (t > WN_LANES ? WN_LANES : t); }

// an H x W frame, a K x K PSF and transform sizes that hold them (ics_img_wiener_sizes)
inline bool wn_shape_ok(int H, int W, int K, int Py, int Px) {
  return H >= 1 && W >= 1 && K >= 3 && (K & 1) && K <= H && K <= W && Py >= H + K - 1 && Px >= W + K - 1 && Py <= WN_MAX && Px <= WN_MAX && !(Py & (Py - 1)) &&
         !(Px & (Px - 1));
}

// before the launches of the line kernels Kern...: lines of 8192 points take 128 KB of dynamic LDS, more than a kernel gets unasked.
// Raises the limit of each to the longest line, once per kernel and device
template <auto Kern>
hipError_t wn_raise_lds_of(int dev) {
  static std::atomic<bool> done[ICS_MAX_DEVICES];
  return ics_configure_lds(done, dev, Kern, ics_img_wiener_lds(WN_MAX));
}
template <auto... Kern>
hipError_t wn_raise_lds(int Py, int Px) {
  if (ics_img_wiener_lds(Py > Px ? Py : Px) <= 64 * 1024) return hipSuccess;
  const int dev = ics_current_device();
  hipError_t e = hipSuccess;
  ((e = e == hipSuccess ? wn_raise_lds_of<Kern>(dev) : e), ...);
  return e;
}

}  // namespace
