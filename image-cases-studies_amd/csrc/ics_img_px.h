// ics_img_px.h -- for ics_img_filters.hip, ics_img_tvdenoise.hip, ics_img_wavelet.hip, ics_img_guided.hip, ics_img_llf.hip, ics_img_noise.hip, ics_img_despeckle.hip, ics_img_blurwidth.hip, ics_img_blurmap.hip, ics_img_mask.hip, ics_img_align.hip, ics_img_edges.hip and ics_img_tvmdeconv.hip (the pixel load) only (everything here is local to
// the unit that includes it): what their kernels and launchers share, the 12-byte pixel access, the luma, the symmetric fold, the B3-spline pass, two launch helpers.
#pragma once
#include "ics_kernels.h"

namespace {

struct __attribute__((packed, aligned(4))) f3u { float x, y, z; };   // one pixel: 12-byte access at 4-byte alignment

__device__ __forceinline__ void ld3(const float* __restrict__ p, float v[3]) {
  const f3u t = *reinterpret_cast<const f3u*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z;
}
__device__ __forceinline__ void st3(float* __restrict__ p, const float v[3]) {
  const f3u t = {v[0], v[1], v[2]};
  *reinterpret_cast<f3u*>(p) = t;
}

// the luma of one pixel (ics_img_blurwidth.hip, ics_img_blurmap.hip, ics_img_mask.hip, ics_img_align.hip, ics_img_edges.hip): (R + G + B) * float32(1 / 3), every operation rounded once
__device__ __forceinline__ float px_luma(const float v[3]) { return __fmul_rn(__fadd_rn(__fadd_rn(v[0], v[1]), v[2]), 0.333333343267440796f); }

// index of the symmetric extension ... x1 x0 | x0 x1 ... x(n-1) | x(n-1) x(n-2) ... (numpy.pad(mode="symmetric")), at any distance
__device__ __forceinline__ int symm(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}
// ... with the division skipped inside the picture (ics_img_wavelet.hip): either form alone changes the code of the other unit's kernels
__device__ __forceinline__ int wv_fold(int i, int n) { return (unsigned)i < (unsigned)n ? i : symm(i, n); }

// one axis pass of the B3 spline (ics_img_wavelet.hip, ics_img_noise.hip): am2 .. ap2 at offsets -2 d .. 2 d
__device__ __forceinline__ float wv_pass(float am2, float am1, float a0, float ap1, float ap2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(__fadd_rn(am2, ap2), 0.0625f), __fmul_rn(__fadd_rn(am1, ap1), 0.25f)), __fmul_rn(a0, 0.375f));
}

// a launch with more dynamic LDS than the default limit of 64 KB needs the kernel's limit raised first
template <typename Kern>
hipError_t set_dynamic_lds(Kern kern, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

// hipLaunchKernelGGL of a `template <bool VEC>` kernel, VEC taken from the run-time `coupling`
#define ICS_LAUNCH_VEC(coupling, kern, ...) \
  do { if (coupling) hipLaunchKernelGGL(kern<true>, __VA_ARGS__); else hipLaunchKernelGGL(kern<false>, __VA_ARGS__); } while (0)
