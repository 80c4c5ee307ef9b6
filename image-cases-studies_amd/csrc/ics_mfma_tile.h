// ics_mfma_tile.h -- what the fp16-split matrix-core units share (ics_conv_mfma.hip, ics_synth_gradk_mfma.hip, ics_gradk_mfma.hip):
// vector types, buffer addressing, the power-of-two tile scale and the (hi, lo) split, the staging of a tile's fp32 HWC rows, and the
// weight-row constants of the Toeplitz convolution.  Each unit pulls it in with `using namespace icsmm;` inside its anonymous
// namespace; the kernels stay in their units (their names are what tests/test_isa.py, scripts/isa_table.sh and the profiles know).
#pragma once
#include "ics_common.h"

namespace icsmm {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u3 __attribute__((ext_vector_type(3)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// power-of-two scale that brings a maximum magnitude m into [2^14, 2^15) (fp16 overflows at 65504);
// 1 for m = 0 / Inf / NaN.  `inv` is the exact inverse.
__device__ __forceinline__ void pow2_scale(float m, float& s, float& inv) {
  const uint32_t e = (__float_as_uint(m) >> 23) & 0xFFu;
  uint32_t sb = 127u;
  if (m > 0.f && e != 255u) { sb = 268u - e; sb = sb > 240u ? 240u : sb; }
  s = __uint_as_float(sb << 23);
  inv = __uint_as_float((254u - sb) << 23);
}

// the two fp16 terms of a scaled fp32 operand: x = hi + lo to 22 significand bits.  As scalars, or as element p of two vectors / arrays.
// (in the convolution's conversion as one v_fma_mix from the raw value: 36 vector instructions fewer per tile, same time)
__device__ __forceinline__ void split_f16(float x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}
template <typename V>
__device__ __forceinline__ void split_f16(float x, V& hi, V& lo, int p) {
  const _Float16 xh = (_Float16)x;
  hi[p] = xh;
  lo[p] = (_Float16)(x - (float)xh);
}

// Buffer addressing (SGPR resource + 32-bit lane offset + SGPR/immediate offset): with flat 64-bit pointers
// the compiler materialised one 64-bit VGPR base per load and spilled them.
constexpr int BUF_WORD3 = 0x00020000;   // gfx9 raw buffer: DATA_FORMAT = 32
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7FFFFFFF, BUF_WORD3);
}

// workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also waits for every outstanding global load
// (vmcnt(0)): with the image operand or the next tile's rows in flight it stalled the whole workgroup for an HBM round trip.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// a copy of `x` the optimiser cannot trace back: values derived from it are recomputed where they are used
// instead of being hoisted out of the tile loop (where they were spilled -- and a scratch reload waits on
// vmcnt, i.e. on the whole prefetch in flight)
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }

// the matrix instructions and the funnel shift, short
__device__ __forceinline__ f4 f_mfma32(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f4 f_mfma16(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ uint32_t f_align(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }

// the staged rows of a tile: task t = (row, 4-pixel group) -> three dwordx4 loads (4-byte aligned).
// `soff` = wave-uniform byte offset of the tile's first staged element.  C: NIT, NT, NTASK, XG.
template <typename C>
__device__ __forceinline__ void load_raw(f32x4u (&v)[C::NIT][3], __amdgpu_buffer_rsrc_t rs, int soff, int tid, int pitch) {
#pragma unroll
  for (int k = 0; k < C::NIT; ++k) {
    int t = tid + k * C::NT;
    t = t < C::NTASK ? t : C::NTASK - 1;  // clamp instead of predicating the load
    const int row = t / C::XG, xg = t - row * C::XG;
    const int toff = 4 * (row * pitch + 12 * xg);
#pragma unroll
    for (int h = 0; h < 3; ++h) v[k][h] = __builtin_bit_cast(f32x4u, __builtin_amdgcn_raw_buffer_load_b128(rs, toff + 16 * h, soff, 0));
  }
}

// one channel of the staged rows -> (hi, lo) fp16 planes; C::row_ptr(plane, row) = where a staged row sits inside a plane (its row class)
template <typename C, int CH>
__device__ __forceinline__ void convert_channel(const f32x4u (&raw)[C::NIT][3], float s_x, unsigned char* plane, int tid) {
#pragma unroll
  for (int k = 0; k < C::NIT; ++k) {
    const int t = tid + k * C::NT;
    if (t < C::NTASK) {
      const int row = t / C::XG, xg = t - row * C::XG;
      unsigned char* dst = C::row_ptr(plane, row) + 8 * xg;
      h4 hi, lo;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int idx = 3 * p + CH;
        split_f16(raw[k][idx >> 2][idx & 3] * s_x, hi, lo, p);
      }
      *reinterpret_cast<h4*>(dst) = hi;
      *reinterpret_cast<h4*>(dst + C::PLANE) = lo;
    }
  }
}

// Weight rows of the Toeplitz convolution in LDS = the global table built by k_psf (ics_common.h), copied verbatim: [c][a] rows of
// 2 * WROWB bytes (the hi and lo split terms interleaved dword by dword), one float 1/s_w behind the last row.  A row holds halves
// 8 .. K+24 of the zero-padded kernel row Wp[idx] = W[idx - 15] (the taps sit at local halves 7 .. K+6, at least ten zeros follow):
// every 8-half window that meets a tap lies inside, and the all-zero windows are redirected to the zero tail.
constexpr int weight_row_bytes(int K) { return (2 * (K + 17) + 3) & ~3; }
constexpr int weight_lds_bytes(int K) { return 3 * K * 2 * weight_row_bytes(K); }
template <int K>
struct MmaWeights {
  static constexpr int WROWB = weight_row_bytes(K);
  static constexpr int WZERO = (K + 7) / 2;      // first all-zero dword of a row
  static constexpr int WLDS = weight_lds_bytes(K);
};

}  // namespace icsmm
