// ics_fft_math.h -- complex arithmetic and the 4 / 8 / 16-point transforms of the transform tiles (ics_fft_tile.h), device and host pass.
#pragma once
#include "ics_tw128.h"

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

#define ICS_FFT_HD __host__ __device__ __forceinline__

namespace icsfft {

// exp(-2 pi i t / 128): device copy (scalar / vector loads through the caches) and host copy (CPU emulation in tools/bench_conv_fft.hip)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ const float d_tw128[128][2] = {ICS_TW128_VALUES};
#else
static const float h_tw128[128][2] = {ICS_TW128_VALUES};
#endif

ICS_FFT_HD v2f tw128(int t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (v2f){d_tw128[t & 127][0], d_tw128[t & 127][1]};
#else
  return (v2f){h_tw128[t & 127][0], h_tw128[t & 127][1]};
#endif
}

// a * b and a * conj(b): one packed multiply + one packed fma.  On the device the operand swaps and sign flips ride on the VOP3P modifiers
// (op_sel / neg): as vector shuffles the compiler spent a v_mov + v_xor on every product with a register operand.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ v2f cmul(v2f a, v2f b) {
  v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));                                   // (a.x b.x, a.x b.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(t));      // + (-a.y b.y, a.y b.x)
  return r;
}
__device__ __forceinline__ v2f cmulc(v2f a, v2f b) {
  v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));                       // (a.x b.x, -a.x b.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));                    // + (a.y b.y, a.y b.x)
  return r;
}
// the same with the second factor in a scalar register pair (wave-uniform twiddles of stages A and G: one scalar operand per instruction)
__device__ __forceinline__ v2f cmul_s(v2f a, v2f b) {
  v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "s"(b));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "s"(b), "v"(t));
  return r;
}
__device__ __forceinline__ v2f cmulc_s(v2f a, v2f b) {
  v2f t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(a), "s"(b));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(b), "v"(t));
  return r;
}
// a + b * (-i) = a + (b.y, -b.x)   and   a + b * (+i) = a + (-b.y, b.x): one instruction each
__device__ __forceinline__ v2f add_mi(v2f a, v2f b) { v2f r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ v2f add_pi(v2f a, v2f b) { v2f r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
#else
ICS_FFT_HD v2f cmul(v2f a, v2f b) { return __builtin_elementwise_fma((v2f){a.y, a.y}, (v2f){-b.y, b.x}, (v2f){a.x, a.x} * b); }
ICS_FFT_HD v2f cmulc(v2f a, v2f b) { return __builtin_elementwise_fma((v2f){a.y, a.y}, (v2f){b.y, b.x}, (v2f){a.x, a.x} * (v2f){b.x, -b.y}); }
ICS_FFT_HD v2f cmul_s(v2f a, v2f b) { return cmul(a, b); }
ICS_FFT_HD v2f cmulc_s(v2f a, v2f b) { return cmulc(a, b); }
ICS_FFT_HD v2f add_mi(v2f a, v2f b) { return (v2f){a.x + b.y, a.y - b.x}; }
ICS_FFT_HD v2f add_pi(v2f a, v2f b) { return (v2f){a.x - b.y, a.y + b.x}; }
#endif
// products with COMPILE-TIME constants stay in C++: the compiler folds the swapped / negated constant and reads it from scalar registers
ICS_FFT_HD v2f cmulk(v2f a, v2f b) { return __builtin_elementwise_fma((v2f){a.y, a.y}, (v2f){-b.y, b.x}, (v2f){a.x, a.x} * b); }
ICS_FFT_HD v2f cmulck(v2f a, v2f b) { return __builtin_elementwise_fma((v2f){a.y, a.y}, (v2f){b.y, b.x}, (v2f){a.x, a.x} * (v2f){b.x, -b.y}); }
// forward twiddles are exp(-i phi): DIR = +1 multiplies by b, DIR = -1 by conj(b)
template <int DIR> ICS_FFT_HD v2f cmuld(v2f a, v2f b) { return DIR > 0 ? cmulk(a, b) : cmulck(a, b); }
// a + b * (-i)^DIR and a - b * (-i)^DIR
template <int DIR> ICS_FFT_HD v2f add_rot(v2f a, v2f b) { return DIR > 0 ? add_mi(a, b) : add_pi(a, b); }
template <int DIR> ICS_FFT_HD v2f sub_rot(v2f a, v2f b) { return DIR > 0 ? add_pi(a, b) : add_mi(a, b); }

template <int DIR> ICS_FFT_HD void fft4(v2f& a0, v2f& a1, v2f& a2, v2f& a3) {
  const v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, d = a1 - a3;
  a0 = t0 + t2; a2 = t0 - t2; a1 = add_rot<DIR>(t1, d); a3 = sub_rot<DIR>(t1, d);
}
// the same with input 2 still to be multiplied by (-i)^DIR (w16^4 of the 16-point transform)
template <int DIR> ICS_FFT_HD void fft4_r2(v2f& a0, v2f& a1, v2f& a2, v2f& a3) {
  const v2f t0 = add_rot<DIR>(a0, a2), t1 = sub_rot<DIR>(a0, a2), t2 = a1 + a3, d = a1 - a3;
  a0 = t0 + t2; a2 = t0 - t2; a1 = add_rot<DIR>(t1, d); a3 = sub_rot<DIR>(t1, d);
}

// 8 points, natural order in, natural order out.  n = 2 n1 + n2, k = k1 + 4 k2.
template <int DIR> ICS_FFT_HD void fft8(v2f (&v)[8]) {
  constexpr float R = 0.70710678118654752440f;
  v2f e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  fft4<DIR>(e0, e1, e2, e3);
  fft4<DIR>(o0, o1, o2, o3);
  // o[k1] *= w8^(k1):  w8 = (1 - i)/sqrt2 forward, (1 + i)/sqrt2 inverse;  w8^2 = -+i rides on the last butterfly;  w8^3 = -(1 + i)/sqrt2 / -(1 - i)/sqrt2
  o1 = add_rot<DIR>(o1, o1) * R;
  o3 = sub_rot<DIR>(o3, o3) * -R;
  v[0] = e0 + o0; v[4] = e0 - o0;
  v[1] = e1 + o1; v[5] = e1 - o1;
  v[2] = add_rot<DIR>(e2, o2); v[6] = sub_rot<DIR>(e2, o2);
  v[3] = e3 + o3; v[7] = e3 - o3;
}

// 16 points, natural order in, natural order out.  n = 4 n1 + n2, k = k1 + 4 k2.
template <int DIR> ICS_FFT_HD void fft16(v2f (&v)[16]) {
  constexpr float C1 = 0.92387953251128675613f, S1 = 0.38268343236508977173f, R = 0.70710678118654752440f;
  v2f a[4][4];   // a[n2][k1]
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) {
    a[n2][0] = v[n2]; a[n2][1] = v[4 + n2]; a[n2][2] = v[8 + n2]; a[n2][3] = v[12 + n2];
    fft4<DIR>(a[n2][0], a[n2][1], a[n2][2], a[n2][3]);
  }
  // a[n2][k1] *= w16^(n2 k1), w16^t = (cos(pi t / 8), -sin(pi t / 8)) forward  (w16^4 = -+i: inside fft4_r2)
  a[1][1] = cmuld<DIR>(a[1][1], (v2f){C1, -S1});
  a[1][2] = cmuld<DIR>(a[1][2], (v2f){R, -R});
  a[1][3] = cmuld<DIR>(a[1][3], (v2f){S1, -C1});
  a[2][1] = cmuld<DIR>(a[2][1], (v2f){R, -R});
  a[2][3] = cmuld<DIR>(a[2][3], (v2f){-R, -R});
  a[3][1] = cmuld<DIR>(a[3][1], (v2f){S1, -C1});
  a[3][2] = cmuld<DIR>(a[3][2], (v2f){-R, -R});
  a[3][3] = cmuld<DIR>(a[3][3], (v2f){-C1, S1});
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) {
    if (k1 == 2) fft4_r2<DIR>(a[0][k1], a[1][k1], a[2][k1], a[3][k1]);
    else fft4<DIR>(a[0][k1], a[1][k1], a[2][k1], a[3][k1]);   // -> k2 = 0..3
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) v[k1 + 4 * k2] = a[k2][k1];
  }
}

}  // namespace icsfft
