// ics_update.h -- the image update of the RL/MM loop, stated once: the arithmetic every update kernel applies per value.
//
// A5 + A6 + A8 + A10 (lib/deconvolution.pyx:499-552), one pass over the u-frame.
//   DoF   = ((gradu - image)/(gradu + image))^2 [ / lambd when non-blind ]      (:499-502, interior)   ics_dof_ratio, ics_dof_mask
//   g     = lambd*gradu + (u - ut)/2.                                           (:519, else-branch)    ics_mm_g
//   g     = float((T + lambd*gradu) + (u - ut)/4.)  in double                   (:517, active MM-TV)   ics_mm_g_tv
//   dt_k  = step*(max u_k + 0)/(max|g_k| + 1e-15)                               (:524, 1/(M*N) == 0)   ics_step_dt
//   u    -= dt_k * g                                                            (:531)                 ics_step_u
//   u     = (1 - DoF)*u + DoF*image   on the interior                           (:552)                 ics_dof_blend
// A9 (:534-549) subtracts exactly zero from `image` and is therefore omitted; the active MM-TV form steps the image
// between ics_dof_mask and ics_dof_blend (pyx:548-549), which is why the two are separate.
// Every operation is rounded separately like the reference's C / numpy float32 code: __f*_rn in the device pass, plain operators in the
// host pass (every unit is built with -ffp-contract=off).  The kernels keep their loads and stores, their `inside` / `own` predicates,
// their channel selection and their loop shape; what they compute per value is here and nowhere else, and tools/check_update_px.hip runs
// exactly these functions on the CPU against the numpy restatement (tests/test_update_host.py).
#pragma once
#include "ics_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define ICS_FADD(a, b) __fadd_rn(a, b)
#define ICS_FSUB(a, b) __fsub_rn(a, b)
#define ICS_FMUL(a, b) __fmul_rn(a, b)
#define ICS_FDIV(a, b) __fdiv_rn(a, b)
#else   /* host pass: tools/check_update_px.hip and the CPU emulation of tools/bench_conv_fft.hip */
#define ICS_FADD(a, b) ((a) + (b))
#define ICS_FSUB(a, b) ((a) - (b))
#define ICS_FMUL(a, b) ((a) * (b))
#define ICS_FDIV(a, b) ((a) / (b))
#endif
#define ICS_UPD_HD __host__ __device__ __forceinline__

// pyx:524; the PSF step (pyx:574) is the same rule with step / K for `step`, max psf for `maxu` and max |gradk| for `maxg`.
// (The macro form is for the two sites whose operands are key loads -- the image step of the active MM-TV form, pyx:548: a function
//  evaluates both loads before the product, and k_update_rows<1> came out scheduled differently.)
#define ICS_STEP_DT(step, maxu, maxg) ICS_FDIV(ICS_FMUL(step, maxu), ICS_FADD(maxg, 1e-15f))
ICS_UPD_HD float ics_step_dt(float step, float maxu, float maxg) { return ICS_STEP_DT(step, maxu, maxg); }
ICS_UPD_HD float ics_mm_g(float lambd, float gradu, float u, float ut) { return ICS_FADD(ICS_FMUL(lambd, gradu), ICS_FMUL(ICS_FSUB(u, ut), 0.5f)); }
ICS_UPD_HD float ics_mm_g_tv(float T, float lambd, float gradu, float u, float ut) {
  return (float)(((double)T + (double)ICS_FMUL(lambd, gradu)) + (double)ICS_FSUB(u, ut) / 4.0);
}
ICS_UPD_HD float ics_step_u(float u, float dt, float g) { return ICS_FSUB(u, ICS_FMUL(dt, g)); }

// The ratio of the DoF mask, (g - f)/(g + f)  (lib/deconvolution.pyx:499; g = raw back-projection, f = image), IEEE in every
// case but one: g == f == 0 EXACTLY gives 1, not 0/0 = NaN.  Where image and u are exactly black the reference's g is the rounding
// noise of its complex64 FFT (~1e-10, either sign) and (g - 0)/(g + 0) == 1 for every non-zero g, so the reference returns a
// finite picture on frames with black bands; this library's convolutions return exact zeros there, and a single NaN would spread
// over the whole frame through the next convolution and the NaN-propagating maxima.  g + f == 0 with g != 0 stays +-inf as in
// the reference.  Contract and measurements: include/ics_hip.h ("DoF ratio"), tests/test_gpu_black.py.
ICS_UPD_HD float ics_dof_ratio(float g, float f) {
  const float d = ICS_FDIV(ICS_FSUB(g, f), ICS_FADD(g, f));
  return (g == 0.f && f == 0.f) ? 1.0f : d;
}
ICS_UPD_HD float ics_dof_mask(float gradu, float f, float lambd, bool blind) {
  const float d = ics_dof_ratio(gradu, f);
  float D = ICS_FMUL(d, d);
  if (!blind) D = ICS_FDIV(D, lambd);
  return D;
}
ICS_UPD_HD float ics_dof_blend(float D, float un, float f) { return ICS_FADD(ICS_FMUL(ICS_FSUB(1.0f, D), un), ICS_FMUL(D, f)); }

// DoF extrema of an outer iteration (pyx:593) as keys (ics_f2key), a NaN flagged apart: what a thread has seen so far.  A plain
// aggregate with statement macros around it: a constructor or a member function takes the struct's address, the optimiser then meets
// the kernels' loops with the three words in memory, and every update kernel's machine code moves.  (Member order: the compiler
// promotes the members last to first, and in this order the kernels keep the registers they had with three separate variables.)
struct IcsDofKeys { uint32_t knan, kmax, kmin; };
#define ICS_DOF_NONE {0u, 0u, 0xFFFFFFFFu}   /* knan, kmax, kmin: nothing seen yet */
#define ICS_DOF_NOTE(keys, D) \
  do { \
    if ((D) != (D)) (keys).knan = 1u; \
    else { const uint32_t k_ = ics_f2key(D); (keys).kmin = (keys).kmin < k_ ? (keys).kmin : k_; (keys).kmax = (keys).kmax > k_ ? (keys).kmax : k_; } \
  } while (0)
// 256-thread workgroups: wave -> workgroup (LDS) -> one atomic per workgroup and value, skipped where the running extremum covers it
// (a statement macro as well: as a function it reached k_update_rows<2> with the operands of one `or` exchanged)
#define ICS_DOF_FLUSH_WORKGROUP4(keys, dofkeys) \
  do { \
    __shared__ uint32_t shd_[4][3]; \
    uint32_t kmin_ = ics_shfl_min_u32((keys).kmin), kmax_ = ics_shfl_max_u32((keys).kmax), knan_ = ics_shfl_max_u32((keys).knan); \
    if ((threadIdx.x & 63) == 0) { shd_[threadIdx.x >> 6][0] = kmin_; shd_[threadIdx.x >> 6][1] = kmax_; shd_[threadIdx.x >> 6][2] = knan_; } \
    __syncthreads(); \
    if (threadIdx.x == 0) { \
      _Pragma("unroll") for (int w_ = 1; w_ < 4; ++w_) { \
        kmin_ = kmin_ < shd_[w_][0] ? kmin_ : shd_[w_][0]; kmax_ = kmax_ > shd_[w_][1] ? kmax_ : shd_[w_][1]; knan_ |= shd_[w_][2]; \
      } \
      if (kmin_ < (dofkeys)[0]) atomicMin((dofkeys) + 0, kmin_); \
      if (kmax_ > (dofkeys)[1]) atomicMax((dofkeys) + 1, kmax_); \
      if (knan_) atomicOr((dofkeys) + 2, 1u); \
    } \
  } while (0)

// Workgroups per CU of the update launch: few long-lived workgroups stream best.  k_update_rows at 4096^2 (4 reads + 1 write, 1.0 GB),
// segments per loop iteration x workgroups per CU: 3x2 0.173 ms, 4x2 0.167, 4x3 0.164, 4x4 0.170, 6x2 0.164, 6x4 0.180; smaller frames
// want fewer still: 2048^2 0.0568 / 0.0526 / 0.0565 ms and 3072^2 0.119 / 0.099 / 0.102 ms with 1 / 2 / 3 per CU, 1024^2 0.0252 / 0.0265 / 0.0299
static inline int ics_update_wgs_per_cu(long px) { return px >= 12000000L ? 3 : (px >= 1500000L ? 2 : 1); }
