// ics_psf_step.h -- the PSF step of a blind inner iteration, stated once: the arithmetic per value of A14 ... A17.
//
// lib/deconvolution.pyx:574-589 on the K x K x 3 PSF and its gradient:
//   dtpsf = step/K * (max psf + 0) / (max|gradk| + 1e-15)          (:574, one value for the three channels)   ics_psf_dt
//   psf  -= dtpsf * gradk                                           (:577-581)                                 ics_psf_step_px
//   correlation: psf = dstack(mean_c psf x 3)                       (:584-585)                                 ics_psf_mean3
//   psf < 0 -> 0                                                    (:587 -> :58-61)                           ics_psf_clamp
//   s_c = the channel's sum, float32, taps in the order (i, j)      (:62-64)                                   ics_psf_channel_sum
//   psf[..., c] /= s_c                                              (:66-70)                                   ics_psf_norm
// Every operation is rounded separately, as in ics_update.h: __f*_rn in the device pass, plain operators in the host pass (every unit is
// built with -ffp-contract=off).  k_psf_spectra (ics_conv_fft.hip; every workgroup of the spectrum launch steps a private copy,
// transform tiles) calls these functions; it keeps its own loads, stores, barriers and reductions -- the maxima are taken on
// order-preserving keys, so their order does not matter -- and tools/check_psf_step.hip runs exactly these functions on the CPU against a
// restatement of its own (tests/test_psf_step_host.py).
// SECOND STATEMENT: k_psf (ics_kernels.hip; one workgroup, every other route, and the stage API) keeps its own text of the same rule.
// Calling these functions from it changed the machine code of k_psf<false> and k_psf<true> (scripts/isa_diff.sh: 108 and 85 lines), and
// that kernel serves every route's goldens.  A change of the rule is made in both places; tests/test_gpu_psf_step_tiles.py holds the two
// against each other bit for bit.
#pragma once
#include "ics_update.h"

ICS_UPD_HD float ics_psf_dt(float step, int K, float maxp, float maxg) { return ics_step_dt(ICS_FDIV(step, (float)K), maxp, maxg); }
ICS_UPD_HD float ics_psf_step_px(float p, float dtpsf, float g) { return ICS_FSUB(p, ICS_FMUL(dtpsf, g)); }
ICS_UPD_HD float ics_psf_mean3(float p0, float p1, float p2) { return ICS_FDIV(ICS_FADD(ICS_FADD(p0, p1), p2), 3.0f); }
ICS_UPD_HD float ics_psf_clamp(float p) { return p < 0.f ? 0.f : p; }
ICS_UPD_HD float ics_psf_norm(float p, float sum) { return ICS_FDIV(p, sum); }
// The sum of channel c of p[K*K][3].  The adds are a dependent chain by definition; the reads are not: 32 of them are requested before the
// adds that use them (one LDS read per add cost ~100 cycles per tap, 10 us of k_psf at 15 x 15 and 45 us at 31 x 31).
ICS_UPD_HD float ics_psf_channel_sum(const float* p, int KK, int c) {
  float s = 0.f;
  int i = 0;
  for (; i + 32 <= KK; i += 32) {
    float v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = p[3 * (i + k) + c];
#pragma unroll
    for (int k = 0; k < 32; ++k) s = ICS_FADD(s, v[k]);
  }
  for (; i < KK; ++i) s = ICS_FADD(s, p[3 * i + c]);
  return s;
}
