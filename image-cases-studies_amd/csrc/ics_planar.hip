// ics_planar.hip -- channel-planar mirrors of the job's frames (ics_common.h: ics_ppitch, ics_plane_floats) for the FFT-tile pipeline
// (ics_conv_fft.hip; ics_job.hip "FFT-tile pipeline: mirrors").
//
// The overlap-save FFT convolution works on one channel of a tile pair at a time; from HWC frames every access touches 4 of each 12 bytes
// and a work unit pulls three times its useful cache lines through the CU's miss path (measured: 30 k of a unit's 70 k shader clocks in the
// window loads alone).  During a run that uses it, the frames therefore live as three planes each, and the kernels between the
// convolutions run on the planes as well:
//   k_hwc_to_planar / k_planar_to_hwc   run boundaries (whole frames), and the stop-test window (A18 / A19 read HWC frames)
//   k_update_planar                     A5 + A6 + A8 + A10 (lib/deconvolution.pyx:499-552) -- the functions of ics_update.h, as k_update_rows
//                                       applies them: bit-identical to the HWC pass
// The PSF gradient reads planes through a template flag of its own kernel (ics_gradk_mfma.hip).
#include "ics_kernels.h"
#include "ics_update.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One thread = 4 consecutive pixels of a buffer row: 3 dwordx4 of HWC <-> one dwordx4 per plane.  Rows [r0, r1) and pixel groups [q0, q1)
// in BUFFER coordinates (row 0 = first allocated row, pixel 0 = first pixel of a row; ax is a multiple of 4, so frame pixel 0 starts a group).
template <bool TO_PLANAR>
__global__ __launch_bounds__(256) void k_planar_convert(const float* __restrict__ src, float* __restrict__ dst, int pitch, int ppitch, size_t plane,
                                                        int r0, int r1, int q0, int q1) {
  const int nq = q1 - q0;
  const long total = (long)(r1 - r0) * nq;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int row = r0 + (int)(t / nq), q = q0 + (int)(t - (long)(row - r0) * nq);
    const size_t oh = (size_t)row * pitch + 12 * (size_t)q, op = (size_t)row * ppitch + 4 * (size_t)q;
    const bool in_hwc = 12 * q + 11 < pitch;       // (the last groups of a plane row can lie beyond the HWC row: zeros)
    if (TO_PLANAR) {
      float v[12];
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const f32x4 a = in_hwc ? *reinterpret_cast<const f32x4*>(src + oh + 4 * h) : (f32x4){0.f, 0.f, 0.f, 0.f};
        v[4 * h] = a.x; v[4 * h + 1] = a.y; v[4 * h + 2] = a.z; v[4 * h + 3] = a.w;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(dst + c * plane + op) = (f32x4){v[c], v[3 + c], v[6 + c], v[9 + c]};
    } else if (in_hwc) {
      float v[12];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + c * plane + op);
        v[c] = a.x; v[3 + c] = a.y; v[6 + c] = a.z; v[9 + c] = a.w;
      }
#pragma unroll
      for (int h = 0; h < 3; ++h) *reinterpret_cast<f32x4*>(dst + oh + 4 * h) = (f32x4){v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
    }
  }
}

// A5 + A6 + A8 + A10 (ics_update.h) on planes: one thread = 4 consecutive pixels of one channel row (dwordx4 per operand).
__global__ __launch_bounds__(256) void k_update_planar(IcsUpdateArgs a, int ppitch, size_t plane) {
  const IcsGeom& G = a.geo;
  float dt[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float maxu = ics_key2f(a.red[ICS_RED_MAXU + c]);
    const float maxg = ics_key2f(a.red[ICS_RED_MAXG + c]);
    dt[c] = ics_step_dt(a.step, maxu, maxg);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.scal[ICS_SC_DT + c] = dt[c]; a.scal[ICS_SC_MAXU + c] = maxu; a.scal[ICS_SC_MAXG + c] = maxg;
    }
  }
  IcsDofKeys dof = ICS_DOF_NONE;
  const float lambd = a.lambd;
  const int nq = (G.uN + 3) / 4;
  const long per_plane = (long)G.uM * nq, total = 3 * per_plane;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t / per_plane);
    const long r = t - (long)c * per_plane;
    const int y = (int)(r / nq), x0 = 4 * (int)(r - (long)y * nq);
    const size_t o = c * plane + (size_t)y * ppitch + x0;       // (frame origin: a.u etc. point at it)
    const f32x4 uq = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.u + o));
    const f32x4 tq = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.ut + o));
    const f32x4 gq = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g + o));
    const f32x4 fq = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.f + o));
    const float dtc = c == 0 ? dt[0] : (c == 1 ? dt[1] : dt[2]);
    const bool yin = (y >= G.pad) && (y < G.pad + G.M);
    float un4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = x0 + e;
      const bool inside = yin && (x >= G.pad) && (x < G.pad + G.N);
      const float uv = uq[e], gv = gq[e];
      // (PAM kinds: the back-projection wrote G = T + lambd gradu; no DoF blend -- k_update_rows, ics_kernels.hip)
      const float g = a.tv_kind >= 2 ? gv : ics_mm_g(lambd, gv, uv, tq[e]);
      float un = ics_step_u(uv, dtc, g);
      if (inside && a.tv_kind < 2) {
        const float fv = fq[e];
        const float D = ics_dof_mask(gv, fv, lambd, a.blind);
        un = ics_dof_blend(D, un, fv);
        if (a.want_dof) ICS_DOF_NOTE(dof, D);
      }
      un4[e] = un;
    }
    if (x0 + 3 < G.uN) *reinterpret_cast<f32x4*>(a.u_out + o) = (f32x4){un4[0], un4[1], un4[2], un4[3]};
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x0 + e < G.uN) a.u_out[o + e] = un4[e];
    }
  }
  if (a.want_dof) ICS_DOF_FLUSH_WORKGROUP4(dof, a.dofkeys);
}

}  // namespace

// `hwc` / `planar`: buffer STARTS (not origins).  Rows [y0, y1) and pixels [x0, x1) in u-frame coordinates, widened to whole 4-pixel groups
// and clipped to the buffer; whole = every allocated row and pixel (aprons included).
hipError_t ics_launch_planar_convert(bool to_planar, const float* src, float* dst, const IcsGeom& g, bool whole, int y0, int y1, int x0, int x1, hipStream_t s) {
  const int pp = ics_ppitch(g);
  int r0 = 0, r1 = g.rows, q0 = 0, q1 = pp / 4;
  if (!whole) {
    r0 = g.ay + y0; r1 = g.ay + y1;
    r0 = r0 < 0 ? 0 : r0; r1 = r1 > g.rows ? g.rows : r1;
    q0 = (g.ax + x0) / 4; q1 = (g.ax + x1 + 3) / 4;
    q0 = q0 < 0 ? 0 : q0; q1 = q1 > pp / 4 ? pp / 4 : q1;
  }
  if (r1 <= r0 || q1 <= q0) return hipSuccess;
  const long total = (long)(r1 - r0) * (q1 - q0);
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (to_planar) hipLaunchKernelGGL(k_planar_convert<true>, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, g.pitch, pp, ics_plane_floats(g), r0, r1, q0, q1);
  else hipLaunchKernelGGL(k_planar_convert<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, g.pitch, pp, ics_plane_floats(g), r0, r1, q0, q1);
  return hipGetLastError();
}

// the update pass on planar mirrors: the frame pointers of `a` are ORIGINS of planar buffers (plane 0)
hipError_t ics_launch_update_planar(const IcsUpdateArgs& a, hipStream_t s) {
  long blocks = (3 * (long)a.geo.uM * ((a.geo.uN + 3) / 4) + 255) / 256;
  const long cap = (long)ics_device_cus(ics_current_device()) * ics_update_wgs_per_cu((long)a.geo.uM * a.geo.uN) * 2;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k_update_planar, dim3((unsigned)blocks), dim3(256), 0, s, a, ics_ppitch(a.geo), ics_plane_floats(a.geo));
  return hipGetLastError();
}
