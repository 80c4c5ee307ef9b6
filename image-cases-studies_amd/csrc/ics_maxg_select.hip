// ics_maxg_select.hip -- the two kernels beside the operand-free mode-2 tile launch k_conv_fft<3> (ics_maxg_select.h; Route::maxg, shipped loop),
// on the channel-planar mirrors (ics_planar.hip):
//   k_update_planar_rec   the update pass A5 + A6 + A8 + A10 of k_update_planar that also records max u and max |(u - ut)/2| of the frame it writes
//   k_maxg_select         max |g| of A7 behind k_conv_fft<3>: g is formed on the tiles that can hold the maximum, and only there
// A unit of its own: in ics_planar.hip the new kernels moved an instruction of k_planar_convert<false> (scripts/isa_diff.sh).
#include "ics_kernels.h"
#include "ics_update.h"
#include "ics_maxg_select.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The same pass for runs whose mode-2 launches take no operands (ics_maxg_select.h; shipped loop): it also records, per channel and over the
// pixels it stores, the key of max u_new as maxima_keys forms it (float maximum that drops NaNs; a NaN anywhere gives the NaN key) and the
// bits of Dmax = max |(u_new - ut) 0.5| -- ut is the majoriser the next back-projection sees, except behind the last inner iteration of an
// outer one (alias_next: it will be u_new itself, the difference is 0 and nothing is recorded).  Dmax is taken as 0.5 max |u_new - ut|, one
// product at the end: x -> |fl(0.5 x)| is monotone in |x|, so the maximum of the images is the image of the maximum, and a NaN stays one.
// A thread's channel only ever grows along its walk, so it keeps one set of maxima and hands it to the channel's set when the channel changes.
// The extra arithmetic (six vector operations a pixel) is not free at 6 waves a SIMD: the operands of the next quad are requested before
// the current one is worked on, which hides most of it (4096^2: 0.172 ms k_update_planar, 0.180 recording as that kernel loops, 0.176 so).
// Wave -> workgroup -> one conditional atomic per workgroup and value, into a zeroed set.
__global__ __launch_bounds__(256) void k_update_planar_rec(IcsUpdateArgs a, int ppitch, size_t plane, uint32_t* __restrict__ rec, int alias_next) {
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
  uint32_t ku[3] = {0u, 0u, 0u}, kd[3] = {0u, 0u, 0u};   // per channel: key of max u_new, bits of max |u_new - ut|
  float cm = -__builtin_inff();                          // of the channel `cc` the thread is in: max u_new, a NaN seen, bits of max |u_new - ut|
  bool cnan = false;
  uint32_t cd = 0u;
  int cc = 0;
  auto hand_over = [&]() {
    const uint32_t k = cnan ? 0xFFC00000u : ics_f2key(cm);      // (a thread that saw no pixel of the channel: the key of -inf, below every pixel's)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (cc == q) { ku[q] = ku[q] > k ? ku[q] : k; kd[q] = kd[q] > cd ? kd[q] : cd; }
    cm = -__builtin_inff(); cnan = false; cd = 0u;
  };
  const float lambd = a.lambd;
  const int nq = (G.uN + 3) / 4;
  const long per_plane = (long)G.uM * nq, total = 3 * per_plane, stride = (long)gridDim.x * 256;
  auto place = [&](long t, int& c, int& y, int& x0) -> size_t {
    c = (int)(t / per_plane);
    const long r = t - (long)c * per_plane;
    y = (int)(r / nq); x0 = 4 * (int)(r - (long)y * nq);
    return c * plane + (size_t)y * ppitch + x0;       // (frame origin: a.u etc. point at it)
  };
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 nu = zero, nt = zero, ng = zero, nf = zero;
  int c = 0, y = 0, x0 = 0;
  size_t o = 0;
  if (t < total) {
    o = place(t, c, y, x0);
    nu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.u + o)); nt = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.ut + o));
    ng = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g + o)); nf = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.f + o));
  }
  for (; t < total; t += stride) {
    const f32x4 uq = nu, tq = nt, gq = ng, fq = nf;      // this quad: requested an iteration ago
    const int c1 = c, y1 = y, x1 = x0;
    const size_t o1 = o;
    if (t + stride < total) {
      o = place(t + stride, c, y, x0);
      nu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.u + o)); nt = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.ut + o));
      ng = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g + o)); nf = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.f + o));
    }
    const float dtc = c1 == 0 ? dt[0] : (c1 == 1 ? dt[1] : dt[2]);
    const bool yin = (y1 >= G.pad) && (y1 < G.pad + G.M);
    float un4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = x1 + e;
      const bool inside = yin && (x >= G.pad) && (x < G.pad + G.N);
      const float uv = uq[e], gv = gq[e];
      float un = ics_step_u(uv, dtc, ics_mm_g(lambd, gv, uv, tq[e]));
      if (inside) {
        const float fv = fq[e];
        const float D = ics_dof_mask(gv, fv, lambd, a.blind);
        un = ics_dof_blend(D, un, fv);
        if (a.want_dof) ICS_DOF_NOTE(dof, D);
      }
      un4[e] = un;
    }
    if (c1 != cc) { hand_over(); cc = c1; }
    if (x1 + 3 < G.uN) {
      *reinterpret_cast<f32x4*>(a.u_out + o1) = (f32x4){un4[0], un4[1], un4[2], un4[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cm = __builtin_fmaxf(cm, un4[e]); cnan |= un4[e] != un4[e];
        cd = __builtin_elementwise_max(cd, __builtin_bit_cast(uint32_t, ICS_FSUB(un4[e], tq[e])) & 0x7FFFFFFFu);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x1 + e < G.uN) {
          a.u_out[o1 + e] = un4[e];
          cm = __builtin_fmaxf(cm, un4[e]); cnan |= un4[e] != un4[e];
          cd = __builtin_elementwise_max(cd, __builtin_bit_cast(uint32_t, ICS_FSUB(un4[e], tq[e])) & 0x7FFFFFFFu);
        }
    }
  }
  hand_over();
  if (a.want_dof) ICS_DOF_FLUSH_WORKGROUP4(dof, a.dofkeys);
  __shared__ uint32_t shr[4][6];
  uint32_t v[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) { v[k] = ics_shfl_max_u32(ku[k]); v[3 + k] = ics_shfl_max_u32(alias_next ? 0u : kd[k]); }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) shr[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t m = shr[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = m > shr[w][threadIdx.x] ? m : shr[w][threadIdx.x];
    if (threadIdx.x >= 3) m = __builtin_bit_cast(uint32_t, ics_maxg_d(__builtin_bit_cast(float, m), 0.f)) & 0x7FFFFFFFu;      // Dmax = |fl(0.5 max |u_new - ut|)|
    uint32_t* dst = rec + (threadIdx.x < 3 ? ICS_MGS_UKEY + threadIdx.x : ICS_MGS_DBITS + (threadIdx.x - 3));
    if (m > *dst) atomicMax(dst, m);
  }
}

// max |g| of A7 behind the operand-free mode-2 launch (ics_maxg_select.h): a workgroup takes ICS_MGS_GROUP tiles of one channel, sixteen lanes
// a tile.  The lanes reduce the tile's wave maxima to Gt; then, for every tile of the group that the skip rule does not exclude, the whole
// workgroup forms g = ics_mm_g over the tile's pixels of the u-frame -- 16-byte quads of the three planes, the pixels the tile kernel's
// epilogue counted -- and at the end raises the iteration's key with the largest |g| it met, a NaN as the NaN key (maxima_keys).
// A tile's rows are cut into ICS_MGS_SLICES slices, one workgroup (blockIdx.z) each: few tiles are scanned -- one per channel on the benchmark
// frame --, and as ONE workgroup per tile the launch took 12 us, ten dependent round trips of its 256 threads.
// Workgroup (0, 0) also hands max u over to the reduction slot and zeroes the other set of the state for the launches to come.
#define ICS_MGS_GROUP 16
#define ICS_MGS_SLICES 8
__global__ __launch_bounds__(256) void k_maxg_select(IcsMaxgSelectArgs m) {
  const int c = blockIdx.y, tid = threadIdx.x;
  uint32_t* const st = m.state;
  if (blockIdx.x == 0 && c == 0 && blockIdx.z == 0 && tid < 8) {
    const int other = m.set ^ 1;
    if (tid < 3) m.red[ICS_RED_MAXU + tid] = st[8 * m.set + ICS_MGS_UKEY + tid];
    st[8 * other + tid] = 0u;
    if (tid < 4) st[ICS_MGS_GMAX + 4 * other + tid] = 0u;
    if (tid == 0) { st[ICS_MGS_SCANNED + other] = 0u; atomicAdd(st + ICS_MGS_LAUNCHES, 1u); }
  }
  __shared__ uint32_t sh[4];
  __shared__ int pick[ICS_MGS_GROUP];
  const int tile0 = blockIdx.x * ICS_MGS_GROUP, mine = tile0 + (tid >> 4);
  uint32_t gtb = mine < m.ntiles ? m.wkeys[((size_t)(3 * (mine >> 1) + c) * 2 + (mine & 1)) * ICS_MGS_WAVES + (tid & 15)] : 0u;
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)gtb, off, 16); gtb = gtb > o ? gtb : o; }
  const float gmax = __builtin_bit_cast(float, st[ICS_MGS_GMAX + 4 * m.set + c]), dmax = __builtin_bit_cast(float, st[8 * m.set + ICS_MGS_DBITS + c]);
  if ((tid & 15) == 0) pick[tid >> 4] = mine < m.ntiles && !ics_maxg_tile_skips(m.lambd, __builtin_bit_cast(float, gtb), gmax, dmax);
  __syncthreads();
  uint32_t ag = 0u;
  int scanned = 0;
  for (int k = 0; k < ICS_MGS_GROUP; ++k) {
    if (!pick[k]) continue;      // (uniform over the workgroup)
    ++scanned;
    const int tile = tile0 + k, ty = tile / m.tiles_x, tx = tile - ty * m.tiles_x, oy = ty * m.Vy, ox = tx * m.V;
    const int remy = m.uM - oy, remx = m.uN - ox;
    const int rows = remy <= m.Vy + m.ext_y ? remy : m.Vy, cols = remx <= m.V + m.ext_x ? remx : m.V;      // (tile_rows / tile_cols of ics_fft_tile.h)
    const int nqx = (cols + 3) >> 2;
    const int y0 = rows * (int)blockIdx.z / ICS_MGS_SLICES, y1 = rows * ((int)blockIdx.z + 1) / ICS_MGS_SLICES;
    for (int i = tid; i < (y1 - y0) * nqx; i += 256) {
      const int y = y0 + i / nqx, xq = i - (y - y0) * nqx;
      const size_t o = c * m.plane + (size_t)(oy + y) * m.ppitch + ox + 4 * xq;
      const f32x4 gq = *reinterpret_cast<const f32x4*>(m.gradu + o), uq = *reinterpret_cast<const f32x4*>(m.u + o), tq = *reinterpret_cast<const f32x4*>(m.ut + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = ics_mm_g(m.lambd, gq[e], uq[e], tq[e]);
        ag = __builtin_elementwise_max(ag, 4 * xq + e < cols ? (__builtin_bit_cast(uint32_t, g) & 0x7FFFFFFFu) : 0u);
      }
    }
  }
  if (!scanned) return;      // (uniform)
  ag = ics_shfl_max_u32(ag);
  if ((tid & 63) == 0) sh[tid >> 6] = ag;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) ag = ag > sh[w] ? ag : sh[w];
    const uint32_t kg = ag > 0x7F800000u ? 0xFFC00000u : ics_f2key(__builtin_bit_cast(float, ag));
    if (kg > m.red[ICS_RED_MAXG + c]) atomicMax(m.red + ICS_RED_MAXG + c, kg);
    if (blockIdx.z == 0) {
      atomicAdd(st + ICS_MGS_SCANNED + m.set, (uint32_t)scanned);
      atomicAdd(st + ICS_MGS_TOTAL, (uint32_t)scanned);
    }
  }
}

}  // namespace

// the update pass on planar mirrors (frame pointers of `a` = ORIGINS of planar buffers, as ics_launch_update_planar) that records into `rec`, one
// zeroed set of the ICS_MGS_* words; shipped loop only (the recording pass has no PAM branch)
hipError_t ics_launch_update_planar_rec(const IcsUpdateArgs& a, uint32_t* rec, int alias_next, hipStream_t s) {
  if (!rec || a.tv_kind) return hipErrorInvalidValue;
  long blocks = (3 * (long)a.geo.uM * ((a.geo.uN + 3) / 4) + 255) / 256;
  const long cap = (long)ics_device_cus(ics_current_device()) * ics_update_wgs_per_cu((long)a.geo.uM * a.geo.uN) * 2;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k_update_planar_rec, dim3((unsigned)blocks), dim3(256), 0, s, a, ics_ppitch(a.geo), ics_plane_floats(a.geo), rec, alias_next);
  return hipGetLastError();
}

hipError_t ics_launch_maxg_select(const IcsMaxgSelectArgs& m, hipStream_t s) {
  if (!m.gradu || !m.u || !m.ut || !m.wkeys || !m.state || !m.red || m.ntiles < 1 || (m.set & ~1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_maxg_select, dim3((unsigned)((m.ntiles + ICS_MGS_GROUP - 1) / ICS_MGS_GROUP), 3, ICS_MGS_SLICES), dim3(256), 0, s, m);
  return hipGetLastError();
}
