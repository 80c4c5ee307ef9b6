// ics_img_tvdenoise.hip -- TV (Rudin-Osher-Fatemi) denoising of device-resident images (ics_img_tv_denoise, include/ics_hip.h):
// H x W x 3 float32, HWC, contiguous.  Chambolle's dual projection iteration for min_u 1/2 |u - f|^2 + weight * TV(u) with a fixed
// number of iterations, tau = 1/8.  State: q = (qx, qy), two H x W x 3 fields that start at 0.
//
//   u        = f + div q        (div q)[y,x] = (qx[y,x] - qx[y,x-1]) + (qy[y,x] - qy[y-1,x]), terms with index -1 are 0
//   gx, gy   = u[y,x+1] - u[y,x], u[y+1,x] - u[y,x]        (0 in the last column / row)
//   s        = gx^2 + gy^2 per channel ("channel" coupling), or that summed over the three channels, smallest first ("vector")
//   q        = (q + tau g) / (1 + (tau / weight) sqrt(s))   IEEE square root and division
//
// The result is f + div q of the last q.  Every value is computed by tv_u / tv_step below in one fixed order of operations (no FMA),
// by both routes, so the routes agree bit for bit and two runs give identical bits.
//
// Route 1 (k_img_tv_iter): one launch per iteration, a lane per pixel, u recomputed on the fly from q and f at the pixel, its right
// and its lower neighbour, q ping-ponged between two frame pairs; then k_img_tv_final.  Algorithmic bytes: read q 24 + read f 12 +
// write q 24 = 60 B/px per iteration.
//
// Route 2 (k_img_tv_block): TVT iterations per launch on a 32 x 32 output tile that lives in LDS.  One iteration needs q one pixel
// further out in every direction, the closing div one more pixel up and to the left, so a workgroup stages the (32 + 1 + 2 TVT)^2
// pixels [y0 - 1 - TVT, y0 + 32 + TVT) of f and q as planes (stride 41 floats, consecutive lanes on consecutive banks) and keeps a
// fourth field u: 12 floats per pixel, 41^2 x 48 B = 80 688 B, two workgroups of 512 lanes = 16 waves per CU in 160 KB.  Iteration
// t (1 .. TVT) computes u on [t, 41 - t]^2 and then q in place on [t, 41 - t)^2: the region whose inputs are still exact shrinks by
// one pixel per side and ends on the output tile plus its upper / left neighbours.  Pixels outside the picture keep q = 0 and the
// last row / column takes g = 0 (the boundary rule above, not a mirror).  A launch writes q of its tile to the other frame pair; the
// last launch (also the one with the remainder iterations % TVT) writes f + div q instead.  Bytes per pixel and launch: read
// 36 x (41 / 32)^2 = 59, write 24 (the last: 12), against 240 for four launches of route 1.
#include "ics_img_px.h"

namespace {

#define TVB 32                         // output tile edge of the blocked route
#define TVT ICS_IMG_TV_BLOCK           // iterations per launch
#define TVS (TVB + 1 + 2 * TVT)        // staged tile edge
#define TVN (TVS * TVS)

__device__ __forceinline__ float tv_u(float f, float qx, float qxl, float qy, float qyu) {
  return __fadd_rn(f, __fadd_rn(__fsub_rn(qx, qxl), __fsub_rn(qy, qyu)));
}

// q <- (q + tau g) / (1 + k sqrt(s)), k = tau / weight; u / ur / ud: u at the pixel, right of it, below it
template <bool VEC>
__device__ __forceinline__ void tv_step(float qx[3], float qy[3], const float u[3], const float ur[3], const float ud[3], bool hasr, bool hasd,
                                        float tau, float k) {
  float gx[3], gy[3], s[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gx[c] = hasr ? __fsub_rn(ur[c], u[c]) : 0.f;
    gy[c] = hasd ? __fsub_rn(ud[c], u[c]) : 0.f;
    s[c] = __fadd_rn(__fmul_rn(gx[c], gx[c]), __fmul_rn(gy[c], gy[c]));
  }
  if (VEC) {   // summed in ascending order: the same value for every order of the channels
    const float lo = fminf(s[0], s[1]), hi = fmaxf(s[0], s[1]);
    s[0] = s[1] = s[2] = __fadd_rn(__fadd_rn(fminf(lo, s[2]), fmaxf(lo, fminf(hi, s[2]))), fmaxf(hi, s[2]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float den = __fadd_rn(1.f, __fmul_rn(k, __fsqrt_rn(s[c])));
    qx[c] = __fdiv_rn(__fadd_rn(qx[c], __fmul_rn(tau, gx[c])), den);
    qy[c] = __fdiv_rn(__fadd_rn(qy[c], __fmul_rn(tau, gy[c])), den);
  }
}

__device__ __forceinline__ void zero3(float v[3]) { v[0] = v[1] = v[2] = 0.f; }

// ---- route 1: one iteration; qxi == nullptr: q = 0 (the first iteration) ----------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_img_tv_iter(const float* __restrict__ f, const float* __restrict__ qxi, const float* __restrict__ qyi,
                                                    float* __restrict__ qxo, float* __restrict__ qyo, int H, int W, float tau, float k) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long L = 3L * W, p = (long)y * L + 3L * x;
  const bool hasr = x + 1 < W, hasd = y + 1 < H, hasl = x > 0, hasu = y > 0;
  float F[3], Fr[3], Fd[3], qx[3], qxl[3], qy[3], qyu[3], qxr[3], qyr[3], qyur[3], qxd[3], qxdl[3], qyd[3];
  ld3(f + p, F);
  zero3(Fr); zero3(Fd);
  if (hasr) ld3(f + p + 3, Fr);
  if (hasd) ld3(f + p + L, Fd);
  zero3(qx); zero3(qxl); zero3(qy); zero3(qyu); zero3(qxr); zero3(qyr); zero3(qyur); zero3(qxd); zero3(qxdl); zero3(qyd);
  if (qxi) {
    ld3(qxi + p, qx); ld3(qyi + p, qy);
    if (hasl) ld3(qxi + p - 3, qxl);
    if (hasu) ld3(qyi + p - L, qyu);
    if (hasr) {
      ld3(qxi + p + 3, qxr); ld3(qyi + p + 3, qyr);
      if (hasu) ld3(qyi + p + 3 - L, qyur);
    }
    if (hasd) {
      ld3(qxi + p + L, qxd); ld3(qyi + p + L, qyd);
      if (hasl) ld3(qxi + p + L - 3, qxdl);
    }
  }
  float u[3], ur[3], ud[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    u[c] = tv_u(F[c], qx[c], qxl[c], qy[c], qyu[c]);
    ur[c] = tv_u(Fr[c], qxr[c], qx[c], qyr[c], qyur[c]);
    ud[c] = tv_u(Fd[c], qxd[c], qxdl[c], qyd[c], qy[c]);
  }
  tv_step<VEC>(qx, qy, u, ur, ud, hasr, hasd, tau, k);
  st3(qxo + p, qx); st3(qyo + p, qy);
}

// out = f + div q
__global__ __launch_bounds__(256) void k_img_tv_final(const float* __restrict__ f, const float* __restrict__ qxi, const float* __restrict__ qyi,
                                                     float* __restrict__ out, int H, int W) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long L = 3L * W, p = (long)y * L + 3L * x;
  float F[3], qx[3], qxl[3], qy[3], qyu[3], u[3];
  ld3(f + p, F); ld3(qxi + p, qx); ld3(qyi + p, qy);
  zero3(qxl); zero3(qyu);
  if (x > 0) ld3(qxi + p - 3, qxl);
  if (y > 0) ld3(qyi + p - L, qyu);
#pragma unroll
  for (int c = 0; c < 3; ++c) u[c] = tv_u(F[c], qx[c], qxl[c], qy[c], qyu[c]);
  st3(out + p, u);
}

// ---- route 2: n <= TVT iterations on an LDS tile; qxi == nullptr: q = 0; out != nullptr: the last launch, writes f + div q -----
template <bool VEC>
__global__ __launch_bounds__(512) void k_img_tv_block(const float* __restrict__ f, const float* __restrict__ qxi, const float* __restrict__ qyi,
                                                     float* __restrict__ qxo, float* __restrict__ qyo, float* __restrict__ out, int H, int W, int n,
                                                     float tau, float k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sf = lds, *sqx = lds + 3 * TVN, *sqy = lds + 6 * TVN, *su = lds + 9 * TVN;    // planes [c][TVS][TVS]
  const int y0 = blockIdx.y * TVB - 1 - TVT, x0 = blockIdx.x * TVB - 1 - TVT;          // picture coordinates of tile position (0, 0)
  const long L = 3L * W;
  for (int e = threadIdx.x; e < TVN; e += 512) {
    const int ly = e / TVS, lx = e - ly * TVS, y = y0 + ly, x = x0 + lx;
    float F[3], qx[3], qy[3];
    zero3(F); zero3(qx); zero3(qy);
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const long p = (long)y * L + 3L * x;
      ld3(f + p, F);
      if (qxi) { ld3(qxi + p, qx); ld3(qyi + p, qy); }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { sf[c * TVN + e] = F[c]; sqx[c * TVN + e] = qx[c]; sqy[c * TVN + e] = qy[c]; }
  }
  __syncthreads();
  for (int t = TVT - n + 1; t <= TVT; ++t) {
    const int mu = TVS - 2 * t + 1;                      // u on [t, TVS - t]^2
    const float inv_mu = 1.f / (float)mu;
    for (int e = threadIdx.x; e < mu * mu; e += 512) {
      const int r = (int)(((float)e + 0.5f) * inv_mu), i = (t + r) * TVS + t + (e - r * mu);
#pragma unroll
      for (int c = 0; c < 3; ++c) su[c * TVN + i] = tv_u(sf[c * TVN + i], sqx[c * TVN + i], sqx[c * TVN + i - 1], sqy[c * TVN + i], sqy[c * TVN + i - TVS]);
    }
    __syncthreads();
    const int mq = mu - 1;                               // q on [t, TVS - t)^2, in place
    const float inv_mq = 1.f / (float)mq;
    for (int e = threadIdx.x; e < mq * mq; e += 512) {
      const int r = (int)(((float)e + 0.5f) * inv_mq), ly = t + r, lx = t + (e - r * mq), i = ly * TVS + lx;
      const int y = y0 + ly, x = x0 + lx;
      if (y < 0 || y >= H || x < 0 || x >= W) continue;  // outside the picture q stays 0
      float qx[3], qy[3], u[3], ur[3], ud[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        qx[c] = sqx[c * TVN + i]; qy[c] = sqy[c * TVN + i];
        u[c] = su[c * TVN + i]; ur[c] = su[c * TVN + i + 1]; ud[c] = su[c * TVN + i + TVS];
      }
      tv_step<VEC>(qx, qy, u, ur, ud, x + 1 < W, y + 1 < H, tau, k);
#pragma unroll
      for (int c = 0; c < 3; ++c) { sqx[c * TVN + i] = qx[c]; sqy[c * TVN + i] = qy[c]; }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < TVB * TVB; e += 512) {
    const int ly = TVT + 1 + e / TVB, lx = TVT + 1 + e % TVB, i = ly * TVS + lx, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const long p = (long)y * L + 3L * x;
    float a[3], b[3];
    if (out) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] = tv_u(sf[c * TVN + i], sqx[c * TVN + i], sqx[c * TVN + i - 1], sqy[c * TVN + i], sqy[c * TVN + i - TVS]);
      st3(out + p, a);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) { a[c] = sqx[c * TVN + i]; b[c] = sqy[c * TVN + i]; }
      st3(qxo + p, a); st3(qyo + p, b);
    }
  }
}

}  // namespace

size_t ics_img_tv_block_lds() { return (size_t)12 * TVN * sizeof(float); }

// frame pairs (qx, qy) a run needs: the last blocked launch writes the result, not q
int ics_img_tv_pairs(int iterations, int route) {
  const int writes = route == 2 ? (iterations + TVT - 1) / TVT - 1 : iterations;
  return writes < 2 ? writes : 2;
}

hipError_t ics_launch_img_tv_denoise(const float* f, int H, int W, float weight, int iterations, int coupling, int route, float* const q[4],
                                     float* out, hipStream_t s) {
  const float tau = 0.125f, k = tau / weight;
  if (iterations < 1 || (route != 1 && route != 2)) return hipErrorInvalidValue;
  const float *qxi = nullptr, *qyi = nullptr;
  if (route == 1) {
    const dim3 grid((W + 63) / 64, (H + 3) / 4);
    for (int it = 0; it < iterations; ++it) {
      float *qxo = q[2 * (it & 1)], *qyo = q[2 * (it & 1) + 1];
      ICS_LAUNCH_VEC(coupling, k_img_tv_iter, grid, dim3(256), 0, s, f, qxi, qyi, qxo, qyo, H, W, tau, k);
      qxi = qxo; qyi = qyo;
    }
    hipLaunchKernelGGL(k_img_tv_final, grid, dim3(256), 0, s, f, qxi, qyi, out, H, W);
    return hipGetLastError();
  }
  const size_t lds = ics_img_tv_block_lds();
  hipError_t e = coupling ? set_dynamic_lds(k_img_tv_block<true>, lds) : set_dynamic_lds(k_img_tv_block<false>, lds);
  if (e != hipSuccess) return e;
  const dim3 grid((W + TVB - 1) / TVB, (H + TVB - 1) / TVB);
  const int launches = (iterations + TVT - 1) / TVT;
  for (int j = 0, done = 0; j < launches; ++j) {
    const bool last = j == launches - 1;
    const int n = iterations - done < TVT ? iterations - done : TVT;
    float *qxo = last ? nullptr : q[2 * (j & 1)], *qyo = last ? nullptr : q[2 * (j & 1) + 1], *o = last ? out : nullptr;
    ICS_LAUNCH_VEC(coupling, k_img_tv_block, grid, dim3(512), lds, s, f, qxi, qyi, qxo, qyo, o, H, W, n, tau, k);
    qxi = qxo; qyi = qyo; done += n;
  }
  return hipGetLastError();
}
