// ics_img_tvdeconv.hip -- TV-regularised deconvolution of a device-resident image by a known PSF (ics_img_tv_deconvolve,
// include/ics_hip.h): minimise sum |Du| + (mu / 2) |h * u - f|^2 by variable splitting (FTVd of Wang, Yang, Yin, Zhang in its
// split-Bregman / ADMM form, Goldstein and Osher), every iteration one per-pixel shrinkage and one linear solve that is diagonal under
// the 2-D transform.  H x W x 3 float32, HWC; the PSF K x K per channel, every channel of sum 1.  fp32, no atomics, every sum in one
// fixed order: two runs give identical bits.  Restated in float64 in tests/tv_deconv_ref.py.
//
//   Py, Px, ext, Hc, L : as in ics_img_wiener.hip (L = 4 sin^2(pi ky / Py) + 4 sin^2(pi kx / Px) is the transfer of D^T D, exactly)
//   N0c = mu conj(Hc) transform(ext_c),  Gc = 1 / (mu |Hc|^2 + beta L),  u = ext, bx = by = 0;  n times, indices mod Px, Py:
//     vx = u[y, x+1] - u[y, x] + bx,  vy = u[y+1, x] - u[y, x] + by
//     m  = sqrt(vx^2 + vy^2), per value ("channel") or summed over the three channels too ("vector");  s = (m - 1/beta) / m above 1/beta, else 0
//     wx = s vx, wy = s vy;  bx = vx - wx, by = vy - wy;  px = wx - bx, py = wy - by
//     z  = (px[y, x-1] - px[y, x]) + (py[y-1, x] - py[y, x])
//     u_c = real(inverse transform((N0c + beta transform(z_c)) Gc))
//   out = u[:H, :W], nothing clipped
//
// One workspace: two spectrum frames A, B and N0 (3 Py Px float2 each, N0 and the spectra behind the first transpose as [c][kx][ky]),
// G (3 Py Px float, [c][kx][ky], scaled by 1 / (Py Px)), two pairs of b planes and the tables of ics_img_wiener.hip.  u and z are the
// two halves of B, real planes [3][Py][Px]: B holds a spectrum only between the two transposes of an iteration, u lives from the
// inverse rows to the shrink pass and z from the shrink pass to the forward rows.  b ping-pongs between its two pairs: a tile reads
// the b of a one-pixel rim that belongs to its neighbours, and in place those might have written theirs already.
//
// The tables and the tiled transpose are the Wiener unit's (ics_launch_img_wiener_tables, ics_launch_img_wiener_transpose).
// Setup: the tables, k_img_tvd_extend (ext -> u, 0 -> b), k_img_tvd_rows (u -> A), a transpose (A -> N0), k_img_tvd_psf_rows,
// k_img_tvd_psf_cols (mu conj(Hc) -> A, Gc / (Py Px) -> G), k_img_tvd_n0 (the line of N0 forward, times A, in place).
// An iteration: k_img_tvd_shrink (u, b -> b', z), k_img_tvd_rows (z -> A), a transpose (A -> B), k_img_tvd_cols (the line of B forward,
// (N0 + beta Z) G, inverse, in place), a transpose (B -> A, all Py rows: the domain is periodic; the last iteration the rows below H
// only), k_img_tvd_inv_rows (A -> u, all Px points; the last iteration the first W points of the rows below H -> out).
#include "ics_img_px.h"
#include "ics_wn_fft.h"

namespace {

#define TVD_LANES 1024                         // lanes of a line's workgroup at most (N / 4 below 4096 points, 64 at least)
#define TVD_TW 64                              // the shrink pass: pixels of a tile along x
#define TVD_TH 16                              //                  and along y; 256 lanes, four pixels each

// grid (3, Py): row y of channel c of the extended frame -> u[c][y][:] (the arithmetic of the Wiener unit's row kernel), zeros -> bx[c][y][:], by[c][y][:]
__global__ __launch_bounds__(256) void k_img_tvd_extend(const float* __restrict__ f, int H, int W, int Py, int Px, float* __restrict__ u, float* __restrict__ bx,
                                                        float* __restrict__ by) {
  const int c = blockIdx.x, y = blockIdx.y;
  const long pitch = 3L * W;
  const bool ext = y >= H;
  const float* r0 = f + (long)(ext ? H - 1 : y) * pitch + c;   // the row itself, or the last one
  const float* r1 = f + c;                                     // the first one
  const float ty = ext ? (float)(y - H + 1) / (float)(Py - H + 1) : 0.f;
  const auto px = [&](int x) { return ext ? (1.f - ty) * r0[3L * x] + ty * r1[3L * x] : r0[3L * x]; };
  const float last = px(W - 1), first = px(0), gx = (float)(Px - W + 1);
  const long row = ((long)c * Py + y) * Px;
  for (int j = threadIdx.x; j < Px; j += 256) {
    float v;
    if (j < W) v = px(j);
    else { const float t = (float)(j - W + 1) / gx; v = (1.f - t) * last + t * first; }
    u[row + j] = v;
    bx[row + j] = 0.f;
    by[row + j] = 0.f;
  }
}

// grid (3, Py): the real row p[c][y][:] -> its transform A[c][y][:]
__global__ __launch_bounds__(TVD_LANES) void k_img_tvd_rows(const float* __restrict__ p, int Py, int Px, int logPx, const float2* __restrict__ tw, float2* __restrict__ A) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long row = ((long)blockIdx.x * Py + blockIdx.y) * Px;
  for (int j = tid; j < Px; j += nthr) sm[j] = make_float2(p[row + j], 0.f);
  __syncthreads();
  const float2* r = wn_fft<false>(sm, sm + Px, Px, logPx, tw);
  for (int j = tid; j < Px; j += nthr) A[row + j] = r[j];
}

// grid (K, 3): row r of channel c of the PSF (planar, [3][K][K]), zero padded to Px points, tap K / 2 at point 0 -> Hr[c][r][:]
__global__ __launch_bounds__(TVD_LANES) void k_img_tvd_psf_rows(const float* __restrict__ psf, int K, int Px, int logPx, const float2* __restrict__ tw,
                                                                float2* __restrict__ Hr) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int r = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const float* p = psf + ((long)c * K + r) * K;
  for (int j = tid; j < Px; j += nthr) {
    int t = j + K / 2;
    if (t >= Px) t -= Px;
    sm[j] = make_float2(t < K ? p[t] : 0.f, 0.f);
  }
  __syncthreads();
  const float2* q = wn_fft<false>(sm, sm + Px, Px, logPx, tw);
  float2* o = Hr + ((long)c * K + r) * Px;
  for (int j = tid; j < Px; j += nthr) o[j] = q[j];
}

// grid (Px, 3): column kx of Hc; mu conj(Hc) -> Hm[c][kx][:], scale / (mu |Hc|^2 + beta L) -> G[c][kx][:] (scale = 1 / (Py Px), a power
// of two: exact.  The denominator is mu at (0, 0), where L is 0 and Hc the channel's sum, and positive everywhere)
__global__ __launch_bounds__(TVD_LANES) void k_img_tvd_psf_cols(const float2* __restrict__ Hr, int K, int Py, int Px, int logPy, const float2* __restrict__ tw,
                                                                const float* __restrict__ lamy, const float* __restrict__ lamx, float mu, float beta, float scale,
                                                                float2* __restrict__ Hm, float* __restrict__ G) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int kx = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const float2* h = Hr + (long)c * K * Px + kx;
  for (int j = tid; j < Py; j += nthr) {
    int t = j + K / 2;
    if (t >= Py) t -= Py;
    sm[j] = t < K ? h[(long)t * Px] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const float2* q = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  const float lx = lamx[kx];
  const long line = ((long)c * Px + kx) * Py;
  for (int j = tid; j < Py; j += nthr) {
    const float2 v = q[j];
    const float den = __fadd_rn(__fmul_rn(mu, __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y))), __fmul_rn(beta, __fadd_rn(lamy[j], lx)));
    Hm[line + j] = make_float2(__fmul_rn(mu, v.x), __fmul_rn(mu, -v.y));
    G[line + j] = __fdiv_rn(scale, den);
  }
}

// grid (Px, 3): the line N0[c][kx][:] (the transposed row transforms of ext) forward, times Hm -> N0, in place
__global__ __launch_bounds__(TVD_LANES) void k_img_tvd_n0(float2* __restrict__ N0, const float2* __restrict__ Hm, int Py, int logPy, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  for (int j = tid; j < Py; j += nthr) sm[j] = N0[line + j];
  __syncthreads();
  const float2* r = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) N0[line + j] = wn_mul(Hm[line + j], r[j]);
}

// grid (ceil(Px / TVD_TW), ceil(Py / TVD_TH)): the shrinkage of one tile and its z.  p is formed on the tile and on the one-pixel rim
// above and left of it (z takes the p of the left and of the upper neighbour), from u on the tile and one pixel around it; the rim's b
// is only read.  bx0, by0 -> bx1, by1 (other planes: see the head of this file)
template <bool VEC>
__global__ __launch_bounds__(256) void k_img_tvd_shrink(const float* __restrict__ u, const float* __restrict__ bx0, const float* __restrict__ by0, float* __restrict__ bx1,
                                                        float* __restrict__ by1, float* __restrict__ z, int Py, int Px, float thr) {
  constexpr int UW = TVD_TW + 2, UH = TVD_TH + 2, PW = TVD_TW + 1, PH = TVD_TH + 1;
  __shared__ float su[3][UH][UW];              // u at (y0 - 1 + r, x0 - 1 + q)
  __shared__ float sp[2][3][PH][PW];           // px, py at (y0 - 1 + r, x0 - 1 + q)
  const int x0 = blockIdx.x * TVD_TW, y0 = blockIdx.y * TVD_TH, tid = threadIdx.x;
  const long plane = (long)Py * Px;
  for (int i = tid; i < 3 * UH * UW; i += 256) {
    const int c = i / (UH * UW), k = i - c * (UH * UW), r = k / UW, q = k - r * UW;
    su[c][r][q] = u[c * plane + (long)((y0 - 1 + r) & (Py - 1)) * Px + ((x0 - 1 + q) & (Px - 1))];
  }
  __syncthreads();
  for (int i = tid; i < PH * PW; i += 256) {
    const int r = i / PW, q = i - r * PW;
    const int y = y0 - 1 + r, x = x0 - 1 + q;
    const long at = (long)(y & (Py - 1)) * Px + (x & (Px - 1));
    const bool own = r > 0 && q > 0 && y < Py && x < Px;
    float vx[3], vy[3], mm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float here = su[c][r][q];
      vx[c] = __fadd_rn(__fsub_rn(su[c][r][q + 1], here), bx0[c * plane + at]);
      vy[c] = __fadd_rn(__fsub_rn(su[c][r + 1][q], here), by0[c * plane + at]);
      mm[c] = __fadd_rn(__fmul_rn(vx[c], vx[c]), __fmul_rn(vy[c], vy[c]));
    }
    if (VEC) mm[0] = mm[1] = mm[2] = __fadd_rn(__fadd_rn(mm[0], mm[1]), mm[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = __fsqrt_rn(mm[c]);
      const float s = m > thr ? __fdiv_rn(__fsub_rn(m, thr), m) : 0.f;
      const float wx = __fmul_rn(s, vx[c]), wy = __fmul_rn(s, vy[c]);
      const float bx = __fsub_rn(vx[c], wx), by = __fsub_rn(vy[c], wy);
      sp[0][c][r][q] = __fsub_rn(wx, bx);
      sp[1][c][r][q] = __fsub_rn(wy, by);
      if (own) { bx1[c * plane + at] = bx; by1[c * plane + at] = by; }
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * TVD_TH * TVD_TW; i += 256) {
    const int c = i / (TVD_TH * TVD_TW), k = i - c * (TVD_TH * TVD_TW), r = k / TVD_TW + 1, q = (k & (TVD_TW - 1)) + 1;
    const int y = y0 - 1 + r, x = x0 - 1 + q;
    if (y < Py && x < Px)
      z[c * plane + (long)y * Px + x] = __fadd_rn(__fsub_rn(sp[0][c][r][q - 1], sp[0][c][r][q]), __fsub_rn(sp[1][c][r - 1][q], sp[1][c][r][q]));
  }
}

// grid (Px, 3): the line B[c][kx][:] forward, (N0 + beta Z) G, inverse, the line staying in LDS in between; written back in place
__global__ __launch_bounds__(TVD_LANES) void k_img_tvd_cols(float2* __restrict__ B, const float2* __restrict__ N0, const float* __restrict__ G, float beta, int Py, int logPy,
                                                            const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  float2* l = B + line;
  for (int j = tid; j < Py; j += nthr) sm[j] = l[j];
  __syncthreads();
  float2* r = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) {
    const float2 zz = r[j], n = N0[line + j];
    const float g = G[line + j];
    r[j] = make_float2(__fmul_rn(__fadd_rn(n.x, __fmul_rn(beta, zz.x)), g), __fmul_rn(__fadd_rn(n.y, __fmul_rn(beta, zz.y)), g));
  }
  __syncthreads();
  const float2* q = wn_fft<true>(r, r == sm ? sm + Py : sm, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) l[j] = q[j];
}

// grid (3, rows): A[c][y][:] inverse, the real part of the first n points -> dst[c * chan + y * pitch + j * step] (u: chan Py Px, pitch
// Px, step 1, n Px on all Py rows; the result image: chan 1, pitch 3 W, step 3, n W on the rows below H)
__global__ __launch_bounds__(TVD_LANES) void k_img_tvd_inv_rows(const float2* __restrict__ A, int Py, int Px, int logPx, const float2* __restrict__ tw, float* __restrict__ dst,
                                                                long chan, long pitch, int step, int n) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int c = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const float2* l = A + ((long)c * Py + y) * Px;
  for (int j = tid; j < Px; j += nthr) sm[j] = l[j];
  __syncthreads();
  const float2* q = wn_fft<true>(sm, sm + Px, Px, logPx, tw);
  float* o = dst + c * chan + y * pitch;
  for (int j = tid; j < n; j += nthr) o[(long)j * step] = q[j].x;
}

int tvd_log2(int v) { int k = 0; while ((1 << k) < v) ++k; return k; }
int tvd_lanes(int P) { const int t = P / 4; return t < 64 ? 64 : (t > TVD_LANES ? TVD_LANES : t); }

}  // namespace

// the one block of a call: A, B, N0 (a spectrum frame each), G (half of one), the two pairs of b planes (half of one each), the tables
size_t ics_img_tvd_workspace_bytes(int K, int Py, int Px) {
  return (size_t)33 * Py * Px * sizeof(float) + ics_img_wiener_table_bytes(K, Py, Px);
}
void* ics_img_tvd_tables(void* workspace, int Py, int Px) { return reinterpret_cast<float*>(workspace) + (size_t)33 * Py * Px; }

hipError_t ics_launch_img_tv_deconvolve(const float* f, int H, int W, int K, float mu, float beta, int iterations, int coupling, int Py, int Px, void* workspace, float* out,
                                        hipStream_t s) {
  if (!f || !workspace || !out || H < 1 || W < 1 || K < 3 || !(K & 1) || K > H || K > W || iterations < 1) return hipErrorInvalidValue;
  if (Py < H + K - 1 || Px < W + K - 1 || Py > ICS_IMG_WIENER_MAX || Px > ICS_IMG_WIENER_MAX || (Py & (Py - 1)) || (Px & (Px - 1))) return hipErrorInvalidValue;
  const int logPy = tvd_log2(Py), logPx = tvd_log2(Px);
  const size_t plane3 = (size_t)3 * Py * Px;                  // floats of three real planes; a spectrum frame is two of them
  float* w = reinterpret_cast<float*>(workspace);
  float2 *A = reinterpret_cast<float2*>(w), *B = reinterpret_cast<float2*>(w + 2 * plane3), *N0 = reinterpret_cast<float2*>(w + 4 * plane3);
  float *G = w + 6 * plane3, *u = w + 2 * plane3, *z = w + 3 * plane3;   // (u, z: the halves of B)
  float *bx[2] = {w + 7 * plane3, w + 9 * plane3}, *by[2] = {w + 8 * plane3, w + 10 * plane3};
  float2* Hr = reinterpret_cast<float2*>(ics_img_tvd_tables(workspace, Py, Px));
  float2* twy = Hr + (size_t)3 * K * Px;
  float2* twx = twy + Py;
  float* lamy = reinterpret_cast<float*>(twx + Px);
  float* lamx = lamy + Py;
  const float* psf = lamx + Px;                  // (== ics_img_wiener_psf_slot of the tables: uploaded by the caller)
  const size_t ldsy = ics_img_wiener_lds(Py), ldsx = ics_img_wiener_lds(Px);
  if (ldsy > 64 * 1024 || ldsx > 64 * 1024) {    // lines of 8192 points: 128 KB of dynamic LDS
    static std::atomic<bool> cfg[6][ICS_MAX_DEVICES];
    const int dev = ics_current_device();
    const size_t top = ics_img_wiener_lds(ICS_IMG_WIENER_MAX);
    hipError_t e = ics_configure_lds(cfg[0], dev, k_img_tvd_rows, top);
    if (e == hipSuccess) e = ics_configure_lds(cfg[1], dev, k_img_tvd_psf_rows, top);
    if (e == hipSuccess) e = ics_configure_lds(cfg[2], dev, k_img_tvd_psf_cols, top);
    if (e == hipSuccess) e = ics_configure_lds(cfg[3], dev, k_img_tvd_n0, top);
    if (e == hipSuccess) e = ics_configure_lds(cfg[4], dev, k_img_tvd_cols, top);
    if (e == hipSuccess) e = ics_configure_lds(cfg[5], dev, k_img_tvd_inv_rows, top);
    if (e != hipSuccess) return e;
  }
  const float scale = 1.f / ((float)Py * (float)Px), thr = 1.f / beta;
  const dim3 rows(3, (unsigned)Py), cols((unsigned)Px, 3), shrink((unsigned)((Px + TVD_TW - 1) / TVD_TW), (unsigned)((Py + TVD_TH - 1) / TVD_TH));
  ics_launch_img_wiener_tables(twy, twx, lamy, lamx, Py, Px, s);
  hipLaunchKernelGGL(k_img_tvd_extend, rows, dim3(256), 0, s, f, H, W, Py, Px, u, bx[0], by[0]);
  hipLaunchKernelGGL(k_img_tvd_rows, rows, dim3(tvd_lanes(Px)), ldsx, s, u, Py, Px, logPx, twx, A);
  ics_launch_img_wiener_transpose(A, Py, Px, Px, N0, s);
  hipLaunchKernelGGL(k_img_tvd_psf_rows, dim3((unsigned)K, 3), dim3(tvd_lanes(Px)), ldsx, s, psf, K, Px, logPx, twx, Hr);
  hipLaunchKernelGGL(k_img_tvd_psf_cols, cols, dim3(tvd_lanes(Py)), ldsy, s, Hr, K, Py, Px, logPy, twy, lamy, lamx, mu, beta, scale, A, G);
  hipLaunchKernelGGL(k_img_tvd_n0, cols, dim3(tvd_lanes(Py)), ldsy, s, N0, A, Py, logPy, twy);
  for (int it = 0; it < iterations; ++it) {
    const int from = it & 1, to = from ^ 1;
    const bool last = it == iterations - 1;
    ICS_LAUNCH_VEC(coupling, k_img_tvd_shrink, shrink, dim3(256), 0, s, u, bx[from], by[from], bx[to], by[to], z, Py, Px, thr);
    hipLaunchKernelGGL(k_img_tvd_rows, rows, dim3(tvd_lanes(Px)), ldsx, s, z, Py, Px, logPx, twx, A);
    ics_launch_img_wiener_transpose(A, Py, Px, Px, B, s);
    hipLaunchKernelGGL(k_img_tvd_cols, cols, dim3(tvd_lanes(Py)), ldsy, s, B, N0, G, beta, Py, logPy, twy);
    ics_launch_img_wiener_transpose(B, Px, Py, last ? H : Py, A, s);
    if (last)
      hipLaunchKernelGGL(k_img_tvd_inv_rows, dim3(3, (unsigned)H), dim3(tvd_lanes(Px)), ldsx, s, A, Py, Px, logPx, twx, out, 1L, 3L * W, 3, W);
    else
      hipLaunchKernelGGL(k_img_tvd_inv_rows, rows, dim3(tvd_lanes(Px)), ldsx, s, A, Py, Px, logPx, twx, u, (long)Py * Px, (long)Px, 1, Px);
  }
  return hipGetLastError();
}
