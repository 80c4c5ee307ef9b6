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
// The tables, the tiled transpose, the rows of the PSF and the inverse rows are the Wiener unit's (ics_launch_img_wiener_*); the shrink
// pass is this unit's and serves ics_img_tvmdeconv.hip too (ics_launch_img_tvd_shrink).
// Setup: the tables, k_img_tvd_extend (ext -> u, 0 -> b), k_img_tvd_rows (u -> A), a transpose (A -> N0), the rows of the PSF,
// k_img_tvd_psf_cols (mu conj(Hc) -> A, Gc / (Py Px) -> G), k_img_tvd_n0 (the line of N0 forward, times A, in place).
// An iteration: k_img_tvd_shrink (u, b -> b', z), k_img_tvd_rows (z -> A), a transpose (A -> B), k_img_tvd_cols (the line of B forward,
// (N0 + beta Z) G, inverse, in place), a transpose (B -> A, all Py rows: the domain is periodic; the last iteration the rows below H
// only), the inverse rows (A -> u, all Px points; the last iteration the first W points of the rows below H -> out).
#include "ics_wn_fft.h"

namespace {

#define TVD_TW 64                              // the shrink pass: pixels of a tile along x
#define TVD_TH 16                              //                  and along y; 256 lanes, four pixels each

// grid (3, Py): row y of channel c of the extended frame -> u[c][y][:], zeros -> bx[c][y][:], by[c][y][:]
__global__ __launch_bounds__(256) void k_img_tvd_extend(const float* __restrict__ f, int H, int W, int Py, int Px, float* __restrict__ u, float* __restrict__ bx,
                                                        float* __restrict__ by) {
  const int c = blockIdx.x, y = blockIdx.y;
  const long row = ((long)c * Py + y) * Px;
  for (int j = threadIdx.x; j < Px; j += 256) {
    u[row + j] = wn_ext<false>(f, c, y, j, H, W, Py, Px);
    bx[row + j] = 0.f;
    by[row + j] = 0.f;
  }
}

// grid (3, Py): the real row p[c][y][:] -> its transform A[c][y][:]
__global__ __launch_bounds__(WN_LANES) void k_img_tvd_rows(const float* __restrict__ p, int Py, int Px, int logPx, const float2* __restrict__ tw, float2* __restrict__ A) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const long row = ((long)blockIdx.x * Py + blockIdx.y) * Px;
  wn_load(sm, p + row, Px);
  wn_store(A + row, wn_fft<false>(sm, sm + Px, Px, logPx, tw), Px);
}

// grid (Px, 3): column kx of Hc; mu conj(Hc) -> Hm[c][kx][:], scale / (mu |Hc|^2 + beta L) -> G[c][kx][:] (scale = 1 / (Py Px), a power
// of two: exact.  The denominator is mu at (0, 0), where L is 0 and Hc the channel's sum, and positive everywhere)
__global__ __launch_bounds__(WN_LANES) void k_img_tvd_psf_cols(const float2* __restrict__ Hr, int K, int Py, int Px, int logPy, const float2* __restrict__ tw,
                                                                const float* __restrict__ lamy, const float* __restrict__ lamx, float mu, float beta, float scale,
                                                                float2* __restrict__ Hm, float* __restrict__ G) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int kx = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const float2* h = Hr + (long)c * K * Px + kx;
  const float2* q = wn_psf_line(sm, Py, logPy, K, tw, [&](int t) { return h[(long)t * Px]; });
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
__global__ __launch_bounds__(WN_LANES) void k_img_tvd_n0(float2* __restrict__ N0, const float2* __restrict__ Hm, int Py, int logPy, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  wn_load(sm, N0 + line, Py);
  const float2* r = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) N0[line + j] = wn_mul(Hm[line + j], r[j]);
}

// grid (ceil(Px / TVD_TW), ceil(Py / TVD_TH)): the shrinkage of one tile and its z.  p is formed on the tile and on the one-pixel rim
// above and left of it (z takes the p of the left and of the upper neighbour), from u on the tile and one pixel around it; the rim's b
// is only read.  bx0, by0 -> bx1, by1 (other planes: see the head of this file).  The two layouts of u and z are compile-time forms,
// HALVES false: planes [3][Py][Px] (this unit); HALVES true: the halves of a spectrum row of 2 Px floats, z = u + Px (the masked unit).
// There u and z lie in one allocation; they never share an element, which is what their __restrict__ rests on
template <bool VEC, bool HALVES>
__global__ __launch_bounds__(256) void k_img_tvd_shrink(const float* __restrict__ u, float* __restrict__ z, const float* __restrict__ bx0, const float* __restrict__ by0,
                                                        float* __restrict__ bx1, float* __restrict__ by1, int Py, int Px, float thr) {
  constexpr int UW = TVD_TW + 2, UH = TVD_TH + 2, PW = TVD_TW + 1, PH = TVD_TH + 1;
  __shared__ float su[3][UH][UW];              // u at (y0 - 1 + r, x0 - 1 + q)
  __shared__ float sp[2][3][PH][PW];           // px, py at (y0 - 1 + r, x0 - 1 + q)
  const int x0 = blockIdx.x * TVD_TW, y0 = blockIdx.y * TVD_TH, tid = threadIdx.x;
  const long plane = (long)Py * Px;
  const auto uz = [&](int c, int y, int x) { return HALVES ? ((long)c * Py + y) * 2 * Px + x : c * plane + (long)y * Px + x; };
  for (int i = tid; i < 3 * UH * UW; i += 256) {
    const int c = i / (UH * UW), k = i - c * (UH * UW), r = k / UW, q = k - r * UW;
    su[c][r][q] = u[uz(c, (y0 - 1 + r) & (Py - 1), (x0 - 1 + q) & (Px - 1))];
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
      z[uz(c, y, x)] = __fadd_rn(__fsub_rn(sp[0][c][r][q - 1], sp[0][c][r][q]), __fsub_rn(sp[1][c][r - 1][q], sp[1][c][r][q]));
  }
}

// grid (Px, 3): the line B[c][kx][:] forward, (N0 + beta Z) G, inverse, the line staying in LDS in between; written back in place
__global__ __launch_bounds__(WN_LANES) void k_img_tvd_cols(float2* __restrict__ B, const float2* __restrict__ N0, const float* __restrict__ G, float beta, int Py, int logPy,
                                                            const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  float2* l = B + line;
  wn_load(sm, l, Py);
  float2* r = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) {
    const float2 zz = r[j], n = N0[line + j];
    const float g = G[line + j];
    r[j] = make_float2(__fmul_rn(__fadd_rn(n.x, __fmul_rn(beta, zz.x)), g), __fmul_rn(__fadd_rn(n.y, __fmul_rn(beta, zz.y)), g));
  }
  __syncthreads();
  wn_store(l, wn_fft<true>(r, r == sm ? sm + Py : sm, Py, logPy, tw), Py);
}

}  // namespace

// the one block of a call: A, B, N0 (a spectrum frame each), G (half of one), the two pairs of b planes (half of one each), the tables
size_t ics_img_tvd_workspace_bytes(int K, int Py, int Px) {
  return (size_t)33 * Py * Px * sizeof(float) + IcsWnTables(nullptr, K, Py, Px).bytes;
}
void* ics_img_tvd_tables(void* workspace, int Py, int Px) { return reinterpret_cast<float*>(workspace) + (size_t)33 * Py * Px; }

void ics_launch_img_tvd_shrink(int coupling, bool halves, const float* u, float* z, const float* bx0, const float* by0, float* bx1, float* by1, int Py, int Px, float thr,
                               hipStream_t s) {
  const dim3 grid((unsigned)((Px + TVD_TW - 1) / TVD_TW), (unsigned)((Py + TVD_TH - 1) / TVD_TH));
  const auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, u, z, bx0, by0, bx1, by1, Py, Px, thr); };
  if (halves) { if (coupling) launch(k_img_tvd_shrink<true, true>); else launch(k_img_tvd_shrink<false, true>); }
  else { if (coupling) launch(k_img_tvd_shrink<true, false>); else launch(k_img_tvd_shrink<false, false>); }
}

hipError_t ics_launch_img_tv_deconvolve(const float* f, int H, int W, int K, float mu, float beta, int iterations, int coupling, int Py, int Px, void* workspace, float* out,
                                        hipStream_t s) {
  if (!f || !workspace || !out || !wn_shape_ok(H, W, K, Py, Px) || iterations < 1) return hipErrorInvalidValue;
  const int logPy = wn_log2(Py), logPx = wn_log2(Px);
  const size_t plane3 = (size_t)3 * Py * Px;                  // floats of three real planes; a spectrum frame is two of them
  float* w = reinterpret_cast<float*>(workspace);
  float2 *A = reinterpret_cast<float2*>(w), *B = reinterpret_cast<float2*>(w + 2 * plane3), *N0 = reinterpret_cast<float2*>(w + 4 * plane3);
  float *G = w + 6 * plane3, *u = w + 2 * plane3, *z = w + 3 * plane3;   // (u, z: the halves of B)
  float *bx[2] = {w + 7 * plane3, w + 9 * plane3}, *by[2] = {w + 8 * plane3, w + 10 * plane3};
  const IcsWnTables t(ics_img_tvd_tables(workspace, Py, Px), K, Py, Px);   // (t.psf: uploaded by the caller)
  const size_t ldsy = ics_img_wiener_lds(Py), ldsx = ics_img_wiener_lds(Px);
  hipError_t e = wn_raise_lds<k_img_tvd_rows, k_img_tvd_psf_cols, k_img_tvd_n0, k_img_tvd_cols>(Py, Px);
  if (e != hipSuccess) return e;
  const float scale = 1.f / ((float)Py * (float)Px), thr = 1.f / beta;
  const dim3 rows(3, (unsigned)Py), cols((unsigned)Px, 3);
  const long chan = (long)Py * Px;                            // u and z: planes
  ics_launch_img_wiener_tables(t.twy, t.twx, t.lamy, t.lamx, Py, Px, s);
  hipLaunchKernelGGL(k_img_tvd_extend, rows, dim3(256), 0, s, f, H, W, Py, Px, u, bx[0], by[0]);
  hipLaunchKernelGGL(k_img_tvd_rows, rows, dim3(wn_lanes(Px)), ldsx, s, u, Py, Px, logPx, t.twx, A);
  ics_launch_img_wiener_transpose(A, Py, Px, Px, N0, s);
  if ((e = ics_launch_img_wiener_psf_rows(t.psf, K, Px, t.twx, t.Hr, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_tvd_psf_cols, cols, dim3(wn_lanes(Py)), ldsy, s, t.Hr, K, Py, Px, logPy, t.twy, t.lamy, t.lamx, mu, beta, scale, A, G);
  hipLaunchKernelGGL(k_img_tvd_n0, cols, dim3(wn_lanes(Py)), ldsy, s, N0, A, Py, logPy, t.twy);
  for (int it = 0; it < iterations; ++it) {
    const int from = it & 1, to = from ^ 1;
    const bool last = it == iterations - 1;
    ics_launch_img_tvd_shrink(coupling, false, u, z, bx[from], by[from], bx[to], by[to], Py, Px, thr, s);
    hipLaunchKernelGGL(k_img_tvd_rows, rows, dim3(wn_lanes(Px)), ldsx, s, z, Py, Px, logPx, t.twx, A);
    ics_launch_img_wiener_transpose(A, Py, Px, Px, B, s);
    hipLaunchKernelGGL(k_img_tvd_cols, cols, dim3(wn_lanes(Py)), ldsy, s, B, N0, G, beta, Py, logPy, t.twy);
    ics_launch_img_wiener_transpose(B, Px, Py, last ? H : Py, A, s);
    e = last ? ics_launch_img_wiener_inv_rows(A, H, Py, Px, t.twx, out, 1L, 3L * W, 3, W, s) : ics_launch_img_wiener_inv_rows(A, Py, Py, Px, t.twx, u, chan, Px, 1, Px, s);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}
