// ics_img_wiener.hip -- Wiener deconvolution of a device-resident image by a known PSF (ics_img_wiener, include/ics_hip.h): H x W x 3
// float32, HWC, contiguous; the PSF K x K per channel, every channel of sum 1.  One 2-D transform of the whole frame, fp32, no atomics,
// every sum in one fixed order: two runs give identical bits.  Restated in float64 in tests/wiener_ref.py.
//
//   Py, Px   = the smallest powers of two >= H + K - 1, W + K - 1 (ics_img_wiener_sizes), at most WN_MAX
//   ext      : the frame extended to Py x Px so that the wrap-around carries no step: along y, for every column, rows H .. Py - 1 are
//              (1 - t / g) f[H - 1] + (t / g) f[0], g = Py - H + 1, t = 1 .. g - 1; then the same along x on all Py rows
//   Hc       = the transform of channel c of the PSF, zero padded, its centre tap rolled to (0, 0)
//   L(ky,kx) = 4 sin^2(pi ky / Py) + 4 sin^2(pi kx / Px)  (= 4 - 2 cos(2 pi ky / Py) - 2 cos(2 pi kx / Px), the Laplacian's transfer)
//   G        = conj(Hc) / (|Hc|^2 + balance L^2);  out_c = real(inverse transform(G * transform(ext_c)))[:H, :W], nothing clipped
//
// The line transform (wn_fft, ics_wn_fft.h): a Stockham autosort transform of one line of N = 2^n points in LDS, radix 4 with one leading radix-2
// stage where n is odd, N / 4 butterflies a stage over the workgroup's lanes, the line ping-ponging between two buffers of N float2.
// Stage reads are four runs of consecutive float2 (conflict free), its writes go out at a stride of p float2.  A lane takes two
// butterflies of a stage at a time, all their loads before the arithmetic.  Twiddles come from one table per axis, laid out by stage:
// the stage of sub-transform length p reads {w, w^2, w^3}, w = exp(-2 pi i k / 4p), of its k = 0 .. p - 1 as 3 p consecutive float2 at
// offset p - p0 (p0 = 1, or 2 behind the radix-2 stage), N - p0 float2 in all -- a wave's 64 lanes read 1.5 KB in a row.  (One table
// exp(-2 pi i m / N) read at a stride of N / 4p was the first form: in the middle stages every lane of a load hit a cache line of its
// own, and the three loads were what a stage took: the whole filter at 4096^2, K = 15 took 9.30 ms, 1.8 ms of it per pass over the
// 3 x 8192 lines of 8192 points, against 6.63 ms now.)
//
// Seven kernels, two frames A, B of 3 Py Px float2 each (a spectrum is never read along a column: lines of 8192 points leave room
// for one column per workgroup, and 8-byte reads a row apart are what ics_stats.hip measured as its slowest pass):
//   k_img_wn_tables    : the two twiddle tables and 4 sin^2 along y and x, in double, rounded once
//   k_img_wn_rows      : a workgroup forms row y of channel c of ext (pixel rows from the image, extension rows from its first and last
//                        row), transforms it and writes A[c][y][:]; all Py rows
//   k_img_wn_transpose : A[c][y][kx] -> B[c][kx][y] in 32 x 32 tiles through LDS, 256-byte segments on both sides
//   k_img_wn_psf_rows  : the K non-zero rows of the rolled PSF -> Hr[c][r][:]
//   k_img_wn_psf_cols  : column kx of Hc from the K values Hr[c][:][kx] at their rolled places, transformed; G / (Py Px) -> A[c][kx][:]
//                        (A is free between the two transposes)
//   k_img_wn_cols      : the line B[c][kx][:] forward, times G, inverse, the line staying in LDS in between; written back in place
//   k_img_wn_transpose : B[c][kx][y < H] -> A[c][y][kx]
//   k_img_wn_inv_rows  : rows y < H inverse, the real part of the first W points -> out
// The tables, the transpose, the PSF rows and the inverse rows serve the other units on this transform too (ics_launch_img_wiener_*).
#include "ics_wn_fft.h"

namespace {

#define WN_TILE 32                             // the transposes' tile side

__global__ __launch_bounds__(256) void k_img_wn_tables(float2* __restrict__ twy, float2* __restrict__ twx, float* __restrict__ lamy, float* __restrict__ lamx, int Py, int Px,
                                                       int logPy, int logPx) {
  const int P0 = Py > Px ? Py : Px;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P0; i += gridDim.x * 256) {
    if (i < Py - ((logPy & 1) ? 2 : 1)) twy[i] = wn_table(i, logPy);
    if (i < Px - ((logPx & 1) ? 2 : 1)) twx[i] = wn_table(i, logPx);
    if (i < Py) { const double s = sinpi((double)i / (double)Py); lamy[i] = (float)(4.0 * s * s); }
    if (i < Px) { const double s = sinpi((double)i / (double)Px); lamx[i] = (float)(4.0 * s * s); }
  }
}

// grid (3, Py), the three channels of a row side by side: row blockIdx.y of channel blockIdx.x of the extended frame -> A[c][y][:]
__global__ __launch_bounds__(WN_LANES) void k_img_wn_rows(const float* __restrict__ f, int H, int W, int Py, int Px, int logPx, const float2* __restrict__ tw,
                                                          float2* __restrict__ A) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int c = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  for (int j = tid; j < Px; j += nthr) sm[j] = make_float2(wn_ext<false>(f, c, y, j, H, W, Py, Px), 0.f);
  __syncthreads();
  wn_store(A + ((long)c * Py + y) * Px, wn_fft<false>(sm, sm + Px, Px, logPx, tw), Px);
}

// grid (ceil(clim / 32), ceil(R / 32), 3): in[plane][R][C] -> out[plane][C][R] for the columns below clim
__global__ __launch_bounds__(256) void k_img_wn_transpose(const float2* __restrict__ in, int R, int C, int clim, float2* __restrict__ out) {
  __shared__ float2 tile[WN_TILE][WN_TILE + 1];
  const int c0 = blockIdx.x * WN_TILE, r0 = blockIdx.y * WN_TILE, tx = threadIdx.x & (WN_TILE - 1), ty = threadIdx.x / WN_TILE;
  const long plane = (long)blockIdx.z * R * C;
#pragma unroll
  for (int k = 0; k < WN_TILE; k += 256 / WN_TILE) {
    const int r = r0 + ty + k, c = c0 + tx;
    if (r < R && c < clim) tile[ty + k][tx] = in[plane + (long)r * C + c];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < WN_TILE; k += 256 / WN_TILE) {
    const int c = c0 + ty + k, r = r0 + tx;
    if (c < clim && r < R) out[plane + (long)c * R + r] = tile[tx][ty + k];
  }
}

// grid (K, 3): row r of channel c of the PSF (planar, [3][K][K]), zero padded to Px points, tap K / 2 at point 0 -> Hr[c][r][:]
__global__ __launch_bounds__(WN_LANES) void k_img_wn_psf_rows(const float* __restrict__ psf, int K, int Px, int logPx, const float2* __restrict__ tw,
                                                              float2* __restrict__ Hr) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const long row = (long)blockIdx.y * K + blockIdx.x;
  const float* p = psf + row * K;
  wn_store(Hr + row * Px, wn_psf_line(sm, Px, logPx, K, tw, [&](int t) { return make_float2(p[t], 0.f); }), Px);
}

// grid (Px, 3): column kx of Hc, then G scaled by `scale` = 1 / (Py Px) (a power of two: exact) -> G[c][kx][:]
__global__ __launch_bounds__(WN_LANES) void k_img_wn_psf_cols(const float2* __restrict__ Hr, int K, int Py, int Px, int logPy, const float2* __restrict__ tw,
                                                              const float* __restrict__ lamy, const float* __restrict__ lamx, float balance, float scale,
                                                              float2* __restrict__ G) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int kx = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const float2* h = Hr + (long)c * K * Px + kx;
  const float2* q = wn_psf_line(sm, Py, logPy, K, tw, [&](int t) { return h[(long)t * Px]; });
  const float lx = lamx[kx];
  float2* o = G + ((long)c * Px + kx) * Py;
  for (int j = tid; j < Py; j += nthr) {
    const float2 v = q[j];
    const float lam = lamy[j] + lx;
    const float den = (v.x * v.x + v.y * v.y) + balance * (lam * lam);
    o[j] = make_float2(__fdiv_rn(v.x, den) * scale, __fdiv_rn(-v.y, den) * scale);
  }
}

// grid (Px, 3): the line B[c][kx][:] -> inverse(G * forward(line)), in place
__global__ __launch_bounds__(WN_LANES) void k_img_wn_cols(float2* __restrict__ B, const float2* __restrict__ G, int Py, int logPy, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  float2* l = B + line;
  const float2* g = G + line;
  wn_load(sm, l, Py);
  float2* r = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) r[j] = wn_mul(r[j], g[j]);
  __syncthreads();
  wn_store(l, wn_fft<true>(r, r == sm ? sm + Py : sm, Py, logPy, tw), Py);
}

// grid (3, rows): A[c][y][:] inverse, the real part of the first n points -> dst[c * chan + y * pitch + j * step] (an HWC image: chan 1,
// pitch 3 W, step 3, n W on the rows below H; planes [3][Py][Px]: chan Py Px, pitch Px, step 1, n Px on all Py rows)
__global__ __launch_bounds__(WN_LANES) void k_img_wn_inv_rows(const float2* __restrict__ A, int Py, int Px, int logPx, const float2* __restrict__ tw, float* __restrict__ dst,
                                                              long chan, long pitch, int step, int n) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int c = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  wn_load(sm, A + ((long)c * Py + y) * Px, Px);
  const float2* q = wn_fft<true>(sm, sm + Px, Px, logPx, tw);
  float* o = dst + c * chan + y * pitch;
  for (int j = tid; j < n; j += nthr) o[(long)j * step] = q[j].x;
}

}  // namespace

// transform sizes of an H x W frame and a K x K PSF; 0: a side would be above ICS_IMG_WIENER_MAX
int ics_img_wiener_sizes(int H, int W, int K, int* Py, int* Px) {
  if ((long)H + K - 1 > WN_MAX || (long)W + K - 1 > WN_MAX) return 0;
  *Py = 1 << wn_log2(H + K - 1); *Px = 1 << wn_log2(W + K - 1);
  return 1;
}
size_t ics_img_wiener_frame_bytes(int Py, int Px) { return (size_t)3 * Py * Px * sizeof(float2); }
size_t ics_img_wiener_lds(int P) { return (size_t)2 * P * sizeof(float2); }

// the passes the other units on this transform share with this one: the tables of the two axes; in[plane][R][C] -> out[plane][C][R] for
// the columns below clim on three planes; the rows of the PSF; the inverse rows
void ics_launch_img_wiener_tables(float2* twy, float2* twx, float* lamy, float* lamx, int Py, int Px, hipStream_t s) {
  const int P0 = Py > Px ? Py : Px;
  hipLaunchKernelGGL(k_img_wn_tables, dim3((unsigned)((P0 + 255) / 256)), dim3(256), 0, s, twy, twx, lamy, lamx, Py, Px, wn_log2(Py), wn_log2(Px));
}
void ics_launch_img_wiener_transpose(const float2* in, int R, int C, int clim, float2* out, hipStream_t s) {
  hipLaunchKernelGGL(k_img_wn_transpose, dim3((unsigned)((clim + WN_TILE - 1) / WN_TILE), (unsigned)((R + WN_TILE - 1) / WN_TILE), 3), dim3(256), 0, s, in, R, C, clim, out);
}
hipError_t ics_launch_img_wiener_psf_rows(const float* psf, int K, int Px, const float2* twx, float2* Hr, hipStream_t s) {
  if (hipError_t e = wn_raise_lds<k_img_wn_psf_rows>(Px, Px); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_wn_psf_rows, dim3((unsigned)K, 3), dim3(wn_lanes(Px)), ics_img_wiener_lds(Px), s, psf, K, Px, wn_log2(Px), twx, Hr);
  return hipSuccess;
}
hipError_t ics_launch_img_wiener_inv_rows(const float2* A, int rows, int Py, int Px, const float2* twx, float* dst, long chan, long pitch, int step, int n, hipStream_t s) {
  if (hipError_t e = wn_raise_lds<k_img_wn_inv_rows>(Px, Px); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_wn_inv_rows, dim3(3, (unsigned)rows), dim3(wn_lanes(Px)), ics_img_wiener_lds(Px), s, A, Py, Px, wn_log2(Px), twx, dst, chan, pitch, step, n);
  return hipSuccess;
}

hipError_t ics_launch_img_wiener(const float* f, int H, int W, int K, float balance, int Py, int Px, float2* A, float2* B, void* tables, float* out, hipStream_t s) {
  if (!f || !A || !B || !tables || !out || !wn_shape_ok(H, W, K, Py, Px)) return hipErrorInvalidValue;
  const int logPy = wn_log2(Py), logPx = wn_log2(Px);
  const IcsWnTables t(tables, K, Py, Px);        // (t.psf: uploaded by the caller)
  const size_t ldsy = ics_img_wiener_lds(Py), ldsx = ics_img_wiener_lds(Px);
  hipError_t e = wn_raise_lds<k_img_wn_rows, k_img_wn_psf_cols, k_img_wn_cols>(Py, Px);
  if (e != hipSuccess) return e;
  const float scale = 1.f / ((float)Py * (float)Px);
  ics_launch_img_wiener_tables(t.twy, t.twx, t.lamy, t.lamx, Py, Px, s);
  hipLaunchKernelGGL(k_img_wn_rows, dim3(3, (unsigned)Py), dim3(wn_lanes(Px)), ldsx, s, f, H, W, Py, Px, logPx, t.twx, A);
  ics_launch_img_wiener_transpose(A, Py, Px, Px, B, s);
  if ((e = ics_launch_img_wiener_psf_rows(t.psf, K, Px, t.twx, t.Hr, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_wn_psf_cols, dim3((unsigned)Px, 3), dim3(wn_lanes(Py)), ldsy, s, t.Hr, K, Py, Px, logPy, t.twy, t.lamy, t.lamx, balance, scale, A);
  hipLaunchKernelGGL(k_img_wn_cols, dim3((unsigned)Px, 3), dim3(wn_lanes(Py)), ldsy, s, B, A, Py, logPy, t.twy);
  ics_launch_img_wiener_transpose(B, Px, Py, H, A, s);
  if ((e = ics_launch_img_wiener_inv_rows(A, H, Py, Px, t.twx, out, 1L, 3L * W, 3, W, s)) != hipSuccess) return e;
  return hipGetLastError();
}
