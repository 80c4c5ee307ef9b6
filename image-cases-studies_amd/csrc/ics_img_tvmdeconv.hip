// ics_img_tvmdeconv.hip -- TV deconvolution of a device-resident image by a known PSF with a masked data term
// (ics_img_tv_deconvolve_masked, include/ics_hip.h): minimise sum |Du| + (mu / 2) |M (h * u - f)|^2, M a 0/1 plane that is 0 on the
// extension of the frame to the transform size, on clipped and non-finite pixels and wherever the caller says so.  The mask breaks the
// diagonal solve of ics_img_tvdeconv.hip; one more splitting variable v = h * u (multiplier d, penalty gamma) restores it (Almeida and
// Figueiredo, IEEE TIP 2013).  H x W x 3 float32, HWC; the PSF K x K per channel, every channel of sum 1.  fp32, no atomics, every sum
// in one fixed order: two runs give identical bits.  Restated in float64 in tests/tvm_deconv_ref.py.
//
//   Py, Px, the ramp, Hc, L : as in ics_img_wiener.hip;  f0 = f with non-finite values 0, ext = the ramp extension of f0
//   m = observed and the three channels finite and the three channels < clip;  M = m on the frame, 0 on the extension
//   Gc = 1 / (gamma |Hc|^2 + beta L),  u = ext, bx = by = d = 0, r_c = real(inverse(Hc transform(ext_c)));  n times:
//     u, bx, by -> bx, by, z : the shrink step of ics_img_tvdeconv.hip
//     t = r + d;  v = (mu M ext + gamma t) / (mu M + gamma);  d = t - v;  q = v - d
//     U_c = (gamma conj(Hc) transform(q_c) + beta transform(z_c)) Gc;  u_c + i r_c = inverse(U_c + i Hc U_c)
//   out = u[:H, :W], nothing clipped; and the count of frame pixels with m false
//
// Two real frames per transform, both ways.  Forward, a row carries q in its real and z in its imaginary part; the transform of a real
// row is Hermitian, so the column kernel takes the two row spectra apart again from lines kx and Px - kx:
// Q = (X[kx] + conj(X[-kx])) / 2, Z = (X[kx] - conj(X[-kx])) / 2i.  It transforms both lines (their multipliers differ), forms U, and
// sends U + i Hc U back through one inverse: u and r are real, so they come out as its real and imaginary part.
//
// One workspace: two spectrum frames A, B (3 Py Px float2 each), Hc (one more, [c][kx][ky]), G (3 Py Px float, [c][kx][ky], scaled by
// 1 / (Py Px)), two pairs of b planes, d, ext, r (three real planes each), M (one plane), the row counts, the tables of
// ics_img_wiener.hip and the caller's byte mask.  u and z live inside the spectrum frame that is idle: row y of channel c of a frame
// is 2 Px floats, u[c][y][:] its first Px and z[c][y][:] its second Px, so the row kernels work in place (a workgroup reads its row
// into LDS before it writes it) and the frames swap roles every iteration.  b ping-pongs as in ics_img_tvdeconv.hip.
//
// The tables, the tiled transpose and the rows of the PSF are the Wiener unit's (ics_launch_img_wiener_*), the shrink pass the TV unit's
// (ics_launch_img_tvd_shrink, in its form for the row halves of this unit).
// Setup: the tables, k_img_tvm_setup (ext, M, 0 -> b, d, the row counts), k_img_tvm_count, the rows of the PSF, k_img_tvm_psf_cols
// (Hc, Gc / (Py Px)), k_img_tvm_rows (ext -> A), a transpose, k_img_tvm_blur_cols (forward, Hc / (Py Px), inverse), a transpose,
// k_img_tvm_inv_rows (ext -> u, real part -> r).
// An iteration, u in X: the shrink pass (u, b -> b', z), k_img_tvm_rows (r, d, M, ext, z -> d, X), a transpose (X -> Y),
// k_img_tvm_cols (lines kx, Px - kx of Y -> line kx of X), a transpose (X -> Y; the last iteration the rows below H only),
// k_img_tvm_inv_rows (Y -> u, r in place; the last iteration the first W points of the rows below H -> out).
#include <utility>
#include "ics_img_px.h"
#include "ics_wn_fft.h"

namespace {

#define TVM_PER 8                              // points of a line per lane at most
static_assert(TVM_PER * WN_LANES == WN_MAX, "the column kernel holds a whole line in its lanes");

// grid (Py): row y of the extended frame -> ext[c][y][:] (of f0), M[y][:], zeros ->
// bx, by, d; the unobserved pixels of the row -> rowcount[y] (lane sums, then a tree in LDS: one order)
__global__ __launch_bounds__(256) void k_img_tvm_setup(const float* __restrict__ f, const unsigned char* __restrict__ observed, float clip, int H, int W, int Py, int Px,
                                                       float* __restrict__ ext, float* __restrict__ bx, float* __restrict__ by, float* __restrict__ d, float* __restrict__ M,
                                                       int* __restrict__ rowcount) {
  __shared__ int cnt[256];
  const int y = blockIdx.x, tid = threadIdx.x;
  const long plane = (long)Py * Px;
  int n = 0;
  for (int j = tid; j < Px; j += 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long at = c * plane + (long)y * Px + j;
      ext[at] = wn_ext<true>(f, c, y, j, H, W, Py, Px);
      bx[at] = 0.f;
      by[at] = 0.f;
      d[at] = 0.f;
    }
    bool m = false;
    if (y < H && j < W) {
      float v[3];
      ld3(f + ((long)y * W + j) * 3, v);
      m = isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && v[0] < clip && v[1] < clip && v[2] < clip && (!observed || observed[(long)y * W + j] != 0);
      n += m ? 0 : 1;
    }
    M[(long)y * Px + j] = m ? 1.f : 0.f;
  }
  cnt[tid] = n;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) cnt[tid] += cnt[tid + h];
    __syncthreads();
  }
  if (tid == 0) rowcount[y] = cnt[0];
}

// grid (1): the row counts of the H frame rows -> total[0]
__global__ __launch_bounds__(256) void k_img_tvm_count(const int* __restrict__ rowcount, int H, long long* __restrict__ total) {
  __shared__ long long cnt[256];
  const int tid = threadIdx.x;
  long long n = 0;
  for (int y = tid; y < H; y += 256) n += rowcount[y];
  cnt[tid] = n;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) cnt[tid] += cnt[tid + h];
    __syncthreads();
  }
  if (tid == 0) total[0] = cnt[0];
}

// grid (Px, 3): column kx of Hc -> Hc[c][kx][:], scale / (gamma |Hc|^2 + beta L) -> G[c][kx][:] (scale = 1 / (Py Px), a power of two:
// exact.  The denominator is gamma at (0, 0), where L is 0 and Hc the channel's sum, and positive everywhere)
__global__ __launch_bounds__(WN_LANES) void k_img_tvm_psf_cols(const float2* __restrict__ Hr, int K, int Py, int Px, int logPy, const float2* __restrict__ tw,
                                                                const float* __restrict__ lamy, const float* __restrict__ lamx, float gamma, float beta, float scale,
                                                                float2* __restrict__ Hc, float* __restrict__ G) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int kx = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const float2* h = Hr + (long)c * K * Px + kx;
  const float2* q = wn_psf_line(sm, Py, logPy, K, tw, [&](int t) { return h[(long)t * Px]; });
  const float lx = lamx[kx];
  const long line = ((long)c * Px + kx) * Py;
  for (int j = tid; j < Py; j += nthr) {
    const float2 v = q[j];
    const float den = __fadd_rn(__fmul_rn(gamma, __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y))), __fmul_rn(beta, __fadd_rn(lamy[j], lx)));
    Hc[line + j] = v;
    G[line + j] = __fdiv_rn(scale, den);
  }
}

// grid (3, Py): row y of channel c -> its transform X[c][y][:], in place over the row's u and z.  r == nullptr (the setup): the row of
// ext alone.  Otherwise the v, d, q update of the row (d in place), q in the real and z in the imaginary part
__global__ __launch_bounds__(WN_LANES) void k_img_tvm_rows(float2* X, const float* __restrict__ ext, const float* __restrict__ r, float* __restrict__ d,
                                                            const float* __restrict__ M, float mu, float gamma, int Py, int Px, int logPx, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const long row = ((long)blockIdx.x * Py + y) * Px;
  float2* line = X + row;
  const float* z = reinterpret_cast<const float*>(line) + Px;
  if (!r) {
    for (int j = tid; j < Px; j += nthr) sm[j] = make_float2(ext[row + j], 0.f);
  } else {
    const float* m = M + (long)y * Px;
    for (int j = tid; j < Px; j += nthr) {
      const float t = __fadd_rn(r[row + j], d[row + j]), w = __fmul_rn(mu, m[j]);
      const float v = __fdiv_rn(__fadd_rn(__fmul_rn(w, ext[row + j]), __fmul_rn(gamma, t)), __fadd_rn(w, gamma));
      const float dn = __fsub_rn(t, v);
      d[row + j] = dn;
      sm[j] = make_float2(__fsub_rn(v, dn), z[j]);
    }
  }
  __syncthreads();
  wn_store(line, wn_fft<false>(sm, sm + Px, Px, logPx, tw), Px);
}

// grid (Px, 3), the setup: the line B[c][kx][:] forward, times Hc (scale = 1 / (Py Px)), inverse, in place
__global__ __launch_bounds__(WN_LANES) void k_img_tvm_blur_cols(float2* __restrict__ B, const float2* __restrict__ Hc, float scale, int Py, int logPy,
                                                                 const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  wn_load(sm, B + line, Py);
  float2* r = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  for (int j = tid; j < Py; j += nthr) {
    const float2 v = wn_mul(Hc[line + j], r[j]);
    r[j] = make_float2(__fmul_rn(v.x, scale), __fmul_rn(v.y, scale));
  }
  __syncthreads();
  wn_store(B + line, wn_fft<true>(r, r == sm ? sm + Py : sm, Py, logPy, tw), Py);
}

// grid (Px, 3): lines kx and Px - kx of Y (the transposed row transforms of q + i z) -> the row spectra of q and of z at kx, both
// forward (z waits in registers, then the transform of q does), U = (gamma conj(Hc) Q + beta Z) G, U + i Hc U inverse -> line kx of X.
// A lane holds points tid + i blockDim.x, i < TVM_PER
__global__ __launch_bounds__(WN_LANES) void k_img_tvm_cols(const float2* __restrict__ Y, float2* __restrict__ X, const float2* __restrict__ Hc, const float* __restrict__ G,
                                                            float gamma, float beta, int Py, int logPy, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int kx = blockIdx.x, Px = gridDim.x, tid = threadIdx.x, nthr = blockDim.x;
  const long line = ((long)blockIdx.y * Px + kx) * Py, mirror = ((long)blockIdx.y * Px + ((Px - kx) & (Px - 1))) * Py;
  float2 hold[TVM_PER];
#pragma unroll
  for (int i = 0; i < TVM_PER; ++i) {
    const int j = tid + i * nthr;
    if (j < Py) {
      const float2 a = Y[line + j], b = Y[mirror + j];
      sm[j] = make_float2(__fmul_rn(0.5f, __fadd_rn(a.x, b.x)), __fmul_rn(0.5f, __fsub_rn(a.y, b.y)));
      hold[i] = make_float2(__fmul_rn(0.5f, __fadd_rn(a.y, b.y)), __fmul_rn(0.5f, __fsub_rn(b.x, a.x)));
    }
  }
  __syncthreads();
  const float2* fq = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
  // the transform of q is in fq, which is sm or sm + Py; every lane takes its points of it, then the line of z goes into sm
  float2 qq[TVM_PER];
#pragma unroll
  for (int i = 0; i < TVM_PER; ++i) {
    const int j = tid + i * nthr;
    if (j < Py) qq[i] = fq[j];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TVM_PER; ++i) {
    const int j = tid + i * nthr;
    if (j < Py) sm[j] = hold[i];
  }
  __syncthreads();
  float2* fz = wn_fft<false>(sm, sm + Py, Py, logPy, tw);
#pragma unroll
  for (int i = 0; i < TVM_PER; ++i) {
    const int j = tid + i * nthr;
    if (j < Py) {
      const float2 h = Hc[line + j], zz = fz[j];
      const float g = G[line + j];
      const float2 hq = wn_mul(make_float2(h.x, -h.y), qq[i]);
      const float2 u = make_float2(__fmul_rn(__fadd_rn(__fmul_rn(gamma, hq.x), __fmul_rn(beta, zz.x)), g), __fmul_rn(__fadd_rn(__fmul_rn(gamma, hq.y), __fmul_rn(beta, zz.y)), g));
      const float2 hu = wn_mul(h, u);
      fz[j] = make_float2(__fsub_rn(u.x, hu.y), __fadd_rn(u.y, hu.x));
    }
  }
  __syncthreads();
  const float2* q = wn_fft<true>(fz, fz == sm ? sm + Py : sm, Py, logPy, tw);
#pragma unroll
  for (int i = 0; i < TVM_PER; ++i) {
    const int j = tid + i * nthr;
    if (j < Py) X[line + j] = q[j];
  }
}

// grid (3, rows): Y[c][y][:] inverse; the real part of the first n points -> dst[c * chan + y * pitch + j * step] (u in place: dst the
// frame itself, chan 2 Py Px, pitch 2 Px, step 1, n Px on all Py rows; the result image: chan 1, pitch 3 W, step 3, n W on the rows
// below H).  r given: the imaginary part -> r[c][y][:]; uinit given too (the setup): the row of uinit -> dst, the real part -> r
__global__ __launch_bounds__(WN_LANES) void k_img_tvm_inv_rows(const float2* Y, int Py, int Px, int logPx, const float2* __restrict__ tw, float* dst, long chan, long pitch,
                                                                int step, int n, const float* __restrict__ uinit, float* __restrict__ r) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int c = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const long row = ((long)c * Py + y) * Px;
  wn_load(sm, Y + row, Px);
  const float2* q = wn_fft<true>(sm, sm + Px, Px, logPx, tw);
  float* o = dst + c * chan + y * pitch;
  for (int j = tid; j < n; j += nthr) {
    const float2 v = q[j];
    o[(long)j * step] = uinit ? uinit[row + j] : v.x;
    if (r) r[row + j] = uinit ? v.x : v.y;
  }
}

}  // namespace

// the one block of a call, in floats of a transform plane (Py Px): A, B, Hc (6 each), G, bx0, by0, bx1, by1, d, ext, r (3 each), M (1)
// = 43; then Py row counts and the total (4 words), the tables, and Py Px bytes for the caller's mask (H W of them used)
size_t ics_img_tvm_workspace_bytes(int K, int Py, int Px) {
  return ((size_t)43 * Py * Px + Py + 4) * sizeof(float) + IcsWnTables(nullptr, K, Py, Px).bytes + (size_t)Py * Px;
}
void* ics_img_tvm_tables(void* workspace, int Py, int Px) { return reinterpret_cast<float*>(workspace) + (size_t)43 * Py * Px + Py + 4; }
long long* ics_img_tvm_total(void* workspace, int Py, int Px) { return reinterpret_cast<long long*>(reinterpret_cast<float*>(workspace) + (size_t)43 * Py * Px + Py); }
unsigned char* ics_img_tvm_mask_slot(void* workspace, int K, int Py, int Px) {
  return reinterpret_cast<unsigned char*>(ics_img_tvm_tables(workspace, Py, Px)) + IcsWnTables(nullptr, K, Py, Px).bytes;
}

hipError_t ics_launch_img_tv_deconvolve_masked(const float* f, int H, int W, int K, bool observed, float clip, float mu, float beta, float gamma, int iterations, int coupling,
                                               int Py, int Px, void* workspace, float* out, hipStream_t s) {
  if (!f || !workspace || !out || !wn_shape_ok(H, W, K, Py, Px) || iterations < 1) return hipErrorInvalidValue;
  if (Py > TVM_PER * wn_lanes(Py)) return hipErrorInvalidValue;
  const int logPy = wn_log2(Py), logPx = wn_log2(Px);
  const size_t plane3 = (size_t)3 * Py * Px;                  // floats of three real planes; a spectrum frame is two of them
  float* w = reinterpret_cast<float*>(workspace);
  float2 *X = reinterpret_cast<float2*>(w), *Y = reinterpret_cast<float2*>(w + 2 * plane3), *Hc = reinterpret_cast<float2*>(w + 4 * plane3);
  float* G = w + 6 * plane3;
  float *bx[2] = {w + 7 * plane3, w + 9 * plane3}, *by[2] = {w + 8 * plane3, w + 10 * plane3};
  float *d = w + 11 * plane3, *ext = w + 12 * plane3, *r = w + 13 * plane3, *M = w + 14 * plane3;
  int* rowcount = reinterpret_cast<int*>(M + (size_t)Py * Px);
  const IcsWnTables t(ics_img_tvm_tables(workspace, Py, Px), K, Py, Px);   // (t.psf: uploaded by the caller)
  const unsigned char* mask = observed ? ics_img_tvm_mask_slot(workspace, K, Py, Px) : nullptr;   // (uploaded by the caller too)
  const size_t ldsy = ics_img_wiener_lds(Py), ldsx = ics_img_wiener_lds(Px);
  hipError_t e = wn_raise_lds<k_img_tvm_rows, k_img_tvm_psf_cols, k_img_tvm_blur_cols, k_img_tvm_cols, k_img_tvm_inv_rows>(Py, Px);
  if (e != hipSuccess) return e;
  const float scale = 1.f / ((float)Py * (float)Px), thr = 1.f / beta;
  const dim3 rows(3, (unsigned)Py), cols((unsigned)Px, 3), lx((unsigned)wn_lanes(Px)), ly((unsigned)wn_lanes(Py));
  const long uchan = 2L * Py * Px, upitch = 2L * Px;         // u inside a spectrum frame
  ics_launch_img_wiener_tables(t.twy, t.twx, t.lamy, t.lamx, Py, Px, s);
  hipLaunchKernelGGL(k_img_tvm_setup, dim3((unsigned)Py), dim3(256), 0, s, f, mask, clip, H, W, Py, Px, ext, bx[0], by[0], d, M, rowcount);
  hipLaunchKernelGGL(k_img_tvm_count, dim3(1), dim3(256), 0, s, rowcount, H, ics_img_tvm_total(workspace, Py, Px));
  if ((e = ics_launch_img_wiener_psf_rows(t.psf, K, Px, t.twx, t.Hr, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_img_tvm_psf_cols, cols, ly, ldsy, s, t.Hr, K, Py, Px, logPy, t.twy, t.lamy, t.lamx, gamma, beta, scale, Hc, G);
  hipLaunchKernelGGL(k_img_tvm_rows, rows, lx, ldsx, s, X, ext, (const float*)nullptr, (float*)nullptr, (const float*)nullptr, mu, gamma, Py, Px, logPx, t.twx);
  ics_launch_img_wiener_transpose(X, Py, Px, Px, Y, s);
  hipLaunchKernelGGL(k_img_tvm_blur_cols, cols, ly, ldsy, s, Y, Hc, scale, Py, logPy, t.twy);
  ics_launch_img_wiener_transpose(Y, Px, Py, Py, X, s);
  hipLaunchKernelGGL(k_img_tvm_inv_rows, rows, lx, ldsx, s, X, Py, Px, logPx, t.twx, reinterpret_cast<float*>(X), uchan, upitch, 1, Px, ext, r);
  for (int it = 0; it < iterations; ++it) {
    const int from = it & 1, to = from ^ 1;
    const bool last = it == iterations - 1;
    ics_launch_img_tvd_shrink(coupling, true, reinterpret_cast<float*>(X), reinterpret_cast<float*>(X) + Px, bx[from], by[from], bx[to], by[to], Py, Px, thr, s);
    hipLaunchKernelGGL(k_img_tvm_rows, rows, lx, ldsx, s, X, ext, r, d, M, mu, gamma, Py, Px, logPx, t.twx);
    ics_launch_img_wiener_transpose(X, Py, Px, Px, Y, s);
    hipLaunchKernelGGL(k_img_tvm_cols, cols, ly, ldsy, s, Y, X, Hc, G, gamma, beta, Py, logPy, t.twy);
    ics_launch_img_wiener_transpose(X, Px, Py, last ? H : Py, Y, s);
    if (last)
      hipLaunchKernelGGL(k_img_tvm_inv_rows, dim3(3, (unsigned)H), lx, ldsx, s, Y, Py, Px, logPx, t.twx, out, 1L, 3L * W, 3, W, (const float*)nullptr, (float*)nullptr);
    else
      hipLaunchKernelGGL(k_img_tvm_inv_rows, rows, lx, ldsx, s, Y, Py, Px, logPx, t.twx, reinterpret_cast<float*>(Y), uchan, upitch, 1, Px, (const float*)nullptr, r);
    std::swap(X, Y);                             // u is in the frame the inverse rows ran on
  }
  return hipGetLastError();
}
