// ics_img_psfest.hip -- the PSF that takes a sharp device-resident frame to a blurred one (ics_img_psf_estimate, include/ics_hip.h): two
// H x W x 3 float32 frames (a window of each), HWC; the K x K x 3 raw kernel and the gradient energy of the sharp frame come back.  One
// 2-D transform of the tapered derivatives, fp32, no atomics, every sum in one fixed order: two runs give identical bits.  Restated in
// float64 in tests/psf_est_ref.py.
//
//   Py, Px   = the transform sizes of ics_img_wiener.hip for H, W, K
//   w        = wy (x) wx, wy[y] = 0.5 - 0.5 cos(pi (j + 0.5) / Ty) for j = min(y, H - 1 - y) < Ty = min(K, H / 2), else 1; wx likewise
//   d_x f    = w (f[y][x + 1] - f[y][x]), 0 in the last column; d_y f likewise along y; zero beyond H x W up to Py x Px (no ramp)
//   A, B     = the transforms of a derivative plane of the sharp and of the blurred frame (6 planes: 3 channels x 2 directions)
//   N, D, S  = sum conj(A) B, sum |A|^2, sum over the pixels of (d s)^2 -- over the 2 planes of a channel (coupling 0) or over all 6 (1)
//   raw[i][j]= real(inverse transform(N / (D + regularisation S)))[(i - K / 2) mod Py][(j - K / 2) mod Px]
//
// A plane carries both frames through one complex transform, Z = transform(d s + i d b): A(k) = (Z(k) + conj Z(-k)) / 2 and
// B(k) = (Z(k) - conj Z(-k)) / 2i.  The solve forms P + M and P - M (P = Z(k), M = conj Z(-k)) and leaves the halves out:
// N' = conj(P + M) (-i)(P - M) = 4 N, D' = |P + M|^2 = 4 D, Q = N' / (D' + 4 regularisation S).
//
// The line transform and the twiddle tables are ics_wn_fft.h's, the tiled transpose the Wiener unit's (ics_launch_img_wiener_transpose).
// Six kernels on two frames Za, Zb of 6 Py Px float2 each:
//   k_img_pe_tables : the two twiddle tables and the two tapers wy, wx, in double, rounded once
//   k_img_pe_rows   : a workgroup forms row y of plane p of d s + i d b from the two frames, adds the row's share of S in a fixed lane
//                     order -> slot[p][y], transforms the row -> Za[p][y][:]; rows H .. Py - 1 are written as zeros
//   (transpose)     : Za[p][y][kx] -> Zb[p][kx][y]
//   k_img_pe_cols   : the line Zb[p][kx][:] forward, in place
//   k_img_pe_energy : one workgroup sums the slots in double -> S[3] (coupling 1: the total, three times)
//   k_img_pe_solve  : line kx of Q from the lines kx (as they lie) and -kx (reversed) of the planes, scaled by 1 / (Py Px), inverse along y
//                     while it is in LDS; only the K rows -K/2 .. K/2 (mod Py) leave -> R[q][i][kx]
//   k_img_pe_crop   : row i of R inverse along x, the real part of the K columns around 0 (mod Px) -> raw[i][j][c]
#include "ics_wn_fft.h"

namespace {

#define PE_PLANES 6                            // derivative planes: plane 2 c + d, d = 0 along x, 1 along y

__global__ __launch_bounds__(256) void k_img_pe_tables(float2* __restrict__ twy, float2* __restrict__ twx, float* __restrict__ wy, float* __restrict__ wx, int Py, int Px,
                                                       int logPy, int logPx, int H, int W, int K) {
  const int P0 = Py > Px ? Py : Px, Ty = K < H / 2 ? K : H / 2, Tx = K < W / 2 ? K : W / 2;   // (H, W <= Py, Px)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P0; i += gridDim.x * 256) {
    if (i < Py - ((logPy & 1) ? 2 : 1)) twy[i] = wn_table(i, logPy);
    if (i < Px - ((logPx & 1) ? 2 : 1)) twx[i] = wn_table(i, logPx);
    if (i < H) { const int j = i < H - 1 - i ? i : H - 1 - i; wy[i] = j < Ty ? (float)(0.5 - 0.5 * cospi(((double)j + 0.5) / (double)Ty)) : 1.f; }
    if (i < W) { const int j = i < W - 1 - i ? i : W - 1 - i; wx[i] = j < Tx ? (float)(0.5 - 0.5 * cospi(((double)j + 0.5) / (double)Tx)) : 1.f; }
  }
}

// grid (6, Py): row blockIdx.y of plane blockIdx.x.  s, b: the first pixel of the window in the two frames, `pitch` floats a frame row
// (k_img_ed_rows of ics_img_edges.hip is this kernel with the sharp derivative under a mask: a change here belongs there too; an all-ones
//  mask must keep giving this kernel's bits, tests/test_gpu_blind_psf.py)
__global__ __launch_bounds__(WN_LANES) void k_img_pe_rows(const float* __restrict__ s, const float* __restrict__ b, long pitch, int H, int W, int Py, int Px, int logPx,
                                                          const float2* __restrict__ tw, const float* __restrict__ wy, const float* __restrict__ wx,
                                                          float2* __restrict__ Z, float* __restrict__ slot) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  __shared__ float red[WN_LANES];
  const int p = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x, c = p >> 1, d = p & 1;
  float2* o = Z + ((long)p * Py + y) * Px;
  if (y >= H) {                                  // (the whole workgroup)
    for (int j = tid; j < Px; j += nthr) o[j] = make_float2(0.f, 0.f);
    return;
  }
  const long off = (long)y * pitch + c, step = d ? pitch : 3;
  const int xlim = d ? (y < H - 1 ? W : 0) : W - 1;   // the columns that have their neighbour inside the window
  const float wrow = wy[y];
  float acc = 0.f;
  for (int j = tid; j < Px; j += nthr) {
    float2 v = make_float2(0.f, 0.f);
    if (j < xlim) {
      const long at = off + 3L * j;
      const float w = wrow * wx[j];
      v = make_float2(w * (s[at + step] - s[at]), w * (b[at + step] - b[at]));
      acc += v.x * v.x;
    }
    sm[j] = v;
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = nthr >> 1; h > 0; h >>= 1) {      // (nthr is a power of two)
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) slot[(long)p * H + y] = red[0];
  wn_store(o, wn_fft<false>(sm, sm + Px, Px, logPx, tw), Px);
}

// grid (Px, 6): the line Z[p][kx][:] forward, in place
__global__ __launch_bounds__(WN_LANES) void k_img_pe_cols(float2* __restrict__ Z, int Py, int logPy, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  float2* l = Z + ((long)blockIdx.y * gridDim.x + blockIdx.x) * Py;
  wn_load(sm, l, Py);
  wn_store(l, wn_fft<false>(sm, sm + Py, Py, logPy, tw), Py);
}

// one workgroup: S of channel c = the slots of planes 2 c and 2 c + 1 (2 H floats in a row), summed in double in one fixed order
__global__ __launch_bounds__(256) void k_img_pe_energy(const float* __restrict__ slot, int H, int coupling, double* __restrict__ S) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double e[3];
  for (int c = 0; c < 3; ++c) {
    double acc = 0.0;
    for (int i = tid; i < 2 * H; i += 256) acc += (double)slot[(long)2 * c * H + i];
    red[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    e[c] = red[0];
    __syncthreads();
  }
  if (tid == 0) {
    const double t = (e[0] + e[1]) + e[2];
    for (int c = 0; c < 3; ++c) S[c] = coupling ? t : e[c];
  }
}

// grid (Px, nq), nq = 3 (coupling 0: plane pair q) or 1 (coupling 1: all six): line kx of Q, inverse along y, the K rows around 0 -> R[q][i][kx]
__global__ __launch_bounds__(WN_LANES) void k_img_pe_solve(const float2* __restrict__ Z, int Py, int Px, int logPy, const float2* __restrict__ tw, int K, int coupling,
                                                           float regularisation, float scale, const double* __restrict__ S, float2* __restrict__ R) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int kx = blockIdx.x, q = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const int mx = (Px - kx) & (Px - 1), p0 = coupling ? 0 : 2 * q, np = coupling ? PE_PLANES : 2;
  const float rs = 4.f * (regularisation * (float)S[q]);
  for (int j = tid; j < Py; j += nthr) {
    const int mj = (Py - j) & (Py - 1);
    float nr = 0.f, ni = 0.f, den = 0.f;
    for (int p = p0; p < p0 + np; ++p) {
      const float2 P = Z[((long)p * Px + kx) * Py + j], Mc = Z[((long)p * Px + mx) * Py + mj];   // M = conj(Mc)
      const float ax = P.x + Mc.x, ay = P.y - Mc.y;          // P + M = 2 A
      const float bx = P.y + Mc.y, by = Mc.x - P.x;          // -i (P - M) = 2 B
      nr += ax * bx + ay * by;                               // conj(2 A) (2 B)
      ni += ax * by - ay * bx;
      den += ax * ax + ay * ay;
    }
    den += rs;
    sm[j] = make_float2(__fdiv_rn(nr, den) * scale, __fdiv_rn(ni, den) * scale);
  }
  __syncthreads();
  const float2* r = wn_fft<true>(sm, sm + Py, Py, logPy, tw);
  for (int i = tid; i < K; i += nthr) R[((long)q * K + i) * Px + kx] = r[(i - K / 2 + Py) & (Py - 1)];
}

// grid (K, nq): row i of R[q] inverse along x, the real part of the K columns around 0 -> raw[i][j][q] (coupling 1: the three channels)
__global__ __launch_bounds__(WN_LANES) void k_img_pe_crop(const float2* __restrict__ R, int Px, int logPx, const float2* __restrict__ tw, int K, int coupling,
                                                          float* __restrict__ raw) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  const int i = blockIdx.x, q = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  wn_load(sm, R + ((long)q * K + i) * Px, Px);
  const float2* r = wn_fft<true>(sm, sm + Px, Px, logPx, tw);
  for (int j = tid; j < K; j += nthr) {
    const float v = r[(j - K / 2 + Px) & (Px - 1)].x;
    float* o = raw + ((long)i * K + j) * 3;
    if (coupling) { o[0] = v; o[1] = v; o[2] = v; }
    else o[q] = v;
  }
}

// the workspace: Za, Zb (6 Py Px float2 each), R (3 K Px float2), the twiddles (Py + Px float2), S (4 doubles, one unused), then floats:
// wy (H), wx (W), the slots (6 H), raw (3 K K)
struct PeCarve {
  float2 *Za = nullptr, *Zb = nullptr, *R = nullptr, *twy = nullptr, *twx = nullptr;
  double* S = nullptr;
  float *wy = nullptr, *wx = nullptr, *slot = nullptr, *raw = nullptr;
  size_t bytes;
  PeCarve(void* ws, int H, int W, int K, int Py, int Px) {
    const size_t frame = (size_t)PE_PLANES * Py * Px * sizeof(float2);
    const size_t oR = 2 * frame, otw = oR + (size_t)3 * K * Px * sizeof(float2), oS = otw + ((size_t)Py + Px) * sizeof(float2), of = oS + 4 * sizeof(double);
    bytes = of + ((size_t)H + W + (size_t)PE_PLANES * H + (size_t)3 * K * K) * sizeof(float);
    if (!ws) return;                             // (the size alone)
    char* at = reinterpret_cast<char*>(ws);
    const auto f2 = [&](size_t o) { return reinterpret_cast<float2*>(at + o); };
    Za = f2(0); Zb = f2(frame); R = f2(oR); twy = f2(otw); twx = f2(otw + (size_t)Py * sizeof(float2));
    S = reinterpret_cast<double*>(at + oS);
    wy = reinterpret_cast<float*>(at + of);
    wx = wy + H;
    slot = wx + W;
    raw = slot + (size_t)PE_PLANES * H;
  }
};

}  // namespace

size_t ics_img_pe_workspace_bytes(int H, int W, int K, int Py, int Px) { return PeCarve(nullptr, H, W, K, Py, Px).bytes; }
float* ics_img_pe_raw(void* workspace, int H, int W, int K, int Py, int Px) { return PeCarve(workspace, H, W, K, Py, Px).raw; }
double* ics_img_pe_energy(void* workspace, int H, int W, int K, int Py, int Px) { return PeCarve(workspace, H, W, K, Py, Px).S; }

// tables -> the rows of the six planes -> transposes, columns, energy, solve, crop, on the carved workspace.  rows == nullptr: k_img_pe_rows
// on the two frames; else the caller's row kernel (ics_img_edges.hip: the sharp frame's derivatives under a mask), launched by `rows`
// with what k_img_pe_rows gets -- it has to write every row of Za and every slot
hipError_t ics_launch_img_psf_estimate_rows(ics_pe_rows_fn rows, void* user, const float* sharp, const float* blurred, long pitch, int H, int W, int K,
                                            float regularisation, int coupling, int Py, int Px, void* workspace, hipStream_t s) {
  if (!sharp || !blurred || !workspace || !wn_shape_ok(H, W, K, Py, Px) || pitch < 3L * W) return hipErrorInvalidValue;
  if (!(regularisation > 0.f) || (coupling != 0 && coupling != 1)) return hipErrorInvalidValue;
  const int logPy = wn_log2(Py), logPx = wn_log2(Px), nq = coupling ? 1 : 3;
  const PeCarve m(workspace, H, W, K, Py, Px);
  const size_t ldsy = ics_img_wiener_lds(Py), ldsx = ics_img_wiener_lds(Px);
  if (hipError_t e = wn_raise_lds<k_img_pe_rows, k_img_pe_cols, k_img_pe_solve, k_img_pe_crop>(Py, Px); e != hipSuccess) return e;
  const int P0 = Py > Px ? Py : Px;
  const size_t half = (size_t)3 * Py * Px;       // the transpose takes three planes a launch
  const float scale = 1.f / ((float)Py * (float)Px);
  hipLaunchKernelGGL(k_img_pe_tables, dim3((unsigned)((P0 + 255) / 256)), dim3(256), 0, s, m.twy, m.twx, m.wy, m.wx, Py, Px, logPy, logPx, H, W, K);
  if (rows) {
    const IcsPeRows r = {sharp, blurred, pitch, H, W, Py, Px, logPx, m.twx, m.wy, m.wx, m.Za, m.slot, wn_lanes(Px), ldsx};
    if (hipError_t e = rows(r, user, s); e != hipSuccess) return e;
  } else
    hipLaunchKernelGGL(k_img_pe_rows, dim3(PE_PLANES, (unsigned)Py), dim3(wn_lanes(Px)), ldsx, s, sharp, blurred, pitch, H, W, Py, Px, logPx, m.twx, m.wy, m.wx, m.Za, m.slot);
  ics_launch_img_wiener_transpose(m.Za, Py, Px, Px, m.Zb, s);
  ics_launch_img_wiener_transpose(m.Za + half, Py, Px, Px, m.Zb + half, s);
  hipLaunchKernelGGL(k_img_pe_cols, dim3((unsigned)Px, PE_PLANES), dim3(wn_lanes(Py)), ldsy, s, m.Zb, Py, logPy, m.twy);
  hipLaunchKernelGGL(k_img_pe_energy, dim3(1), dim3(256), 0, s, m.slot, H, coupling, m.S);
  hipLaunchKernelGGL(k_img_pe_solve, dim3((unsigned)Px, (unsigned)nq), dim3(wn_lanes(Py)), ldsy, s, m.Zb, Py, Px, logPy, m.twy, K, coupling, regularisation, scale, m.S, m.R);
  hipLaunchKernelGGL(k_img_pe_crop, dim3((unsigned)K, (unsigned)nq), dim3(wn_lanes(Px)), ldsx, s, m.R, Px, logPx, m.twx, K, coupling, m.raw);
  return hipGetLastError();
}

hipError_t ics_launch_img_psf_estimate(const float* sharp, const float* blurred, long pitch, int H, int W, int K, float regularisation, int coupling, int Py, int Px,
                                       void* workspace, hipStream_t s) {
  return ics_launch_img_psf_estimate_rows(nullptr, nullptr, sharp, blurred, pitch, H, W, K, regularisation, coupling, Py, Px, workspace, s);
}
