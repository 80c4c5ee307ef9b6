// ics_img_align.hip -- registration of two device-resident images and the projective warp of one (ics_img_align, ics_img_align_sums,
// ics_img_warp, include/ics_hip.h): H x W x 3 float32, HWC, contiguous.  The kernels of one Gauss-Newton step of forward-additive
// Lucas-Kanade on the luma; the loop, the damping and the 10 x 10 solve are the host's (ics_images.hip).  Restated in numpy, float64 and
// float32, in tests/align_ref.py.
//
//   luma   Y = ((R + G) + B) * (1 / 3) (px_luma), smoothed by the binomial 1 2 1 each way inside the window (below); level l + 1 = ((a + b) + (c + d)) * 0.25 of a 2 x 2 block, an odd last row or column dropped
//   pixel  of the fixed plane T (H x W) against the moving plane I (Hm x Wm), A the matrix between the planes' own frames (coordinates
//          from the centre, divided by half the longer side):
//            xn = (x - cfx) isf, yn = (y - cfy) isf;  D = (A6 xn + A7 yn) + 1, iD = 1 / D
//            un = ((A0 xn + A1 yn) + A2) iD, vn = ((A3 xn + A4 yn) + A5) iD;  u = un sm + cmx, v = vn sm + cmy
//          counted where 1 <= u < Wm - 2 and 1 <= v < Hm - 2; x0 = floor(u), fx = u - x0, y0, fy likewise
//            bil(p00, p01, p10, p11) = t + fy (s - t), t = p00 + fx (p01 - p00), s = p10 + fx (p11 - p10)
//            val = bil(I around), gx = bil(0.5 (I[y][x + 1] - I[y][x - 1]) around), gy = bil(0.5 (I[y + 1][x] - I[y - 1][x]) around)
//            r = (gain val + bias) - T;  hu = ((gain sm) gx) iD, hv = ((gain sm) gy) iD
//            J = [hu, hv] | [hu xn, hu yn, hu, hv xn, hv yn, hv] | [.., q xn, q yn], q = -(hu un + hv vn); PHOTO: and [val, 1]
//   slot   per tile: the upper triangle of J^T J row-major, J^T r, sum r^2, the count (as a float: at most 1024)
//
// k_img_al_sums<MODEL, PHOTO>: a workgroup of one wave takes a 32 x 32 tile; lane = 32 (y % 2) + x, a lane adds the products of its 16
// pixels top to bottom in registers, writes them to its row of the LDS table (pitch odd: no bank is hit twice), and lane k adds column k
// over the 64 rows in lane order: float32 in one fixed order, no atomics.  The moving plane is read through the caches (a tile's
// footprint under a near-identity warp is a compact block of about 34 x 34 floats).  k_img_al_reduce: one workgroup, the tiles' slots
// added in double -- lane (p, k) walks the tiles p, p + parts, ... of sum k, then lane k adds the parts in order.  k_img_al_warp: a lane
// per output pixel, Keys' cubic convolution (a = -0.5) over 4 x 4 taps clamped to the frame.
#include "ics_img_px.h"

namespace {

#define ALT 32                                 // tile side of the sums kernel
#define ALLANES 64                             // its workgroup: one wave, 16 pixels a lane
#define ALRED 1024                             // lanes of the reduction

__device__ __forceinline__ float al_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float al_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float al_sub(float a, float b) { return __fsub_rn(a, b); }

__host__ __device__ constexpr int al_params(int model, bool photo) { return (model == 0 ? 2 : model == 1 ? 6 : 8) + (photo ? 2 : 0); }
__host__ __device__ constexpr int al_slot(int n) { return n * (n + 1) / 2 + n + 2; }
__host__ __device__ constexpr int al_upper(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }   // (i, j), i <= j, in the row-major upper triangle

struct AlArgs { float A[8]; float isf, cfx, cfy, sm, cmx, cmy, gain, bias, k; };   // k = gain sm
struct AlMat { double m[9]; };

// the luma of pixel (y, x) of the window, both clamped into it
__device__ __forceinline__ float al_luma_at(const float* __restrict__ f, long pitch, int H, int W, int y, int x) {
  float v[3];
  ld3(f + (long)min(max(y, 0), H - 1) * pitch + 3L * min(max(x, 0), W - 1), v);
  return px_luma(v);
}

// the luma plane of a window, smoothed by the binomial 1 2 1 each way (the window repeats its edge): a row is (l + r) + 2 c, the three
// rows are combined the same way, times 1 / 16
__global__ __launch_bounds__(256) void k_img_al_luma(const float* __restrict__ f, long pitch, int H, int W, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  float row[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    row[j] = al_add(al_add(al_luma_at(f, pitch, H, W, y - 1 + j, x - 1), al_luma_at(f, pitch, H, W, y - 1 + j, x + 1)), al_mul(2.f, al_luma_at(f, pitch, H, W, y - 1 + j, x)));
  out[i] = al_mul(al_add(al_add(row[0], row[2]), al_mul(2.f, row[1])), 0.0625f);
}

__global__ __launch_bounds__(256) void k_img_al_half(const float* __restrict__ in, int W, int oh, int ow, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)oh * ow) return;
  const int y = (int)(i / ow), x = (int)(i - (long)y * ow);
  const float* p = in + 2L * y * W + 2L * x;
  out[i] = al_mul(al_add(al_add(p[0], p[1]), al_add(p[W], p[W + 1])), 0.25f);
}

__device__ __forceinline__ float al_bil(float p00, float p01, float p10, float p11, float fx, float fy) {
  const float t = al_add(p00, al_mul(fx, al_sub(p01, p00)));
  const float s = al_add(p10, al_mul(fx, al_sub(p11, p10)));
  return al_add(t, al_mul(fy, al_sub(s, t)));
}

template <int MODEL, bool PHOTO>
__global__ __launch_bounds__(ALLANES) void k_img_al_sums(const float* __restrict__ T, int H, int W, const float* __restrict__ I, int Hm, int Wm, AlArgs a,
                                                         float* __restrict__ slots) {
  constexpr int N = al_params(MODEL, PHOTO), NS = al_slot(N), PITCH = NS | 1;
  __shared__ float red[ALLANES * PITCH];
  const int tx = (W + ALT - 1) / ALT, ty = blockIdx.x / tx, tc = blockIdx.x - ty * tx;
  const int x = tc * ALT + (threadIdx.x & 31), yb = ty * ALT + (threadIdx.x >> 5);
  float acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.f;
  const float xn = al_mul(al_sub((float)x, a.cfx), a.isf);
  const float wlim = (float)(Wm - 2), hlim = (float)(Hm - 2);
  for (int step = 0; step < ALT / 2; ++step) {
    const int y = yb + 2 * step;
    if (y >= H || x >= W) continue;
    const float yn = al_mul(al_sub((float)y, a.cfy), a.isf);
    const float D = al_add(al_add(al_mul(a.A[6], xn), al_mul(a.A[7], yn)), 1.f);
    const float iD = __fdiv_rn(1.f, D);
    const float un = al_mul(al_add(al_add(al_mul(a.A[0], xn), al_mul(a.A[1], yn)), a.A[2]), iD);
    const float vn = al_mul(al_add(al_add(al_mul(a.A[3], xn), al_mul(a.A[4], yn)), a.A[5]), iD);
    const float u = al_add(al_mul(un, a.sm), a.cmx), v = al_add(al_mul(vn, a.sm), a.cmy);
    if (!(u >= 1.f && u < wlim && v >= 1.f && v < hlim)) continue;           // (a NaN position does not count)
    const float fu = floorf(u), fv = floorf(v), fx = al_sub(u, fu), fy = al_sub(v, fv);
    const float* p = I + (long)((int)fv - 1) * Wm + ((int)fu - 1);           // rows y0 - 1 .. y0 + 2, columns x0 - 1 .. x0 + 2, inside the plane
    const float r0b = p[1], r0c = p[2];
    const float r1a = p[Wm], r1b = p[Wm + 1], r1c = p[Wm + 2], r1d = p[Wm + 3];
    const float r2a = p[2 * Wm], r2b = p[2 * Wm + 1], r2c = p[2 * Wm + 2], r2d = p[2 * Wm + 3];
    const float r3b = p[3 * Wm + 1], r3c = p[3 * Wm + 2];
    const float val = al_bil(r1b, r1c, r2b, r2c, fx, fy);
    const float gx = al_bil(al_mul(0.5f, al_sub(r1c, r1a)), al_mul(0.5f, al_sub(r1d, r1b)), al_mul(0.5f, al_sub(r2c, r2a)), al_mul(0.5f, al_sub(r2d, r2b)), fx, fy);
    const float gy = al_bil(al_mul(0.5f, al_sub(r2b, r0b)), al_mul(0.5f, al_sub(r2c, r0c)), al_mul(0.5f, al_sub(r3b, r1b)), al_mul(0.5f, al_sub(r3c, r1c)), fx, fy);
    const float r = al_sub(al_add(al_mul(a.gain, val), a.bias), T[(long)y * W + x]);
    const float hu = al_mul(al_mul(a.k, gx), iD), hv = al_mul(al_mul(a.k, gy), iD);
    float J[N];
    if constexpr (MODEL == 0) {
      J[0] = hu; J[1] = hv;
    } else {
      J[0] = al_mul(hu, xn); J[1] = al_mul(hu, yn); J[2] = hu;
      J[3] = al_mul(hv, xn); J[4] = al_mul(hv, yn); J[5] = hv;
      if constexpr (MODEL == 2) {
        const float q = -al_add(al_mul(hu, un), al_mul(hv, vn));
        J[6] = al_mul(q, xn); J[7] = al_mul(q, yn);
      }
    }
    if constexpr (PHOTO) { J[N - 2] = val; J[N - 1] = 1.f; }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (j >= i) acc[al_upper(N, i, j)] = al_add(acc[al_upper(N, i, j)], al_mul(J[i], J[j]));
#pragma unroll
    for (int i = 0; i < N; ++i) acc[N * (N + 1) / 2 + i] = al_add(acc[N * (N + 1) / 2 + i], al_mul(J[i], r));
    acc[NS - 2] = al_add(acc[NS - 2], al_mul(r, r));
    acc[NS - 1] = al_add(acc[NS - 1], 1.f);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) red[threadIdx.x * PITCH + k] = acc[k];
  __syncthreads();
  for (int k = threadIdx.x; k < NS; k += ALLANES) {
    float s = red[k];
    for (int l = 1; l < ALLANES; ++l) s = al_add(s, red[l * PITCH + k]);
    slots[(long)blockIdx.x * NS + k] = s;
  }
}

// one workgroup: out[k] = the sum over the tiles of slots[tile][k], in double.  Lane (p, k), p < parts = ALRED / ns, adds the tiles
// p, p + parts, ... in that order (eight loads in flight, added in order); lane k then adds the parts in order.
__global__ __launch_bounds__(ALRED) void k_img_al_reduce(const float* __restrict__ slots, int tiles, int ns, double* __restrict__ out) {
  __shared__ double part[ALRED];
  const int parts = ALRED / ns, p = threadIdx.x / ns, k = threadIdx.x - p * ns;
  double s = 0.0;
  if (p < parts) {
    int t = p;
    for (; t + 7 * parts < tiles; t += 8 * parts) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = slots[(long)(t + q * parts) * ns + k];
#pragma unroll
      for (int q = 0; q < 8; ++q) s = __dadd_rn(s, (double)v[q]);
    }
    for (; t < tiles; t += parts) s = __dadd_rn(s, (double)slots[(long)t * ns + k]);
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if ((int)threadIdx.x < ns) {
    double tot = part[threadIdx.x];
    for (int q = 1; q < parts; ++q) tot = __dadd_rn(tot, part[q * ns + threadIdx.x]);
    out[threadIdx.x] = tot;
  }
}

// Keys' cubic convolution, a = -0.5: the weights of the taps at -1, 0, 1, 2 for the fraction t
__device__ __forceinline__ void al_keys(float t, float w[4]) {
  w[0] = al_mul(al_sub(al_mul(al_add(al_mul(-0.5f, t), 1.f), t), 0.5f), t);
  w[1] = al_add(al_mul(al_mul(al_sub(al_mul(1.5f, t), 2.5f), t), t), 1.f);
  w[2] = al_mul(al_add(al_mul(al_add(al_mul(-1.5f, t), 2.f), t), 0.5f), t);
  w[3] = al_mul(al_mul(al_sub(al_mul(0.5f, t), 0.5f), t), t);
}

__global__ __launch_bounds__(256) void k_img_al_warp(const float* __restrict__ src, int H, int W, AlMat M, float* __restrict__ out, int oh, int ow) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)oh * ow) return;
  const int yi = (int)(i / ow), xi = (int)(i - (long)yi * ow);
  // the position in double: a float32 one is 1e-4 px off at x = 2000, which a pixel of an edge shows at the parity gate
  const double x = (double)xi, y = (double)yi;
  const double D = __dadd_rn(__dadd_rn(__dmul_rn(M.m[6], x), __dmul_rn(M.m[7], y)), M.m[8]);
  double u = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(M.m[0], x), __dmul_rn(M.m[1], y)), M.m[2]), D);
  double v = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(M.m[3], x), __dmul_rn(M.m[4], y)), M.m[5]), D);
  u = fmin(u >= -2.0 ? u : -2.0, (double)(W + 1));                           // (a NaN goes to -2; every tap of such a position is an edge pixel)
  v = fmin(v >= -2.0 ? v : -2.0, (double)(H + 1));
  const double fu = floor(u), fv = floor(v);
  float wx[4], wy[4];
  al_keys((float)__dsub_rn(u, fu), wx);
  al_keys((float)__dsub_rn(v, fv), wy);
  const int x0 = (int)fu, y0 = (int)fv;
  int xs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) xs[k] = 3 * min(max(x0 - 1 + k, 0), W - 1);
  float line[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float* row = src + (long)min(max(y0 - 1 + j, 0), H - 1) * (3L * W);
    float p[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) ld3(row + xs[k], p[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      line[j][c] = al_add(al_add(al_add(al_mul(wx[0], p[0][c]), al_mul(wx[1], p[1][c])), al_mul(wx[2], p[2][c])), al_mul(wx[3], p[3][c]));
  }
  float r[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = al_add(al_add(al_add(al_mul(wy[0], line[0][c]), al_mul(wy[1], line[1][c])), al_mul(wy[2], line[2][c])), al_mul(wy[3], line[3][c]));
  st3(out + 3L * i, r);
}

// the frame of a plane: half its longer side and its centre
void al_frame(int H, int W, double* s, double* cx, double* cy) { *s = (H > W ? H : W) / 2.0; *cx = (W - 1) / 2.0; *cy = (H - 1) / 2.0; }

template <int MODEL, bool PHOTO>
void al_launch_sums(const float* T, int H, int W, const float* I, int Hm, int Wm, const AlArgs& a, float* slots, int tiles, hipStream_t s) {
  hipLaunchKernelGGL((k_img_al_sums<MODEL, PHOTO>), dim3((unsigned)tiles), dim3(ALLANES), 0, s, T, H, W, I, Hm, Wm, a, slots);
}

}  // namespace

int ics_img_al_params(int model, int photometric) { return model < 0 || model > 2 ? 0 : al_params(model, photometric != 0); }
int ics_img_al_slot_floats(int model, int photometric) { return model < 0 || model > 2 ? 0 : al_slot(al_params(model, photometric != 0)); }
long ics_img_al_tiles(int H, int W) { return (long)((H + ALT - 1) / ALT) * ((W + ALT - 1) / ALT); }

hipError_t ics_launch_img_al_luma(const float* f, long pitch, int H, int W, float* out, hipStream_t s) {
  if (!f || !out || H < 1 || W < 1 || pitch < 3L * W) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_img_al_luma, dim3((unsigned)(((long)H * W + 255) / 256)), dim3(256), 0, s, f, pitch, H, W, out);
  return hipGetLastError();
}

hipError_t ics_launch_img_al_half(const float* in, int H, int W, float* out, hipStream_t s) {
  const int oh = H / 2, ow = W / 2;
  if (!in || !out || oh < 1 || ow < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_img_al_half, dim3((unsigned)(((long)oh * ow + 255) / 256)), dim3(256), 0, s, in, W, oh, ow, out);
  return hipGetLastError();
}

hipError_t ics_launch_img_al_sums(const float* T, int H, int W, const float* I, int Hm, int Wm, int model, int photometric, const double A[9], double gain, double bias,
                                  float* slots, double* out, hipStream_t s) {
  if (!T || !I || !A || !slots || !out || H < 1 || W < 1 || Hm < 1 || Wm < 1 || model < 0 || model > 2) return hipErrorInvalidValue;
  const long tiles = ics_img_al_tiles(H, W);
  if (tiles > 0x7fffffffL / 128) return hipErrorInvalidValue;
  double sf, cfx, cfy, sm, cmx, cmy;
  al_frame(H, W, &sf, &cfx, &cfy);
  al_frame(Hm, Wm, &sm, &cmx, &cmy);
  AlArgs a;
  for (int k = 0; k < 8; ++k) a.A[k] = (float)(A[k] / A[8]);
  a.isf = (float)(1.0 / sf); a.cfx = (float)cfx; a.cfy = (float)cfy;
  a.sm = (float)sm; a.cmx = (float)cmx; a.cmy = (float)cmy;
  a.gain = (float)gain; a.bias = (float)bias; a.k = a.gain * a.sm;
  const bool photo = photometric != 0;
  switch (model * 2 + (photo ? 1 : 0)) {
    case 0: al_launch_sums<0, false>(T, H, W, I, Hm, Wm, a, slots, (int)tiles, s); break;
    case 1: al_launch_sums<0, true>(T, H, W, I, Hm, Wm, a, slots, (int)tiles, s); break;
    case 2: al_launch_sums<1, false>(T, H, W, I, Hm, Wm, a, slots, (int)tiles, s); break;
    case 3: al_launch_sums<1, true>(T, H, W, I, Hm, Wm, a, slots, (int)tiles, s); break;
    case 4: al_launch_sums<2, false>(T, H, W, I, Hm, Wm, a, slots, (int)tiles, s); break;
    default: al_launch_sums<2, true>(T, H, W, I, Hm, Wm, a, slots, (int)tiles, s); break;
  }
  hipLaunchKernelGGL(k_img_al_reduce, dim3(1), dim3(ALRED), 0, s, slots, (int)tiles, ics_img_al_slot_floats(model, photometric), out);
  return hipGetLastError();
}

hipError_t ics_launch_img_al_warp(const float* src, int H, int W, const double M[9], float* out, int oh, int ow, hipStream_t s) {
  if (!src || !M || !out || H < 1 || W < 1 || oh < 1 || ow < 1) return hipErrorInvalidValue;
  AlMat m;
  for (int k = 0; k < 9; ++k) m.m[k] = M[k] / M[8];
  hipLaunchKernelGGL(k_img_al_warp, dim3((unsigned)(((long)oh * ow + 255) / 256)), dim3(256), 0, s, src, H, W, m, out, oh, ow);
  return hipGetLastError();
}
