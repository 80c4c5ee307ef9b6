// ics_img_wavelet.hip -- wavelet equaliser of device-resident images (ics_img_wavelet_equalize, include/ics_hip.h): H x W x 3 float32,
// HWC, contiguous.  An undecimated B3-spline ("a trous", starlet) decomposition into J <= 8 detail scales; every detail is
// soft-thresholded, multiplied by a gain, and the scales are summed back.
//
//   c_0      = f,  c_{j+1} = V_j(H_j(c_j)):  taps [1 4 6 4 1] / 16 at offsets {-2 .. 2} * 2^j along x, then along y
//   index    outside the picture: folded as numpy.pad(mode="symmetric"), i mod 2n and then 2n - 1 - i if >= n (wv_fold, ics_img_px.h)
//   one pass ((a[-2] + a[+2]) / 16 + (a[-1] + a[+1]) * 4 / 16) + a[0] * 6 / 16   (wv_pass, no FMA)
//   w_j      = c_j - c_{j+1};  s_j = sign(w) max(|w| - t_j, 0) ("channel") or w * (max(m - t_j, 0) / m), m = |w| over the three
//              channels with the squares added smallest first ("vector"), 0 where m = 0
//   out      = residual * c_J + (((g_0 s_0) + g_1 s_1) + ...) from zero   (wv_detail, wv_out)
//
// Every value is computed by these inline functions in one fixed order by both routes, so the routes agree bit for bit.
//
// Route 1 (k_img_wv_scale): one launch per scale, a lane per pixel.  The lane reads the 5 x 5 dilated neighbourhood of c_j directly
// (25 12-byte loads, consecutive lanes on consecutive pixels of five rows: served by L1 / L2; a staged tile would need a halo of
// 2 * 2^j pixels per side, from j = 3 on more than the tile itself, and at j = 7 it fits no LDS), forms the five row sums and from
// them c_{j+1}, writes c_{j+1} to the other of two pooled frames and read-modify-writes the accumulator, which lives in the result
// frame.  The last launch writes residual * c_J + accumulator instead.  Frame transits: 3 for the first scale (no accumulator to
// read), 4 per middle scale, 3 for the last.
//
// Route 2 (k_img_wv_fused): the first F = ICS_IMG_WAVELET_FUSED = 3 scales in one launch on a 48 x 32 output tile in LDS.  Scale j
// needs c_j 2 * 2^j pixels further out, so the staged region is the tile plus 2 * (2^F - 1) = 14 pixels per side, 76 x 60 pixels,
// loaded through wv_fold: a tile position outside the picture holds the symmetric extension of c_0.  The extension of c_{j+1} is the
// filter applied to the extension of c_j (the taps are symmetric; a mirrored position sees a[-k] and a[+k] exchanged, and wv_pass
// adds exactly these pairs first), so the scales are plain shifted reads on the tile, on a region that shrinks by 2 * 2^j per side
// and ends on the output tile.  LDS: three planes of c (stride 76 floats, consecutive lanes on consecutive banks) and one plane for
// the row pass of the channel in work: 4 x 4560 floats = 72 960 B, two workgroups of 512 lanes = 16 waves per CU in 160 KB.  A lane
// owns three output pixels and keeps their c_j and accumulator in registers.  It writes c_F and the accumulator once (or the result,
// when J <= F); the remaining scales run as in route 1.
#include "ics_img_px.h"

namespace {

#define WVF ICS_IMG_WAVELET_FUSED
#define WVTW 48                                // output tile of the fused route
#define WVTH 32
#define WVHALO (2 * ((1 << WVF) - 1))          // 14
#define WVSW (WVTW + 2 * WVHALO)               // staged tile: 76 x 60
#define WVSH (WVTH + 2 * WVHALO)
#define WVN (WVSW * WVSH)
#define WVLANES 512
#define WVPX (WVTW * WVTH / WVLANES)           // output pixels per lane: 3

struct wv_prm { float g[WVF], t[WVF]; };

// acc += g * shrink(cur - nxt, t)
template <bool VEC>
__device__ __forceinline__ void wv_detail(const float cur[3], const float nxt[3], float t, float g, float acc[3]) {
  float w[3], s[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = __fsub_rn(cur[c], nxt[c]);
  if (VEC) {   // the squares summed in ascending order: the same value for every order of the channels
    const float q0 = __fmul_rn(w[0], w[0]), q1 = __fmul_rn(w[1], w[1]), q2 = __fmul_rn(w[2], w[2]);
    const float lo = fminf(q0, q1), hi = fmaxf(q0, q1);
    const float m = __fsqrt_rn(__fadd_rn(__fadd_rn(fminf(lo, q2), fmaxf(lo, fminf(hi, q2))), fmaxf(hi, q2)));
    const float k = m > 0.f ? __fdiv_rn(fmaxf(__fsub_rn(m, t), 0.f), m) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = __fmul_rn(w[c], k);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = copysignf(fmaxf(__fsub_rn(fabsf(w[c]), t), 0.f), w[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(g, s[c]));
}

__device__ __forceinline__ void wv_out(const float cJ[3], const float acc[3], float residual, float o[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = __fadd_rn(__fmul_rn(residual, cJ[c]), acc[c]);
}

// ---- route 1: scale j, d = 2^j.  first: the accumulator starts at 0; last: out = residual * c_{j+1} + accumulator, cout unused ------
template <bool VEC>
__global__ __launch_bounds__(256) void k_img_wv_scale(const float* __restrict__ cin, float* __restrict__ cout, float* __restrict__ out, int H, int W,
                                                     int d, float gain, float thr, float residual, int first, int last) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long L = 3L * W, p = (long)y * L + 3L * x;
  int xs[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) xs[k] = 3 * wv_fold(x + (k - 2) * d, W);
  float h[5][3], cur[3], nxt[3], acc[3];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const float* row = cin + (long)wv_fold(y + (r - 2) * d, H) * L;
    float a[5][3];
#pragma unroll
    for (int k = 0; k < 5; ++k) ld3(row + xs[k], a[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      h[r][c] = wv_pass(a[0][c], a[1][c], a[2][c], a[3][c], a[4][c]);
      if (r == 2) cur[c] = a[2][c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    nxt[c] = wv_pass(h[0][c], h[1][c], h[2][c], h[3][c], h[4][c]);
    acc[c] = 0.f;
  }
  if (!first) ld3(out + p, acc);
  wv_detail<VEC>(cur, nxt, thr, gain, acc);
  if (last) {
    float o[3];
    wv_out(nxt, acc, residual, o);
    st3(out + p, o);
  } else {
    st3(cout + p, nxt);
    st3(out + p, acc);
  }
}

// ---- route 2: scales 0 .. n - 1 (n <= WVF) on an LDS tile.  last (n == J): out = residual * c_n + accumulator, cout unused ---------
template <bool VEC>
__global__ __launch_bounds__(WVLANES) void k_img_wv_fused(const float* __restrict__ f, float* __restrict__ cout, float* __restrict__ out, int H, int W,
                                                         int n, wv_prm prm, float residual, int last) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sc = lds, *sh = lds + 3 * WVN;                                    // planes c[3][WVSH][WVSW], row pass [WVSH][WVSW]
  const int y0 = blockIdx.y * WVTH - WVHALO, x0 = blockIdx.x * WVTW - WVHALO;   // picture coordinates of tile position (0, 0)
  const long L = 3L * W;
  for (int e = threadIdx.x; e < WVN; e += WVLANES) {
    const int ly = e / WVSW, lx = e - ly * WVSW;
    float v[3];
    ld3(f + (long)wv_fold(y0 + ly, H) * L + 3L * wv_fold(x0 + lx, W), v);
#pragma unroll
    for (int c = 0; c < 3; ++c) sc[c * WVN + e] = v[c];
  }
  __syncthreads();
  int oi[WVPX];
  float cur[WVPX][3], acc[WVPX][3];
#pragma unroll
  for (int k = 0; k < WVPX; ++k) {
    const int e = threadIdx.x + k * WVLANES;
    oi[k] = (WVHALO + e / WVTW) * WVSW + WVHALO + e % WVTW;
#pragma unroll
    for (int c = 0; c < 3; ++c) { cur[k][c] = sc[c * WVN + oi[k]]; acc[k][c] = 0.f; }
  }
#pragma unroll
  for (int j = 0; j < WVF; ++j) {
    if (j >= n) break;
    const int d = 1 << j, m0 = 2 * (d - 1), m1 = 2 * (2 * d - 1);           // c_j is exact m0 pixels inside the staged tile, c_{j+1} m1
    const int rw = WVSW - 2 * m1, nh = rw * (WVSH - 2 * m0), nv = rw * (WVSH - 2 * m1);
    const float inv = 1.f / (float)rw;
    for (int c = 0; c < 3; ++c) {
      float* p = sc + c * WVN;
      for (int e = threadIdx.x; e < nh; e += WVLANES) {                      // rows [m0, WVSH - m0), columns [m1, WVSW - m1)
        const int r = (int)(((float)e + 0.5f) * inv), i = (m0 + r) * WVSW + m1 + (e - r * rw);
        sh[i] = wv_pass(p[i - 2 * d], p[i - d], p[i], p[i + d], p[i + 2 * d]);
      }
      __syncthreads();
      for (int e = threadIdx.x; e < nv; e += WVLANES) {                      // rows [m1, WVSH - m1), the same columns; c_{j+1} in place
        const int r = (int)(((float)e + 0.5f) * inv), i = (m1 + r) * WVSW + m1 + (e - r * rw);
        p[i] = wv_pass(sh[i - 2 * d * WVSW], sh[i - d * WVSW], sh[i], sh[i + d * WVSW], sh[i + 2 * d * WVSW]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < WVPX; ++k) {
      float nxt[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) nxt[c] = sc[c * WVN + oi[k]];
      wv_detail<VEC>(cur[k], nxt, prm.t[j], prm.g[j], acc[k]);
#pragma unroll
      for (int c = 0; c < 3; ++c) cur[k][c] = nxt[c];
    }
  }
#pragma unroll
  for (int k = 0; k < WVPX; ++k) {
    const int e = threadIdx.x + k * WVLANES, y = blockIdx.y * WVTH + e / WVTW, x = blockIdx.x * WVTW + e % WVTW;
    if (y >= H || x >= W) continue;
    const long q = (long)y * L + 3L * x;
    if (last) {
      float o[3];
      wv_out(cur[k], acc[k], residual, o);
      st3(out + q, o);
    } else {
      st3(cout + q, cur[k]);
      st3(out + q, acc[k]);
    }
  }
}

}  // namespace

size_t ics_img_wavelet_fused_lds() { return (size_t)4 * WVN * sizeof(float); }

// H x W x 3 frames for the c_j a run writes (the last scale writes the result, not c_J)
int ics_img_wavelet_frames(int scales, int route) {
  const int writes = route == 2 ? (scales > WVF ? scales - WVF : 0) : scales - 1;
  return writes < 2 ? writes : 2;
}

hipError_t ics_launch_img_wavelet(const float* f, int H, int W, int scales, const float* gains, const float* thresholds, float residual,
                                  int coupling, int route, float* const tmp[2], float* out, hipStream_t s) {
  if (scales < 1 || scales > ICS_IMG_WAVELET_MAX_SCALES || !gains || (route != 1 && route != 2)) return hipErrorInvalidValue;
  const float* cin = f;
  int j = 0, w = 0;
  if (route == 2) {
    const int n = scales < WVF ? scales : WVF, last = n == scales;
    wv_prm prm;
    for (int i = 0; i < WVF; ++i) { prm.g[i] = i < n ? gains[i] : 0.f; prm.t[i] = i < n && thresholds ? thresholds[i] : 0.f; }
    const size_t lds = ics_img_wavelet_fused_lds();
    hipError_t e = coupling ? set_dynamic_lds(k_img_wv_fused<true>, lds) : set_dynamic_lds(k_img_wv_fused<false>, lds);
    if (e != hipSuccess) return e;
    const dim3 grid((W + WVTW - 1) / WVTW, (H + WVTH - 1) / WVTH);
    float* cout = last ? nullptr : tmp[0];
    ICS_LAUNCH_VEC(coupling, k_img_wv_fused, grid, dim3(WVLANES), lds, s, f, cout, out, H, W, n, prm, residual, last);
    cin = cout; j = n; w = 1;
  }
  const dim3 grid((W + 63) / 64, (H + 3) / 4);
  for (; j < scales; ++j, ++w) {
    const int last = j == scales - 1;
    float* cout = last ? nullptr : tmp[w & 1];
    const float g = gains[j], t = thresholds ? thresholds[j] : 0.f;
    ICS_LAUNCH_VEC(coupling, k_img_wv_scale, grid, dim3(256), 0, s, cin, cout, out, H, W, 1 << j, g, t, residual, j == 0, last);
    cin = cout;
  }
  return hipGetLastError();
}
