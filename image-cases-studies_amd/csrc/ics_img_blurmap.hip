// ics_img_blurmap.hip -- map of the local blur width of device-resident images (ics_img_blur_map, include/ics_hip.h): H x W x 3 float32,
// HWC, contiguous.  Zhuo and Sim's gradient ratio: the luma smoothed by two Gaussians sa < sb; at an edge pixel of a step blurred by a
// Gaussian of s the gradient magnitudes stand in the ratio R = sqrt((s^2 + sb^2) / (s^2 + sa^2)), hence s^2 = (sb^2 - R^2 sa^2) / (R^2 - 1).
//
// Over the window [y0, y1) x [x0, x1), every coordinate clamped to the window, every operation rounded once (no FMA):
//   Y        = (R + G + B) * (1 / 3) (px_luma)
//   S_s      = the rows pass, then the columns pass with the taps g_s[-r .. r] of the host's table: acc = 0, acc = acc + g[i] * v, i ascending
//   gx, gy   = 0.5 * (S[y, x+1] - S[y, x-1]), 0.5 * (S[y+1, x] - S[y-1, x]);  A, B = sqrt(gx gx + gy gy) of S_sa, of S_sb
//   sector   : ics_img_edges.hip's rule on the gradient of S_sa; neighbour offsets (dy, dx) = (0, 1), (1, 1), (1, 0), (1, -1)
//   kept     : A > A[y+dy, x+dx], A >= A[y-dy, x-dx], A >= edge, B > 0, R = A / B > 1, s2 = (sb^2 - (R R) sa^2) / (R R - 1) <= max_sigma^2;
//              sigma = sqrt(max(s2, 0))
//   cells    : BMCELL x BMCELL pixels from the window's origin: weight = sum A, moment = sum A sigma, count, over the kept pixels; a pixel
//              that is not kept adds exactly 0; a row left to right, the row sums top to bottom
//
// k_img_bm: persistent workgroups of 512 lanes walk the BMTH x BMTW pixel tiles (2 x 4 cells) of the window.  With r = r_b a tile stages
// the luma with a halo of r + 2 pixels, Y[BMTH + 4 + 2 r][BMTW + 4 + 2 r], at the clamped coordinates, so that the passes need no
// clamping of their own: the rows pass gives Sh_a and Sh_b on [BMTH + 4 + 2 r][BMTW + 4], the columns pass S_a and S_b on
// [BMTH + 4][BMTW + 4] (two pixels around the tile: the gradients of the tile's neighbours), then A on [BMTH + 2][BMTW + 2] (one pixel
// around it: the suppression's neighbours), in the plane Sh_a leaves free.  Gradients and the suppression read their neighbours at the
// tile position of the clamped picture coordinate; positions outside the window are never read.  A lane then takes four pixels:
// gradients of both planes, sector, suppression, ratio, and stores A and A sigma (0 where not kept) transposed at pitch BMTH + 1 over
// the dead Y plane; lane (cell column, tile row) of the first two waves adds the 16 values of its cell row in order, lane c of the
// first eight the 16 row sums of cell c: float32 in one fixed order, no atomics.  The pixels whose luma is not finite are counted per
// workgroup (integers: any order) and stored at bad[workgroup].
#include "ics_img_px.h"

namespace {

#define BMCELL ICS_IMG_BLURMAP_CELL
#define BMR ICS_IMG_BLURMAP_MAX_RADIUS
#define BMTH 32                                // tile: rows ...
#define BMTW 64                                // ... and columns
#define BMLANES 512
#define BMSH (BMTH + 4)                        // rows of S
#define BMSW (BMTW + 4)                        // columns of Sh and S
#define BMAH (BMTH + 2)                        // rows of A
#define BMAW (BMTW + 2)                        // columns of A
#define BMVP (BMTH + 1)                        // pitch of the transposed value planes
#define BMCELLS ((BMTH / BMCELL) * (BMTW / BMCELL))
#define BMROWS (3 * BMCELLS * BMCELL)          // row sums: weight, moment, count

static_assert(BMCELL == 16 && BMTH % BMCELL == 0 && BMTW % BMCELL == 0 && BMTH * BMTW == 4 * BMLANES && (BMTW / BMCELL) * BMTH <= BMLANES && BMCELLS <= 64, "lane layout");
static_assert(2 * BMTW * BMVP <= (BMSH + 4) * (BMSW + 4) + (BMSH + 4) * BMSW && BMAH * BMAW <= (BMSH + 4) * BMSW, "the planes that are reused hold what reuses them at the smallest radius (2)");

// (sqrtf: correctly rounded, see ics_img_noise.hip; __fsqrt_rn is the native approximation here)
__device__ __forceinline__ float bm_mag(float gx, float gy) { return sqrtf(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy))); }

// one pass at one position with the taps of sigma_b: acc = 0, acc = acc + g[|j|] * p[j * step], j = -RB .. RB (the taps are symmetric, g[k]
// the tap at distance k, the same in every lane: scalar registers)
template <int RB>
__device__ __forceinline__ float bm_pass_b(const float g[RB + 1], const float* p, int step) {
  float acc = 0.f;
#pragma unroll
  for (int j = -RB; j <= RB; ++j) acc = __fadd_rn(acc, __fmul_rn(g[j < 0 ? -j : j], p[j * step]));
  return acc;
}
// ... and with those of sigma_a, whose radius the kernel is not compiled for: the 2 ra + 1 taps wait in LDS
__device__ __forceinline__ float bm_pass_a(const float* g, const float* p, int step, int ra) {
  float acc = 0.f;
  p -= ra * step;
  for (int i = 0; i <= 2 * ra; ++i) acc = __fadd_rn(acc, __fmul_rn(g[i], p[i * step]));
  return acc;
}

// (two workgroups per CU, four waves per SIMD: 128 registers)
template <int RB>
__global__ __launch_bounds__(BMLANES) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_img_bm(const float* __restrict__ f, int W, int y0, int y1, int x0, int x1, int ra,
                                                            const float* __restrict__ taps, float sa2, float sb2, float edge, float ms2,
                                                            float* __restrict__ weight, float* __restrict__ moment, int* __restrict__ count, int* __restrict__ bad,
                                                            float* __restrict__ sparse, int rows, int cols) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int r = RB, YH = BMSH + 2 * r, YW = BMSW + 2 * r;
  float *Y = lds, *Shb = Y + YH * YW, *Sha = Shb + YH * BMSW, *Sa = Sha + YH * BMSW, *Sb = Sa + BMSH * BMSW, *rsum = Sb + BMSH * BMSW;
  float *Ap = Sha, *vw = Y, *vm = Y + BMTW * BMVP;                           // A in the plane of Sh_a; the value planes over Y (and the head of Sh_b)
  float gb[RB + 1];
#pragma unroll
  for (int k = 0; k <= RB; ++k) gb[k] = taps[2 * BMR + 1 + RB + k];
  float* ga = rsum + BMROWS;
  if ((int)threadIdx.x <= 2 * ra) ga[threadIdx.x] = taps[threadIdx.x];          // (the first barrier of the first tile stands before their first use)
  const int hw = y1 - y0, ww = x1 - x0;
  const int tx = (ww + BMTW - 1) / BMTW, tiles = tx * ((hw + BMTH - 1) / BMTH);
  const long pitch = 3L * W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nbad = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t / tx, tc = t - ty * tx, by = y0 + ty * BMTH, bx = x0 + tc * BMTW;
    __syncthreads();                                                         // the tile before is done with
    // the luma with its halo: a wave per row, a lane per column
    for (int yy = wave; yy < YH; yy += BMLANES / 64) {
      const float* row = f + (long)min(max(by - r - 2 + yy, y0), y1 - 1) * pitch;
      for (int xx = lane; xx < YW; xx += 64) {
        float v[3];
        ld3(row + 3L * min(max(bx - r - 2 + xx, x0), x1 - 1), v);
        Y[yy * YW + xx] = px_luma(v);
      }
    }
    __syncthreads();
    // rows pass: Sh[yy][xs] = sum g[i] Y[yy][xs + r + i]
    for (int o = tid; o < YH * BMSW; o += BMLANES) {
      const int yy = o / BMSW, xs = o - yy * BMSW;
      const float* p = Y + yy * YW + xs + r;
      Sha[o] = bm_pass_a(ga, p, 1, ra); Shb[o] = bm_pass_b<RB>(gb, p, 1);
    }
    __syncthreads();
    // columns pass: S[ys][xs] = sum g[i] Sh[ys + r + i][xs]
    for (int o = tid; o < BMSH * BMSW; o += BMLANES) {
      Sa[o] = bm_pass_a(ga, Sha + o + r * BMSW, BMSW, ra); Sb[o] = bm_pass_b<RB>(gb, Shb + o + r * BMSW, BMSW);
    }
    __syncthreads();
    // A one pixel around the tile, inside the window; S at the picture coordinate (y, x) is S[y - (by - 2)][x - (bx - 2)].  The tile's
    // own pixels are looked at for a luma that is not finite here, while Y still stands
    for (int o = tid; o < BMAH * BMAW; o += BMLANES) {
      const int ya = o / BMAW, xa = o - ya * BMAW, gy = by - 1 + ya, gx = bx - 1 + xa;
      if (gy < y0 || gy >= y1 || gx < x0 || gx >= x1) continue;
      const int sy = gy - (by - 2), sx = gx - (bx - 2);
      const int syp = min(gy + 1, y1 - 1) - (by - 2), sym = max(gy - 1, y0) - (by - 2), sxp = min(gx + 1, x1 - 1) - (bx - 2), sxm = max(gx - 1, x0) - (bx - 2);
      const float ax = __fmul_rn(0.5f, __fsub_rn(Sa[sy * BMSW + sxp], Sa[sy * BMSW + sxm]));
      const float ay = __fmul_rn(0.5f, __fsub_rn(Sa[syp * BMSW + sx], Sa[sym * BMSW + sx]));
      Ap[o] = bm_mag(ax, ay);
      if (ya >= 1 && ya <= BMTH && xa >= 1 && xa <= BMTW) {
        const float l = Y[(ya + 1 + r) * YW + xa + 1 + r];
        nbad += !(fabsf(l) < __builtin_inff());
      }
    }
    __syncthreads();
    // four pixels per lane: consecutive lanes on consecutive columns
#pragma unroll 1
    for (int k = 0; k < BMTH * BMTW / BMLANES; ++k) {
      const int p = tid + k * BMLANES, py = p / BMTW, px = p - py * BMTW, gy = by + py, gx = bx + px;
      float w = 0.f, m = 0.f;
      if (gy < y1 && gx < x1) {
        const int sy = py + 2, sx = px + 2;
        const int syp = min(gy + 1, y1 - 1) - (by - 2), sym = max(gy - 1, y0) - (by - 2), sxp = min(gx + 1, x1 - 1) - (bx - 2), sxm = max(gx - 1, x0) - (bx - 2);
        const float ax = __fmul_rn(0.5f, __fsub_rn(Sa[sy * BMSW + sxp], Sa[sy * BMSW + sxm]));
        const float ay = __fmul_rn(0.5f, __fsub_rn(Sa[syp * BMSW + sx], Sa[sym * BMSW + sx]));
        const float A = Ap[(py + 1) * BMAW + px + 1];
        const float fx = fabsf(ax), fy = fabsf(ay);
        int dy, dx;
        if (fy <= __fmul_rn(0.41421357f, fx)) { dy = 0; dx = 1; }
        else if (fx <= __fmul_rn(0.41421357f, fy)) { dy = 1; dx = 0; }
        else { dy = 1; dx = __fmul_rn(ax, ay) > 0.f ? 1 : -1; }
        const float fwd = Ap[(min(max(gy + dy, y0), y1 - 1) - (by - 1)) * BMAW + min(max(gx + dx, x0), x1 - 1) - (bx - 1)];
        const float back = Ap[(min(max(gy - dy, y0), y1 - 1) - (by - 1)) * BMAW + min(max(gx - dx, x0), x1 - 1) - (bx - 1)];
        float sg = -1.f;
        if (A > fwd && A >= back && A >= edge) {                             // an edge pixel: few of a picture's, and only they pay for the ratio
          const float cx = __fmul_rn(0.5f, __fsub_rn(Sb[sy * BMSW + sxp], Sb[sy * BMSW + sxm]));
          const float cy = __fmul_rn(0.5f, __fsub_rn(Sb[syp * BMSW + sx], Sb[sym * BMSW + sx]));
          const float B = bm_mag(cx, cy);
          const float R = __fdiv_rn(A, B), R2 = __fmul_rn(R, R);
          const float s2 = __fdiv_rn(__fsub_rn(sb2, __fmul_rn(R2, sa2)), __fsub_rn(R2, 1.f));
          if (B > 0.f && R > 1.f && s2 <= ms2) {
            sg = sqrtf(fmaxf(s2, 0.f));
            w = A; m = __fmul_rn(A, sg);
          }
        }
        if (sparse) sparse[(long)(gy - y0) * ww + (gx - x0)] = sg;
      }
      vw[px * BMVP + py] = w;
      vm[px * BMVP + py] = m;
    }
    __syncthreads();
    // lane (cell column c4, tile row yr): the 16 values of its cell row, left to right
    if (tid < (BMTW / BMCELL) * BMTH) {
      const int c4 = tid / BMTH, yr = tid - c4 * BMTH;
      float sw = 0.f, sm = 0.f;
      int n = 0;
#pragma unroll
      for (int j = 0; j < BMCELL; ++j) {
        const float w = vw[(c4 * BMCELL + j) * BMVP + yr];
        sw = __fadd_rn(sw, w);
        sm = __fadd_rn(sm, vm[(c4 * BMCELL + j) * BMVP + yr]);
        n += w > 0.f;                                                        // (a kept pixel has A >= edge > 0)
      }
      const int o = ((yr / BMCELL) * (BMTW / BMCELL) + c4) * BMCELL + yr % BMCELL;
      rsum[o] = sw; rsum[BMCELLS * BMCELL + o] = sm; rsum[2 * BMCELLS * BMCELL + o] = __int_as_float(n);
    }
    __syncthreads();
    // lane c: the 16 row sums of cell c, top to bottom
    if (tid < BMCELLS) {
      const int cy = ty * (BMTH / BMCELL) + tid / (BMTW / BMCELL), cx = tc * (BMTW / BMCELL) + tid % (BMTW / BMCELL);
      float sw = 0.f, sm = 0.f;
      int n = 0;
#pragma unroll
      for (int j = 0; j < BMCELL; ++j) {
        sw = __fadd_rn(sw, rsum[tid * BMCELL + j]);
        sm = __fadd_rn(sm, rsum[BMCELLS * BMCELL + tid * BMCELL + j]);
        n += __float_as_int(rsum[2 * BMCELLS * BMCELL + tid * BMCELL + j]);
      }
      if (cy < rows && cx < cols) {
        weight[(long)cy * cols + cx] = sw; moment[(long)cy * cols + cx] = sm; count[(long)cy * cols + cx] = n;
      }
    }
  }
  // the workgroup's pixels that are not finite: over the wave, then over the waves
  __syncthreads();
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) nbad += __shfl_xor(nbad, m);
  int* wb = reinterpret_cast<int*>(rsum);
  if (lane == 0) wb[wave] = nbad;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int i = 0; i < BMLANES / 64; ++i) s += wb[i];
    bad[blockIdx.x] = s;
  }
}

}  // namespace

size_t ics_img_blurmap_lds(int r) {
  return ((size_t)(BMSH + 2 * r) * (BMSW + 2 * r) + (size_t)2 * (BMSH + 2 * r) * BMSW + (size_t)2 * BMSH * BMSW + BMROWS + 2 * BMR + 1) * sizeof(float);
}
int ics_img_blurmap_radius(float sigma) { return (int)ceilf(3.f * sigma); }
long ics_img_blurmap_tiles(int hw, int ww) { return (long)((ww + BMTW - 1) / BMTW) * ((hw + BMTH - 1) / BMTH); }
int ics_img_blurmap_grid(int hw, int ww, int cus) {
  // persistent workgroups, two per CU: 66 948 B of LDS each at the largest radius, four waves per SIMD at 128 registers
  long grid = (long)(cus > 0 ? cus : 256) * 2;
  if (const int m = ics_debug().max_wgs.load(std::memory_order_relaxed); m > 0 && grid > m) grid = m;   // test hook: several tiles per workgroup on small frames
  const long tiles = ics_img_blurmap_tiles(hw, ww);
  return (int)(grid > tiles ? tiles : grid);
}
// the normalised taps of sigma, 2 r + 1 of them: exponentials summed in ascending order and divided in double, rounded to float32
void ics_img_blurmap_taps(float sigma, float* g) {
  const int r = ics_img_blurmap_radius(sigma);
  const double s = (double)sigma;
  double e[2 * BMR + 1], tot = 0.0;
  for (int i = -r; i <= r; ++i) { e[i + r] = exp(-(double)(i * i) / (2.0 * s * s)); tot += e[i + r]; }
  for (int i = 0; i <= 2 * r; ++i) g[i] = (float)(e[i] / tot);
}

hipError_t ics_launch_img_blurmap(const float* f, int H, int W, int y0, int y1, int x0, int x1, float sigma_a, float sigma_b, float edge, float max_sigma, int grid,
                                  const float* taps, float* weight, float* moment, int* count, int* bad, float* sparse, hipStream_t s) {
  if (!f || !taps || !weight || !moment || !count || !bad || y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1) return hipErrorInvalidValue;
  if (!(sigma_a >= 0.5f) || !(sigma_a < sigma_b) || !(edge > 0.f) || !(max_sigma > 0.f)) return hipErrorInvalidValue;
  const int ra = ics_img_blurmap_radius(sigma_a), r = ics_img_blurmap_radius(sigma_b);
  if (ra < 2 || r > BMR || ra > r) return hipErrorInvalidValue;
  const long tiles = ics_img_blurmap_tiles(y1 - y0, x1 - x0);
  if (grid < 1 || grid > tiles || tiles > 0x7fffffffL) return hipErrorInvalidValue;
  const int rows = (y1 - y0 + BMCELL - 1) / BMCELL, cols = (x1 - x0 + BMCELL - 1) / BMCELL;
  const size_t lds = ics_img_blurmap_lds(r);
  const auto launch = [&](auto kern) {
    hipError_t e = set_dynamic_lds(kern, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BMLANES), lds, s, f, W, y0, y1, x0, x1, ra, taps, sigma_a * sigma_a, sigma_b * sigma_b, edge,
                       max_sigma * max_sigma, weight, moment, count, bad, sparse, rows, cols);
    return hipGetLastError();
  };
  switch (r) {                                                               // a kernel per radius of sigma_b: its taps in scalar registers, its planes at constant pitches
    case 2: return launch(k_img_bm<2>);
    case 3: return launch(k_img_bm<3>);
    case 4: return launch(k_img_bm<4>);
    case 5: return launch(k_img_bm<5>);
    case 6: return launch(k_img_bm<6>);
    case 7: return launch(k_img_bm<7>);
    default: return launch(k_img_bm<8>);
  }
}
