// ics_img_mask.hip -- the window of a device-resident image on which the blind phase should estimate the PSF (ics_img_window_scores,
// include/ics_hip.h): H x W x 3 float32, HWC, contiguous.  A window is good when it holds strong edges in every orientation and no clipped
// pixels: the score is the smaller eigenvalue of the window's structure tensor of luma differences (Shi and Tomasi), clipped pixels left out.
//
//   usable   = |R|, |G|, |B| all < clip (a NaN or an inf is never usable)
//   Y        = (R + G + B) * (1 / 3), every operation rounded once (px_luma)
//   dx[y,x]  = Y[y,x+1] - Y[y,x] where x + 1 < x1 and both pixels are usable, else 0; dy[y,x] = Y[y+1,x] - Y[y,x] likewise with y + 1 < y1
//   cells    : MKCELL x MKCELL pixels, the grid anchored at (y0 + off, x0 + off), n = size / MKCELL, off = (size - MKCELL n) / 2;
//              per cell Sxx = sum dx dx, Syy = sum dy dy, Sxy = sum dx dy and the number of unusable pixels
//   box (i,j): origin (y0 + MKCELL i, x0 + MKCELL j), the cells [i, i + n) x [j, j + n) summed in double in row-major order;
//              trace = (Sxx + Syy) / (MKCELL n)^2, score = max(0, (Sxx + Syy - sqrt((Sxx - Syy)^2 + 4 Sxy^2)) / 2 / (MKCELL n)^2)
//   choice   : the largest score, ties to the lowest i, then the lowest j
//
// k_img_mk_cells: persistent workgroups of 256 lanes walk the MKT x MKT pixel tiles (4 x 4 cells) of the cell grid.  A tile stages its
// luma, one more column and one more row than the tile, in LDS once: every pixel is read from HBM once per tile, its three channels are
// tested there and an unusable pixel -- or a position outside the region -- is staged as NaN, so that a difference is dropped by one
// unordered compare of its two lumas.  Wave w owns cell row w of the tile and lane l column l: it walks the 16 rows of its column (per row
// two LDS reads, the luma below and the one right of that; the pixel's own and its right neighbour are the two read a row earlier),
// adds the three products and the NaN count in row order, and the 16 columns of a cell are added by four exchanges inside the row of
// 16 lanes (distance 8, 4, 2, 1): float32 in one fixed order, no atomics.  Lane 0 of a cell stores {Sxx, Syy, Sxy, count (as bits)}.
// k_img_mk_windows: a lane per candidate box, the n x n cells summed directly (the table lives in L2).  k_img_mk_pick: one workgroup,
// the arg-max with the tie rule, {i, j, score, trace, clipped} to the result block.
#include "ics_img_px.h"

namespace {

#define MKT 64                                 // tile side in pixels: MKT / MKCELL cells a side
#define MKCELL ICS_IMG_MASK_CELL
#define MKLANES 256
#define MKP (MKT + 1)                          // rows and pitch of the staged luma: the tile and the pixels that complete its differences
#define MKSTAGE (MKP * MKP / MKLANES)          // full staging rounds: 16 (a 17th covers the remaining MKP * MKP - 16 * 256 = 129 lumas)

static_assert(MKCELL == 16 && MKT == 64 && MKLANES == 4 * 64 && MKT / MKCELL == MKLANES / 64, "a wave per cell row, a lane per column, 16 lanes per cell");

// luma number idx of the tile at (by, bx): NaN for an unusable pixel and for a position outside the region (the load is clamped into it)
__device__ __forceinline__ float mk_stage(const float* __restrict__ f, long pitch, int by, int bx, int y1, int x1, float clip, int idx) {
  const int r = idx / MKP, c = idx - r * MKP, y = by + r, x = bx + c;
  float v[3];
  ld3(f + (long)min(y, y1 - 1) * pitch + 3L * min(x, x1 - 1), v);
  const bool usable = fabsf(v[0]) < clip && fabsf(v[1]) < clip && fabsf(v[2]) < clip && y < y1 && x < x1;
  return usable ? px_luma(v) : __builtin_nanf("");
}

__global__ __launch_bounds__(MKLANES) void k_img_mk_cells(const float* __restrict__ f, int W, int y1, int x1, int oy, int ox, int ncy, int ncx, float clip,
                                                          float4* __restrict__ cells) {
  __shared__ float Y[MKP * MKP];
  const int tx = (ncx + MKT / MKCELL - 1) / (MKT / MKCELL), tiles = tx * ((ncy + MKT / MKCELL - 1) / (MKT / MKCELL));
  const long pitch = 3L * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t / tx, tc = t - ty * tx, by = oy + ty * MKT, bx = ox + tc * MKT;
    __syncthreads();                                                         // the tile before is done with
#pragma unroll 8
    for (int k = 0; k < MKSTAGE; ++k) Y[k * MKLANES + threadIdx.x] = mk_stage(f, pitch, by, bx, y1, x1, clip, k * MKLANES + threadIdx.x);
    if (MKSTAGE * MKLANES + threadIdx.x < MKP * MKP) Y[MKSTAGE * MKLANES + threadIdx.x] = mk_stage(f, pitch, by, bx, y1, x1, clip, MKSTAGE * MKLANES + threadIdx.x);
    __syncthreads();
    const float* p = Y + wave * MKCELL * MKP + lane;
    float a = p[0], b = p[1], sxx = 0.f, syy = 0.f, sxy = 0.f;
    int bad = 0;
#pragma unroll
    for (int r = 1; r <= MKCELL; ++r) {
      const float d = p[r * MKP], e = p[r * MKP + 1];                        // below, and right of that
      const float dx = __builtin_isunordered(a, b) ? 0.f : __fsub_rn(b, a);
      const float dy = __builtin_isunordered(a, d) ? 0.f : __fsub_rn(d, a);
      sxx = __fadd_rn(sxx, __fmul_rn(dx, dx));
      syy = __fadd_rn(syy, __fmul_rn(dy, dy));
      sxy = __fadd_rn(sxy, __fmul_rn(dx, dy));
      bad += a != a;
      a = d; b = e;
    }
#pragma unroll
    for (int m = MKCELL / 2; m > 0; m >>= 1) {
      sxx = __fadd_rn(sxx, __shfl_xor(sxx, m));
      syy = __fadd_rn(syy, __shfl_xor(syy, m));
      sxy = __fadd_rn(sxy, __shfl_xor(sxy, m));
      bad += __shfl_xor(bad, m);
    }
    const int cy = ty * (MKT / MKCELL) + wave, cx = tc * (MKT / MKCELL) + lane / MKCELL;
    if (lane % MKCELL == 0 && cy < ncy && cx < ncx) cells[(long)cy * ncx + cx] = make_float4(sxx, syy, sxy, __int_as_float(bad));
  }
}

// a lane per candidate: the cells [i, i + n) x [j, j + n) in row-major order in double; table = score[cand], trace[cand], clipped[cand]
__global__ __launch_bounds__(256) void k_img_mk_windows(const float4* __restrict__ cells, int ncx, int nci, int ncj, int n, double* __restrict__ table) {
  const int cand = nci * ncj, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cand) return;
  const int i = c / ncj, j = c - i * ncj;
  double sxx = 0.0, syy = 0.0, sxy = 0.0;
  long long bad = 0;
  const auto add = [&](const float4 v) {
    sxx = __dadd_rn(sxx, (double)v.x);
    syy = __dadd_rn(syy, (double)v.y);
    sxy = __dadd_rn(sxy, (double)v.z);
    bad += __float_as_int(v.w);
  };
  for (int cy = i; cy < i + n; ++cy) {
    const float4* row = cells + (long)cy * ncx + j;
    int k = 0;
    for (; k + 8 <= n; k += 8) {                                             // eight loads in flight, added in order (a large box is bound by the bytes they move from L2)
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = row[k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) add(v[u]);
    }
    for (; k < n; ++k) add(row[k]);
  }
  const double side = (double)(MKCELL * n), area = side * side;              // (exact)
  const double tr = __dadd_rn(sxx, syy), df = __dsub_rn(sxx, syy);
  const double root = __dsqrt_rn(__dadd_rn(__dmul_rn(df, df), __dmul_rn(4.0, __dmul_rn(sxy, sxy))));
  const double sc = __ddiv_rn(__dmul_rn(0.5, __dsub_rn(tr, root)), area);
  table[c] = sc > 0.0 ? sc : 0.0;
  table[cand + c] = __ddiv_rn(tr, area);
  reinterpret_cast<long long*>(table)[2L * cand + c] = bad;
}

// one workgroup: the largest score, ties to the lowest candidate number (row-major: the lowest i, then the lowest j)
#define MKPICK 1024
__global__ __launch_bounds__(MKPICK) void k_img_mk_pick(const double* __restrict__ table, int cand, int ncj, double* __restrict__ result) {
  __shared__ double bs[MKPICK];
  __shared__ int bc[MKPICK];
  double best = -1.0;                                                        // (every score is >= 0)
  int at = 0x7fffffff;
  int c = threadIdx.x;
  for (; c + 7 * MKPICK < cand; c += 8 * MKPICK) {                           // eight loads in flight, compared in candidate order
    double s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = table[c + k * MKPICK];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s[k] > best) { best = s[k]; at = c + k * MKPICK; }
  }
  for (; c < cand; c += MKPICK) {
    const double s = table[c];
    if (s > best) { best = s; at = c; }
  }
  bs[threadIdx.x] = best; bc[threadIdx.x] = at;
  __syncthreads();
  for (int h = MKPICK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      const double s = bs[threadIdx.x + h];
      const int o = bc[threadIdx.x + h];
      if (s > bs[threadIdx.x] || (s == bs[threadIdx.x] && o < bc[threadIdx.x])) { bs[threadIdx.x] = s; bc[threadIdx.x] = o; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int w = bc[0];
    result[0] = (double)(w / ncj);
    result[1] = (double)(w % ncj);
    result[2] = bs[0];
    result[3] = table[cand + w];
    result[4] = (double)reinterpret_cast<const long long*>(table)[2L * cand + w];
  }
}

}  // namespace

size_t ics_img_mask_lds() { return (size_t)MKP * MKP * sizeof(float); }
int ics_img_mask_candidates(int extent, int size) { return size >= MKCELL && extent >= size ? (extent - size) / MKCELL + 1 : 0; }
int ics_img_mask_cells(int extent, int size) { const int c = ics_img_mask_candidates(extent, size); return c > 0 ? c - 1 + size / MKCELL : 0; }

hipError_t ics_launch_img_mask(const float* f, int H, int W, int y0, int y1, int x0, int x1, int size, float clip, int cus, float* cells, double* table, double* result,
                               hipStream_t s) {
  if (!f || !cells || !table || !result || y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1 || size < MKCELL || !(clip > 0.f)) return hipErrorInvalidValue;
  const int nci = ics_img_mask_candidates(y1 - y0, size), ncj = ics_img_mask_candidates(x1 - x0, size);
  if (nci <= 0 || ncj <= 0) return hipErrorInvalidValue;
  const int n = size / MKCELL, off = (size - MKCELL * n) / 2, ncy = nci - 1 + n, ncx = ncj - 1 + n;   // (the last cell ends at or before y1, x1)
  if ((long)ncy * ncx > 0x7fffffffL / 4) return hipErrorInvalidValue;
  const int per = MKT / MKCELL;
  const long tiles = (long)((ncx + per - 1) / per) * ((ncy + per - 1) / per);
  // persistent workgroups, eight per CU (two waves of each per SIMD: the kernel stays below 64 registers, eight times its LDS is 135 KB of
  // 160): a tile is loads, a barrier, arithmetic, a barrier, and what hides one workgroup's loads is the others' work
  long grid = (long)(cus > 0 ? cus : 256) * 8;
  if (const int m = ics_debug().max_wgs.load(std::memory_order_relaxed); m > 0 && grid > m) grid = m;   // test hook: several tiles per workgroup on small frames
  if (grid > tiles) grid = tiles;
  const int cand = nci * ncj;
  hipLaunchKernelGGL(k_img_mk_cells, dim3((unsigned)grid), dim3(MKLANES), 0, s, f, W, y1, x1, y0 + off, x0 + off, ncy, ncx, clip, reinterpret_cast<float4*>(cells));
  hipLaunchKernelGGL(k_img_mk_windows, dim3((unsigned)((cand + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(cells), ncx, nci, ncj, n, table);
  hipLaunchKernelGGL(k_img_mk_pick, dim3(1), dim3(MKPICK), 0, s, table, cand, ncj, result);
  return hipGetLastError();
}
