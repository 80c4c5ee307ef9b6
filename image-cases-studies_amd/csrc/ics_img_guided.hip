// ics_img_guided.hip -- guided filter of device-resident images with the picture as its own guide (ics_img_guided, include/ics_hip.h):
// H x W x 3 float32, HWC, contiguous.  He, Sun and Tang's filter: an edge-preserving base layer q from box means and a closed-form
// solve per pixel, and the detail I - q scaled back onto it.
//
//   I'       = I - 0.5
//   mean(x)  = (sum of x over the (2 r + 1)^2 window clipped to the picture) / (its pixel count, gf_count); a sum runs along x
//              first, then along y, the taps added from zero in ascending offset order -r .. r (gf_box), a tap outside the picture +0
//   channel  mu = mean(I'_c), v = mean(I'_c^2) - mu mu, a = v / (v + eps), b = mu - a mu                                (gf_solve)
//   vector   mu_i = mean(I'_i), S_ij = mean(I'_i I'_j) - mu_i mu_j, M = S + eps E, c_ij its six cofactors,
//            det = (M00 c00 + M01 c01) + M02 c02, A_ij = [i = j] - eps (c_ij / det), b_i = mu_i - ((A_i0 mu_0 + A_i1 mu_1) + A_i2 mu_2)
//                                                                                                                        (gf_solve)
//   q        = (mean(a) I' + mean(b)) + 0.5, or (((mean(A_i0) I'_0 + mean(A_i1) I'_1) + mean(A_i2) I'_2) + mean(b_i)) + 0.5
//   out      = q when detail == 0, else q + detail (I - q)                                                                 (gf_out)
//
// Every value is computed by these inline functions in one fixed order of operations (no FMA, IEEE division) by every route, and a
// box sum never depends on where a tile starts (no running sums), so the routes agree bit for bit and two runs give identical bits.
//
// Planes.  A pixel has K = 6 (channel: mean of I'_c, of I'_c^2) or 9 (vector: mean of I'_i, of the six I'_i I'_j) moment sums and as
// many coefficients (a, b or the six A_ij, b); the coefficient frame is planar, [K][H][W].  All box sums run on LDS planes of odd row
// stride: the row pass has its lanes on consecutive rows (stride odd: one bank each), the column pass on consecutive columns, and a
// lane forms GFP = 4 neighbouring sums from one stream of 2 r + 4 taps held in registers (gf_box), 1 / 4 of the LDS reads.
//
// Route 1, two launches on 32 x 32 output tiles of 256 lanes.  k_img_gf_coef stages I' of the tile plus an r halo (zero outside the
// picture), forms every moment plane by a row pass into a scratch plane and a column pass, solves and writes the coefficients.
// k_img_gf_apply stages one coefficient plane plus halo at a time (zero outside), box-sums it into registers (a lane owns four
// vertical neighbours: 4 K sums), reads I and writes the result.  Algorithmic bytes per pixel: 12 + 4 K written, 4 K + 12 read, 12
// written = 84 (channel) / 108 (vector).  LDS of k_img_gf_coef at r = 32: 3 x 96 x 97 + 96 x 33 + K x 32 x 33 floats = 162 432 B
// (vector), one workgroup per CU; at r = 8 72 576 B, two; k_img_gf_apply: 49 920 B at r = 32, 15 744 B at r = 8.
//
// Route 2 (k_img_gf_fused), r <= ICS_IMG_GUIDED_FUSED_RADIUS: the same two phases in one launch, the coefficients of the tile plus an
// r halo kept in LDS.  The coefficient region is C x C, C = 32 + 2 r rounded up to a multiple of 4 (whole groups of GFP), I' is staged
// on (C + 2 r)^2: 3 (C + 2 r)(C + 2 r + 1) + (C + 2 r)(C + 1) + K C (C + 1) floats, 147 136 B at r = 8 (vector), 173 696 B at r = 9.
#include "ics_img_px.h"

namespace {

#define GFT 32                         // output tile edge
#define GFP 4                          // neighbouring sums a lane forms from one stream of taps
#define GFLANES 256                    // (GFT / GFP) * GFT: in the apply phase a lane owns GFP vertical neighbours

// ---- the arithmetic every route shares ------------------------------------------------------------------------------------------
// pixels of the window of (y, x) that lie in the picture
__device__ __forceinline__ float gf_count(int y, int x, int H, int W, int r) {
  const int ny = min(y + r, H - 1) - max(y - r, 0) + 1, nx = min(x + r, W - 1) - max(x - r, 0) + 1;
  return (float)(ny * nx);
}

// acc[i] = sum over t = i .. i + r2 of v(t), v(t) = a[t * st] (PROD: * b[t * st]), each sum from zero in ascending t
template <bool PROD>
__device__ __forceinline__ void gf_box(const float* a, const float* b, int st, int r2, float acc[GFP]) {
#pragma unroll
  for (int i = 0; i < GFP; ++i) acc[i] = 0.f;
  int t = 0;
#pragma unroll
  for (; t < GFP - 1; ++t) {
    const float v = PROD ? __fmul_rn(a[t * st], b[t * st]) : a[t * st];
#pragma unroll
    for (int i = 0; i < GFP; ++i) if (t >= i && t <= i + r2) acc[i] = __fadd_rn(acc[i], v);
  }
  for (; t <= r2; ++t) {               // the taps all GFP windows hold
    const float v = PROD ? __fmul_rn(a[t * st], b[t * st]) : a[t * st];
#pragma unroll
    for (int i = 0; i < GFP; ++i) acc[i] = __fadd_rn(acc[i], v);
  }
  for (; t < r2 + GFP; ++t) {
    const float v = PROD ? __fmul_rn(a[t * st], b[t * st]) : a[t * st];
#pragma unroll
    for (int i = 0; i < GFP; ++i) if (t >= i && t <= i + r2) acc[i] = __fadd_rn(acc[i], v);
  }
}

// the distinct entries (i, j), i <= j, of a symmetric 3 x 3 in the order 00 01 02 11 12 22
__device__ __forceinline__ int gf_pi(int p) { return p < 3 ? 0 : p < 5 ? 1 : 2; }
__device__ __forceinline__ int gf_pj(int p) { return p < 3 ? p : p < 5 ? p - 2 : 2; }
__device__ __forceinline__ int gf_at(int i, int j) { const int lo = i < j ? i : j, hi = i < j ? j : i; return lo == 0 ? hi : lo + hi + 1; }

// m: the K moment means of a pixel -> k: its K coefficients
template <bool VEC>
__device__ __forceinline__ void gf_solve(const float* m, float eps, float* k) {
  if (!VEC) {                          // gf_channel: m = mu[3], mean(I'^2)[3]; k = a[3], b[3]
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float mu = m[c], v = __fsub_rn(m[3 + c], __fmul_rn(mu, mu));
      const float a = __fdiv_rn(v, __fadd_rn(v, eps));
      k[c] = a;
      k[3 + c] = __fsub_rn(mu, __fmul_rn(a, mu));
    }
    return;
  }
  // gf_vector: m = mu[3], mean(I'_i I'_j)[6]; k = A[6], b[3]
  float M[6], c[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    M[p] = __fsub_rn(m[3 + p], __fmul_rn(m[gf_pi(p)], m[gf_pj(p)]));
    if (gf_pi(p) == gf_pj(p)) M[p] = __fadd_rn(M[p], eps);
  }
  const float M00 = M[0], M01 = M[1], M02 = M[2], M11 = M[3], M12 = M[4], M22 = M[5];
  c[0] = __fsub_rn(__fmul_rn(M11, M22), __fmul_rn(M12, M12));
  c[1] = __fsub_rn(__fmul_rn(M02, M12), __fmul_rn(M01, M22));
  c[2] = __fsub_rn(__fmul_rn(M01, M12), __fmul_rn(M02, M11));
  c[3] = __fsub_rn(__fmul_rn(M00, M22), __fmul_rn(M02, M02));
  c[4] = __fsub_rn(__fmul_rn(M01, M02), __fmul_rn(M00, M12));
  c[5] = __fsub_rn(__fmul_rn(M00, M11), __fmul_rn(M01, M01));
  const float det = __fadd_rn(__fadd_rn(__fmul_rn(M00, c[0]), __fmul_rn(M01, c[1])), __fmul_rn(M02, c[2]));
#pragma unroll
  for (int p = 0; p < 6; ++p) k[p] = __fsub_rn(gf_pi(p) == gf_pj(p) ? 1.f : 0.f, __fmul_rn(eps, __fdiv_rn(c[p], det)));
#pragma unroll
  for (int i = 0; i < 3; ++i)
    k[6 + i] = __fsub_rn(m[i], __fadd_rn(__fadd_rn(__fmul_rn(k[gf_at(i, 0)], m[0]), __fmul_rn(k[gf_at(i, 1)], m[1])), __fmul_rn(k[gf_at(i, 2)], m[2])));
}

// mk: the K coefficient means of a pixel, I: the pixel -> o.  detail == 0 returns q itself, not a blend with weight 0
template <bool VEC>
__device__ __forceinline__ void gf_out(const float* mk, const float I[3], float detail, float o[3]) {
  float Ic[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) Ic[c] = __fsub_rn(I[c], 0.5f);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float q;
    if (VEC) q = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(mk[gf_at(i, 0)], Ic[0]), __fmul_rn(mk[gf_at(i, 1)], Ic[1])), __fmul_rn(mk[gf_at(i, 2)], Ic[2])), mk[6 + i]);
    else q = __fadd_rn(__fmul_rn(mk[i], Ic[i]), mk[3 + i]);
    q = __fadd_rn(q, 0.5f);
    o[i] = detail == 0.f ? q : __fadd_rn(q, __fmul_rn(detail, __fsub_rn(I[i], q)));
  }
}

// ---- the passes on LDS planes ---------------------------------------------------------------------------------------------------
// row sums: dst[row * ds + x] = sum over t = 0 .. r2 of a[row * ss + x + t] (* b[...]), rows [0, nrows), x in [0, ncols), ncols a
// multiple of GFP.  Lanes on consecutive rows.
template <bool PROD>
__device__ __forceinline__ void gf_rows(const float* a, const float* b, int ss, float* dst, int ds, int nrows, int ncols, int r2) {
  const int items = nrows * (ncols / GFP);
  for (int e = threadIdx.x; e < items; e += GFLANES) {
    const int g = e / nrows, row = e - g * nrows, o = row * ss + g * GFP;
    float acc[GFP];
    gf_box<PROD>(a + o, PROD ? b + o : nullptr, 1, r2, acc);
#pragma unroll
    for (int i = 0; i < GFP; ++i) dst[row * ds + g * GFP + i] = acc[i];
  }
}

// column sums: dst[y * ds + x] = sum over t = 0 .. r2 of src[(y + t) * ss + x], y in [0, nrows), nrows a multiple of GFP.  Lanes on
// consecutive columns.
__device__ __forceinline__ void gf_cols(const float* src, int ss, float* dst, int ds, int nrows, int ncols, int r2) {
  const int items = (nrows / GFP) * ncols;
  for (int e = threadIdx.x; e < items; e += GFLANES) {
    const int g = e / ncols, x = e - g * ncols;
    float acc[GFP];
    gf_box<false>(src + g * GFP * ss + x, nullptr, ss, r2, acc);
#pragma unroll
    for (int i = 0; i < GFP; ++i) dst[(g * GFP + i) * ds + x] = acc[i];
  }
}

template <bool VEC> struct gf_k { static constexpr int K = VEC ? 9 : 6; };

// The coefficients of the C x C region whose pixel (0, 0) is picture pixel (cy0, cx0): C a multiple of GFP.  sI: 3 planes of
// (C + 2 r) rows, stride C + 2 r + 1; tmp: (C + 2 r) rows, stride C + 1; pl: K planes of C rows, stride C + 1.  Written to the
// planar frame `gcoef` (inside the picture) or, gcoef == nullptr, left in pl with zeros outside the picture.
template <bool VEC>
__device__ __forceinline__ void gf_coefficients(const float* __restrict__ src, int H, int W, int r, float eps, int cy0, int cx0, int C, float* sI, float* tmp,
                                                float* pl, float* __restrict__ gcoef) {
  constexpr int K = gf_k<VEC>::K;
  const int IN = C + 2 * r, SI = IN + 1, CS = C + 1, NI = IN * SI, NC = C * CS, r2 = 2 * r;
  for (int e = threadIdx.x; e < IN * IN; e += GFLANES) {
    const int ly = e / IN, lx = e - ly * IN, y = cy0 - r + ly, x = cx0 - r + lx;
    float v[3] = {0.f, 0.f, 0.f};
    if (y >= 0 && y < H && x >= 0 && x < W) {
      ld3(src + ((long)y * W + x) * 3, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = __fsub_rn(v[c], 0.5f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) sI[c * NI + ly * SI + lx] = v[c];
  }
  __syncthreads();
  for (int m = 0; m < K; ++m) {
    if (m < 3) gf_rows<false>(sI + m * NI, nullptr, SI, tmp, CS, IN, C, r2);
    else {
      const int i = VEC ? gf_pi(m - 3) : m - 3, j = VEC ? gf_pj(m - 3) : m - 3;
      gf_rows<true>(sI + i * NI, sI + j * NI, SI, tmp, CS, IN, C, r2);
    }
    __syncthreads();
    gf_cols(tmp, CS, pl + m * NC, CS, C, C, r2);
    __syncthreads();
  }
  for (int e = threadIdx.x; e < C * C; e += GFLANES) {
    const int ly = e / C, lx = e - ly * C, y = cy0 + ly, x = cx0 + lx, o = ly * CS + lx;
    float k[K];
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float cnt = gf_count(y, x, H, W, r);
      float m[K];
#pragma unroll
      for (int n = 0; n < K; ++n) m[n] = __fdiv_rn(pl[n * NC + o], cnt);
      gf_solve<VEC>(m, eps, k);
      if (gcoef) {
#pragma unroll
        for (int n = 0; n < K; ++n) gcoef[((long)n * H + y) * W + x] = k[n];
      }
    } else {
#pragma unroll
      for (int n = 0; n < K; ++n) k[n] = 0.f;
    }
    if (!gcoef) {
#pragma unroll
      for (int n = 0; n < K; ++n) pl[n * NC + o] = k[n];
    }
  }
}

// The output tile at (ty0, tx0) from coefficient planes with an r halo: plane n is cp + n * cn, row stride cs, its element (0, 0)
// the coefficient of picture pixel (ty0 - r, tx0 - r); tmp: (GFT + 2 r) rows, stride GFT + 1.  STAGE: the planes are read from the
// planar frame gcoef instead, one at a time through buf ((GFT + 2 r) rows, stride GFT + 2 r + 1).
template <bool VEC, bool STAGE>
__device__ __forceinline__ void gf_apply(const float* __restrict__ src, const float* __restrict__ gcoef, const float* cp, int cn, int cs, float* buf, float* tmp,
                                         float* __restrict__ out, int H, int W, int r, float detail, int ty0, int tx0) {
  constexpr int K = gf_k<VEC>::K;
  const int IN = GFT + 2 * r, TS = GFT + 1, r2 = 2 * r;
  const int lx = threadIdx.x % GFT, gy = threadIdx.x / GFT;
  float S[K][GFP];
#pragma unroll
  for (int n = 0; n < K; ++n) {
    const float* p = cp + n * cn;
    int ss = cs;
    if (STAGE) {
      for (int e = threadIdx.x; e < IN * IN; e += GFLANES) {
        const int by = e / IN, bx = e - by * IN, y = ty0 - r + by, x = tx0 - r + bx;
        buf[by * (IN + 1) + bx] = y >= 0 && y < H && x >= 0 && x < W ? gcoef[((long)n * H + y) * W + x] : 0.f;
      }
      __syncthreads();
      p = buf; ss = IN + 1;
    }
    gf_rows<false>(p, nullptr, ss, tmp, TS, IN, GFT, r2);
    __syncthreads();
    gf_box<false>(tmp + gy * GFP * TS + lx, nullptr, TS, r2, S[n]);
    __syncthreads();                   // tmp (and buf) are rewritten for the next plane
  }
  const int x = tx0 + lx;
  if (x >= W) return;
#pragma unroll
  for (int i = 0; i < GFP; ++i) {
    const int y = ty0 + gy * GFP + i;
    if (y >= H) break;
    const float cnt = gf_count(y, x, H, W, r);
    float mk[K], I[3], o[3];
#pragma unroll
    for (int n = 0; n < K; ++n) mk[n] = __fdiv_rn(S[n][i], cnt);
    const long q = ((long)y * W + x) * 3;
    ld3(src + q, I);
    gf_out<VEC>(mk, I, detail, o);
    st3(out + q, o);
  }
}

// ---- route 1 ----------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(GFLANES) void k_img_gf_coef(const float* __restrict__ src, float* __restrict__ coef, int H, int W, int r, float eps) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int IN = GFT + 2 * r;
  float *sI = lds, *tmp = sI + 3 * IN * (IN + 1), *pl = tmp + IN * (GFT + 1);
  gf_coefficients<VEC>(src, H, W, r, eps, blockIdx.y * GFT, blockIdx.x * GFT, GFT, sI, tmp, pl, coef);
}

template <bool VEC>
__global__ __launch_bounds__(GFLANES) void k_img_gf_apply(const float* __restrict__ src, const float* __restrict__ coef, float* __restrict__ out, int H, int W,
                                                         int r, float detail) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int IN = GFT + 2 * r;
  float *buf = lds, *tmp = buf + IN * (IN + 1);
  gf_apply<VEC, true>(src, coef, nullptr, 0, 0, buf, tmp, out, H, W, r, detail, blockIdx.y * GFT, blockIdx.x * GFT);
}

// ---- route 2 ----------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int gf_fused_c(int r) { return (GFT + 2 * r + GFP - 1) / GFP * GFP; }

template <bool VEC>
__global__ __launch_bounds__(GFLANES) void k_img_gf_fused(const float* __restrict__ src, float* __restrict__ out, int H, int W, int r, float eps, float detail) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int C = gf_fused_c(r), IN = C + 2 * r;
  float *sI = lds, *tmp = sI + 3 * IN * (IN + 1), *pl = tmp + IN * (C + 1);
  const int ty0 = blockIdx.y * GFT, tx0 = blockIdx.x * GFT;
  gf_coefficients<VEC>(src, H, W, r, eps, ty0 - r, tx0 - r, C, sI, tmp, pl, nullptr);
  __syncthreads();
  gf_apply<VEC, false>(src, nullptr, pl, C * (C + 1), C + 1, nullptr, tmp, out, H, W, r, detail, ty0, tx0);
}

constexpr size_t gf_coef_lds(int r, int C, int K) { return sizeof(float) * (size_t)(3 * (C + 2 * r) * (C + 2 * r + 1) + (C + 2 * r) * (C + 1) + K * C * (C + 1)); }
static_assert(gf_coef_lds(ICS_IMG_GUIDED_MAX_RADIUS, GFT, 9) <= 160 * 1024, "route 1 at the largest radius does not fit the LDS");
static_assert(gf_coef_lds(ICS_IMG_GUIDED_FUSED_RADIUS, gf_fused_c(ICS_IMG_GUIDED_FUSED_RADIUS), 9) <= 160 * 1024 &&
              gf_coef_lds(ICS_IMG_GUIDED_FUSED_RADIUS + 1, gf_fused_c(ICS_IMG_GUIDED_FUSED_RADIUS + 1), 9) > 160 * 1024,
              "ICS_IMG_GUIDED_FUSED_RADIUS is not the largest radius whose fused tile fits the LDS");

}  // namespace

// floats of the coefficient frame route 1 needs (route 2: none)
size_t ics_img_guided_coef_floats(int H, int W, int coupling, int route) { return route == 2 ? 0 : (size_t)(coupling ? 9 : 6) * H * W; }

hipError_t ics_launch_img_guided(const float* src, int H, int W, int radius, float eps, float detail, int coupling, int route, float* coef, float* out,
                                 hipStream_t s) {
  if (radius < 1 || radius > ICS_IMG_GUIDED_MAX_RADIUS || (route != 1 && route != 2) || (route == 2 && radius > ICS_IMG_GUIDED_FUSED_RADIUS))
    return hipErrorInvalidValue;
  const int K = coupling ? 9 : 6, r = radius;
  const dim3 grid((W + GFT - 1) / GFT, (H + GFT - 1) / GFT), block(GFLANES);
  if (route == 2) {
    const size_t lds = gf_coef_lds(r, gf_fused_c(r), K);
    hipError_t e = coupling ? set_dynamic_lds(k_img_gf_fused<true>, lds) : set_dynamic_lds(k_img_gf_fused<false>, lds);
    if (e != hipSuccess) return e;
    ICS_LAUNCH_VEC(coupling, k_img_gf_fused, grid, block, lds, s, src, out, H, W, r, eps, detail);
    return hipGetLastError();
  }
  if (!coef) return hipErrorInvalidValue;
  const size_t lds_a = gf_coef_lds(r, GFT, K), lds_b = sizeof(float) * (size_t)((GFT + 2 * r) * (GFT + 2 * r + 1) + (GFT + 2 * r) * (GFT + 1));
  hipError_t e = coupling ? set_dynamic_lds(k_img_gf_coef<true>, lds_a) : set_dynamic_lds(k_img_gf_coef<false>, lds_a);
  if (e == hipSuccess) e = coupling ? set_dynamic_lds(k_img_gf_apply<true>, lds_b) : set_dynamic_lds(k_img_gf_apply<false>, lds_b);
  if (e != hipSuccess) return e;
  ICS_LAUNCH_VEC(coupling, k_img_gf_coef, grid, block, lds_a, s, src, coef, H, W, r, eps);
  ICS_LAUNCH_VEC(coupling, k_img_gf_apply, grid, block, lds_b, s, src, (const float*)coef, out, H, W, r, detail);
  return hipGetLastError();
}
