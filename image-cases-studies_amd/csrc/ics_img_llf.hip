// ics_img_llf.hip -- fast local Laplacian filter of device-resident images (ics_img_local_laplacian, include/ics_hip.h): H x W x 3
// float32, HWC, contiguous.  Paris, Hasinoff and Kautz (2011) in the sampled form of Aubry et al. (2014): K remapped copies of the
// signal, a Gaussian pyramid of each, and an output Laplacian pyramid whose coefficient at (l, p) is interpolated between the two
// copies whose reference values bracket G[l](p).
//
//   signal    coupling 0 (channel): each channel by itself, out_c = R[0] of that channel;
//             coupling 1 (vector):  Y = (0.2126 R + 0.7152 G) + 0.0722 B, out_c = in_c + (Y' - Y), Y' = R[0]                (llf_signal)
//   reduce    size n -> (n + 1) / 2: taps 1 4 6 4 1 at the input indices 2 y - 2 .. 2 y + 2, folded by the symmetric extension (symm of
//             ics_img_px.h), (((a0 + a4) + 2 a2) + 4 a2) + 4 (a1 + a3) along y, then the same along x, then times 1 / 256  (llf_reduce5)
//             The weight 6 is split into 2 + 4: every partial sum of a constant c is then c times a power of two (2 c, 4 c, 8 c,
//             16 c), so a constant is reduced to itself exactly whatever its bits; ((a0 + a4) + 4 (a1 + a3)) + 6 a2 rounds 10 c and 6 c,
//             and a constant picture would come back an ulp off for some arguments.
//   expand    to a given size, indices clamped to the coarse level: position 2 k: (((c[k-1] + c[k+1]) + 2 c[k]) + 4 c[k]) 0.125 (the
//             same split), position 2 k + 1: (c[k] + c[k+1]) 0.5; along y, then along x                                     (llf_expand1)
//   remap     about g, d = i - g:  r_g(i) = g + d (edges + (detail - edges) exp((d d) ninv)), ninv = float32(-1 / (2 sigma^2)) formed in
//             double; detail - edges is one float32 subtraction                                                              (llf_remap)
//   samples   g_k = k / (K - 1) (IEEE division), k = 0 .. K - 1                                                             (llf_sample)
//   pyramids  G[0..J] of the signal, P_k[0..J] of r_{g_k}(signal), L_k[l] = P_k[l] - expand(P_k[l+1])
//   output Laplacian at level l < J, pixel p:  t = clamp(G[l](p) (K - 1), 0, K - 1), k0 = min(floor(t), K - 2), f = t - k0,
//             OL[l](p) = a + f (b - a), a = L_k0[l](p), b = L_{k0+1}[l](p)                                                  (llf_blend)
//   collapse  R[J] = G[J], R[l] = OL[l] + expand(R[l+1]); the filtered signal is R[0]
//
// Every value is computed by these inline functions in one fixed order of operations (no FMA, one expf) by every route, and no value
// depends on where a tile starts, so the routes agree bit for bit and two runs give identical bits.
//
// Planes.  The signal and P_k[0] are never stored: both are recomputed from the source pixel where they are read (the level-0 reduce
// and the level-0 collapse).  `pyr` holds K + 1 pyramids of levels 1 .. J, planar, pyramid 0 the un-remapped G, pyramid 1 + k the
// sample k: (K + 1) n floats, n = the pixels of levels 1 .. J <= H W / 3 + J.  `r0` / `r1` hold R[l] of odd / even l >= 1, at most
// the pixels of level 1 each.  Temporary bytes per pixel at K = 8: 4 (K + 1) / 3 + 2 = 14 for both couplings, "channel" running its
// three channels one after another through the same buffers (three allocations).
//
// A reduce works on 32 x 32 output tiles of 256 lanes: the 67 x 67 inputs the tile needs are staged in LDS (row stride 68), the
// pass along y writes 32 x 67 sums into a scratch plane with the lanes on consecutive columns (one bank each), the pass along x
// reads six neighbours of it as three 8-byte reads with the lanes on consecutive outputs (8 bytes per lane: no conflict) and stores
// a coalesced row.
//
// Route 1, per sample: for every pyramid a chain of J launches; k_img_llf_reduce0 stages llf_remap(llf_signal(source)) directly,
// k_img_llf_reduce goes on from level 1.  LDS of k_img_llf_reduce0 and k_img_llf_reduce: (67 + 32) x 68 floats = 26 928 B.
// Route 2, samples batched: k_img_llf_reduce0_batched stages the signal of its tile once and loops over the K + 1 pyramids,
// remapping from LDS into a second plane; below level 0 one k_img_llf_reduce launch per level has the pyramid as its grid's z.
// LDS: (2 x 67 + 32) x 68 floats = 45 152 B, three workgroups per CU.
// Both routes then run k_img_llf_collapse once per level, coarse to fine: per pixel G[l](p), k0 and f, the two Laplacian coefficients
// from P_k[l] and the 3 x 3 clamped neighbours in P_k[l+1], the blend, plus expand(R[l+1]); at level 0 it reads the source pixel
// instead of G[0] and P_k[0] and writes the result.
//
// Algorithmic bytes per pixel at level 0, vector, K = 8 (levels below add a third): route 1 reads the frame K + 1 times, 9 x 12 = 108,
// and writes K + 1 quarter-size planes, 9; route 2 reads it once, 12 + 9.  The collapse reads 12, writes 12 and reads the three
// quarter-size planes it needs, 3.  Together 144 against 48.  Channel, three passes of 4-byte reads: 3 x (9 x 4 + 9 + 4 + 4 + 3) = 168
// against 3 x (4 + 9 + 4 + 4 + 3) = 72.
#include "ics_img_px.h"

namespace {

#define LLT 32                         // output tile edge of a reduce
#define LLIN 67                        // 2 * LLT + 3: the inputs a tile needs per axis
#define LLS 68                         // row stride of the LDS planes (even: the pass along x reads 8-byte pairs)
#define LLLANES 256

struct LlfParams { float ninv, de, edges, km1; int K; };

// ---- the arithmetic every route shares ------------------------------------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ float llf_signal(const float* __restrict__ src, long px, int ch) {
  if (!VEC) return src[px * 3 + ch];
  float v[3];
  ld3(src + px * 3, v);
  return __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, v[0]), __fmul_rn(0.7152f, v[1])), __fmul_rn(0.0722f, v[2]));
}

__device__ __forceinline__ float llf_sample(int k, float km1) { return __fdiv_rn((float)k, km1); }

__device__ __forceinline__ float llf_remap(float i, float g, const LlfParams& p) {
  const float d = __fsub_rn(i, g);
  const float e = expf(__fmul_rn(__fmul_rn(d, d), p.ninv));
  return __fadd_rn(g, __fmul_rn(d, __fadd_rn(p.edges, __fmul_rn(p.de, e))));
}

__device__ __forceinline__ float llf_reduce5(float a0, float a1, float a2, float a3, float a4) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(a0, a4), __fmul_rn(2.f, a2)), __fmul_rn(4.f, a2)), __fmul_rn(4.f, __fadd_rn(a1, a3)));
}

// one axis of expand at an even (cm, c0, cp = c[k-1], c[k], c[k+1]) or odd (c0, cp = c[k], c[k+1]) position
__device__ __forceinline__ float llf_expand1(float cm, float c0, float cp, bool odd) {
  if (odd) return __fmul_rn(__fadd_rn(c0, cp), 0.5f);
  return __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(cm, cp), __fmul_rn(2.f, c0)), __fmul_rn(4.f, c0)), 0.125f);
}

// expand(c)(y, x) of the hc x wc plane c: along y on the three clamped columns, then along x
__device__ __forceinline__ float llf_expand(const float* __restrict__ c, int hc, int wc, int y, int x) {
  const int ky = y >> 1, kx = x >> 1;
  const bool oy = y & 1, ox = x & 1;
  const int ym = max(ky - 1, 0), yp = min(ky + 1, hc - 1);
  const int xs[3] = {max(kx - 1, 0), kx, min(kx + 1, wc - 1)};
  float col[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) col[j] = llf_expand1(c[ym * wc + xs[j]], c[ky * wc + xs[j]], c[yp * wc + xs[j]], oy);
  return llf_expand1(col[0], col[1], col[2], ox);
}

// k0 and f of a pixel whose un-remapped value is g
__device__ __forceinline__ int llf_bracket(float g, const LlfParams& p, float* f) {
  const float t = fminf(fmaxf(__fmul_rn(g, p.km1), 0.f), p.km1);
  const int k0 = min((int)floorf(t), p.K - 2);
  *f = __fsub_rn(t, (float)k0);
  return k0;
}

__device__ __forceinline__ float llf_blend(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }

// ---- a reduce on LDS planes -------------------------------------------------------------------------------------------------------
// in: LLIN rows of stride LLS, its element (0, 0) the (folded) input (2 oy0 - 2, 2 ox0 - 2); tmp: LLT rows of stride LLS; the tile's
// outputs inside ho x wo go to dst.  Two barriers; the caller has one between its writes of `in` and this.
__device__ __forceinline__ void llf_reduce_tile(const float* in, float* tmp, float* __restrict__ dst, int ho, int wo, int oy0, int ox0) {
  for (int e = threadIdx.x; e < LLT * LLIN; e += LLLANES) {
    const int oy = e / LLIN, ix = e - oy * LLIN;
    const float* a = in + 2 * oy * LLS + ix;
    tmp[oy * LLS + ix] = llf_reduce5(a[0], a[LLS], a[2 * LLS], a[3 * LLS], a[4 * LLS]);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < LLT * LLT; e += LLLANES) {
    const int oy = e / LLT, ox = e - oy * LLT;
    const float2* t = reinterpret_cast<const float2*>(tmp + oy * LLS + 2 * ox);
    const float2 t01 = t[0], t23 = t[1], t45 = t[2];      // (t45.y is the next output's, or the pad column: unused)
    const float v = __fmul_rn(llf_reduce5(t01.x, t01.y, t23.x, t23.y, t45.x), 1.f / 256.f);
    if (oy0 + oy < ho && ox0 + ox < wo) dst[(oy0 + oy) * wo + ox0 + ox] = v;
  }
  __syncthreads();
}

// level 0 -> 1 of one pyramid: kk = 0 the un-remapped signal, kk = 1 + k the sample k
template <bool VEC>
__global__ __launch_bounds__(LLLANES) void k_img_llf_reduce0(const float* __restrict__ src, int ch, float* __restrict__ pyr, long ps, int kk, int H, int W,
                                                              LlfParams p) {
  __shared__ __attribute__((aligned(16))) float in[LLIN * LLS];
  __shared__ __attribute__((aligned(16))) float tmp[LLT * LLS];
  const int oy0 = blockIdx.y * LLT, ox0 = blockIdx.x * LLT;
  const float g = llf_sample(kk - 1, p.km1);
  for (int e = threadIdx.x; e < LLIN * LLIN; e += LLLANES) {
    const int ly = e / LLIN, lx = e - ly * LLIN;
    const float v = llf_signal<VEC>(src, (long)symm(2 * oy0 - 2 + ly, H) * W + symm(2 * ox0 - 2 + lx, W), ch);
    in[ly * LLS + lx] = kk ? llf_remap(v, g, p) : v;
  }
  __syncthreads();
  llf_reduce_tile(in, tmp, pyr + kk * ps, (H + 1) / 2, (W + 1) / 2, oy0, ox0);
}

// level 0 -> 1 of all K + 1 pyramids: the signal of the tile is read once
template <bool VEC>
__global__ __launch_bounds__(LLLANES) void k_img_llf_reduce0_batched(const float* __restrict__ src, int ch, float* __restrict__ pyr, long ps, int H, int W,
                                                                      LlfParams p) {
  __shared__ __attribute__((aligned(16))) float sig[LLIN * LLS];
  __shared__ __attribute__((aligned(16))) float in[LLIN * LLS];
  __shared__ __attribute__((aligned(16))) float tmp[LLT * LLS];
  const int oy0 = blockIdx.y * LLT, ox0 = blockIdx.x * LLT;
  for (int e = threadIdx.x; e < LLIN * LLIN; e += LLLANES) {
    const int ly = e / LLIN, lx = e - ly * LLIN;
    sig[ly * LLS + lx] = llf_signal<VEC>(src, (long)symm(2 * oy0 - 2 + ly, H) * W + symm(2 * ox0 - 2 + lx, W), ch);
  }
  __syncthreads();
  llf_reduce_tile(sig, tmp, pyr, (H + 1) / 2, (W + 1) / 2, oy0, ox0);
  for (int k = 0; k < p.K; ++k) {
    const float g = llf_sample(k, p.km1);
    for (int e = threadIdx.x; e < LLIN * LLIN; e += LLLANES) {
      const int o = e / LLIN * LLS + e % LLIN;
      in[o] = llf_remap(sig[o], g, p);
    }
    __syncthreads();
    llf_reduce_tile(in, tmp, pyr + (1 + k) * ps, (H + 1) / 2, (W + 1) / 2, oy0, ox0);
  }
}

// level l -> l + 1, l >= 1, of the pyramids kk0 + blockIdx.z: src_off / dst_off are the levels' offsets inside a pyramid
__global__ __launch_bounds__(LLLANES) void k_img_llf_reduce(float* __restrict__ pyr, long ps, int kk0, long src_off, long dst_off, int h, int w) {
  __shared__ __attribute__((aligned(16))) float in[LLIN * LLS];
  __shared__ __attribute__((aligned(16))) float tmp[LLT * LLS];
  const int oy0 = blockIdx.y * LLT, ox0 = blockIdx.x * LLT;
  float* base = pyr + (kk0 + (long)blockIdx.z) * ps;
  const float* s = base + src_off;
  for (int e = threadIdx.x; e < LLIN * LLIN; e += LLLANES) {
    const int ly = e / LLIN, lx = e - ly * LLIN;
    in[ly * LLS + lx] = s[symm(2 * oy0 - 2 + ly, h) * w + symm(2 * ox0 - 2 + lx, w)];
  }
  __syncthreads();
  llf_reduce_tile(in, tmp, base + dst_off, (h + 1) / 2, (w + 1) / 2, oy0, ox0);
}

// R[l] = OL[l] + expand(R[l+1]) on the h x w level l; the coarse level is hc x wc at off_c inside a pyramid, level l (l >= 1) at
// off_l.  L0: level 0, G[0] and P_k[0] come from the source pixel and the result goes to the H x W x 3 frame `out`.
template <bool VEC, bool L0>
__global__ __launch_bounds__(LLLANES) void k_img_llf_collapse(const float* __restrict__ src, int ch, const float* __restrict__ pyr, long ps, long off_l,
                                                               long off_c, const float* __restrict__ rin, float* __restrict__ rout, int h, int w, int hc,
                                                               int wc, LlfParams p) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const long px = (long)y * w + x;
  const float g = L0 ? llf_signal<VEC>(src, px, ch) : pyr[off_l + px];
  float f;
  const int k0 = llf_bracket(g, p, &f);
  float lap[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float* pk = pyr + (1 + k0 + i) * ps;
    const float fine = L0 ? llf_remap(g, llf_sample(k0 + i, p.km1), p) : pk[off_l + px];
    lap[i] = __fsub_rn(fine, llf_expand(pk + off_c, hc, wc, y, x));
  }
  const float r = __fadd_rn(llf_blend(lap[0], lap[1], f), llf_expand(rin, hc, wc, y, x));
  if (!L0) { rout[px] = r; return; }
  if (!VEC) { rout[px * 3 + ch] = r; return; }
  float v[3];
  ld3(src + px * 3, v);
  const float dy = __fsub_rn(r, g);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(v[c], dy);
  st3(rout + px * 3, v);
}

// pixels of levels 1 .. J of an H x W picture; off[l] (l = 1 .. J): the level's offset inside a pyramid
size_t llf_levels(int H, int W, int J, long* off, int* hs, int* ws) {
  size_t n = 0;
  int h = H, w = W;
  hs[0] = H; ws[0] = W;
  for (int l = 1; l <= J; ++l) {
    h = (h + 1) / 2; w = (w + 1) / 2;
    hs[l] = h; ws[l] = w;
    off[l] = (long)n;
    n += (size_t)h * w;
  }
  return n;
}

}  // namespace

size_t ics_img_llf_pyramid_floats(int H, int W, int levels, int samples) {
  long off[ICS_IMG_LLF_MAX_LEVELS + 1];
  int hs[ICS_IMG_LLF_MAX_LEVELS + 1], ws[ICS_IMG_LLF_MAX_LEVELS + 1];
  return (size_t)(samples + 1) * llf_levels(H, W, levels, off, hs, ws);
}
size_t ics_img_llf_collapse_floats(int H, int W) { return (size_t)((H + 1) / 2) * ((W + 1) / 2); }

hipError_t ics_launch_img_llf(const float* src, int H, int W, float sigma, float detail, float edges, int levels, int samples, int coupling, int route,
                              float* pyr, float* r0, float* r1, float* out, hipStream_t s) {
  if (levels < 1 || levels > ICS_IMG_LLF_MAX_LEVELS || samples < 2 || samples > ICS_IMG_LLF_MAX_SAMPLES || (route != 1 && route != 2) || !pyr || !r0 || !r1)
    return hipErrorInvalidValue;
  const int J = levels, K = samples;
  long off[ICS_IMG_LLF_MAX_LEVELS + 1];
  int hs[ICS_IMG_LLF_MAX_LEVELS + 1], ws[ICS_IMG_LLF_MAX_LEVELS + 1];
  const long ps = (long)llf_levels(H, W, J, off, hs, ws);
  const LlfParams p = {(float)(-1.0 / (2.0 * (double)sigma * (double)sigma)), detail - edges, edges, (float)(K - 1), K};
  const dim3 block(LLLANES);
  auto tiles = [](int h, int w, int z) { return dim3((w + LLT - 1) / LLT, (h + LLT - 1) / LLT, z); };
  for (int ch = 0; ch < (coupling ? 1 : 3); ++ch) {
    if (route == 2) {
      ICS_LAUNCH_VEC(coupling, k_img_llf_reduce0_batched, tiles(hs[1], ws[1], 1), block, 0, s, src, ch, pyr, ps, H, W, p);
      for (int l = 1; l < J; ++l)
        hipLaunchKernelGGL(k_img_llf_reduce, tiles(hs[l + 1], ws[l + 1], K + 1), block, 0, s, pyr, ps, 0, off[l], off[l + 1], hs[l], ws[l]);
    } else {
      for (int kk = 0; kk <= K; ++kk) {
        ICS_LAUNCH_VEC(coupling, k_img_llf_reduce0, tiles(hs[1], ws[1], 1), block, 0, s, src, ch, pyr, ps, kk, H, W, p);
        for (int l = 1; l < J; ++l)
          hipLaunchKernelGGL(k_img_llf_reduce, tiles(hs[l + 1], ws[l + 1], 1), block, 0, s, pyr, ps, kk, off[l], off[l + 1], hs[l], ws[l]);
      }
    }
    const float* rin = pyr + off[J];                     // R[J] = G[J]
    for (int l = J - 1; l >= 0; --l) {
      float* rout = l == 0 ? out : (l & 1 ? r0 : r1);
      const dim3 grid((ws[l] + 63) / 64, (hs[l] + 3) / 4);
      if (l == 0) {
        if (coupling) hipLaunchKernelGGL((k_img_llf_collapse<true, true>), grid, block, 0, s, src, ch, (const float*)pyr, ps, 0L, off[1], rin, rout, H, W, hs[1], ws[1], p);
        else hipLaunchKernelGGL((k_img_llf_collapse<false, true>), grid, block, 0, s, src, ch, (const float*)pyr, ps, 0L, off[1], rin, rout, H, W, hs[1], ws[1], p);
      } else {
        hipLaunchKernelGGL((k_img_llf_collapse<false, false>), grid, block, 0, s, src, ch, (const float*)pyr, ps, off[l], off[l + 1], rin, rout, hs[l], ws[l],
                           hs[l + 1], ws[l + 1], p);
      }
      rin = rout;
    }
  }
  return hipGetLastError();
}
