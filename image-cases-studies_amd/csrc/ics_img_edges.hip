// ics_img_edges.hip -- edge prediction on device-resident images (ics_img_shock, ics_img_edge_mask, include/ics_hip.h): H x W x 3 float32,
// HWC, contiguous.  The two halves of Cho and Lee's prediction step: a shock filter that turns the ramps of a blurred frame into steps,
// and the choice of the gradients worth trusting, the same number for every orientation.  Restated in tests/edges_ref.py; no FMA, IEEE
// square roots: the float32 evaluation of that file is the result of every route here bit for bit.
//
// ---- shock filter, one step (Osher and Rudin).  Every plane below exists on the picture only, and every read of a neighbour goes through
// coordinates clamped to the picture (the edge repeated, in each plane on its own):
//   Y        = ((R + G) + B) * float32(1 / 3)                                  "vector"; "channel": Y = the channel itself, three times
//   Ys       = V(H(Y)), H(a)[x] = ((a[x-1] + a[x+1]) + (a[x] + a[x])) * 0.25 along x, V the same along y
//   L        = ((Ys[x-1] + Ys[x+1]) + (Ys[y-1] + Ys[y+1])) - 4 Ys
//   s        = min(max(L * float32(1 / flat), -1), 1)                          a steer that is continuous in L
//   a, b     = u - u[x-1], u[x+1] - u;  c, d = u - u[y-1], u[y+1] - u          per channel u
//   m(p, q)  = p * q > 0 ? copysign(min(|p|, |q|), p) : 0
//   g        = sqrt(m(a, b)^2 + m(c, d)^2)
//   out      = u - (dt * s) * g
// Route 1 (k_img_ed_shock): one launch per step, a lane per pixel, the five Ys it needs each from its own nine clamped reads of the
// frame; two frames ping-pong.  12 B read (the neighbourhood comes from the caches) + 12 B written per pixel and step.
// Route 2 (k_img_ed_shock_block): up to EDT steps per launch on a 32 x 32 output tile in LDS.  A step consumes two pixels of halo (one
// for the differences, two for the Laplacian of the smoothed plane), so a workgroup stages (32 + 4 EDT)^2 = 48^2 pixels as planes of
// stride 48 (consecutive lanes on consecutive banks along a row): the three channels twice (the step reads one set and writes the other),
// Y and Ys, 8 floats per pixel, 48^2 x 32 B = 73 728 B, two workgroups of 512 lanes per CU.  Step t computes Y on the staged square less
// 2 t - 2 pixels per side, Ys on it less 2 t - 1, the channels less 2 t: the exact region ends on the output tile.  A neighbour is read
// at the tile coordinate of the clamped picture coordinate, positions outside the picture are neither written nor read: what route 1
// sees.  (12 x (48 / 32)^2 = 27 B read + 12 B written per pixel and launch.)  A remainder of iterations % EDT steps is the last launch.
//
// ---- gradient selection:
//   gx, gy   = u[x+1] - u, u[y+1] - u per channel, 0 in the last column / row
//   "vector": g = sqrt((q0 + q1) + q2), q_c = gx_c^2 + gy_c^2; sx = (gx0 + gx1) + gx2, sy likewise.  "channel": g = sqrt(q_c), sx = gx_c,
//            sy = gy_c, three independent selections
//   sector   none if not g > 0; 0 if |sy| <= T |sx|; 2 if |sx| <= T |sy|; else 1 if sx * sy > 0, else 3          T = 0.41421357f
//   t_b      = the per_sector-th largest g of sector b (its smallest where it holds fewer); t = min over the sectors that hold any;
//   mask     = g >= t; kept = the pixels of the mask
// An exact radix select over the 31 bits of g below the sign, in three passes of 11 + 10 + 10 bits as in ics_img_noise.hip, for the
// 4 ("vector") or 12 ("channel") populations at once: a pass counts, per population, the keys whose higher bits equal the prefix found
// so far; k_img_ed_select (one workgroup) turns the first pass's totals into ranks from below (n_b - per_sector, or 0), finds the bin
// of each rank, and after the last pass takes the minimum.  Prefixes, ranks, thresholds and counts live in a state block behind the
// histograms; only integer counts are added, so the order in which atomics arrive changes nothing.  A workgroup's histogram is in LDS,
// 2048 bins x 4 B per population taken at launch: 32 KB "vector", 96 KB "channel".
// Route 1 (k_img_ed_recompute x 3, k_img_ed_mask): every pass forms g and the sector from the frame.
// Route 2 (k_img_ed_keys, k_img_ed_hist x 2, k_img_ed_mask_keys): the first pass stores the keys (4 B per pixel and population set)
// and the sectors (in the byte plane that becomes the mask); the later passes read those.
//
// ---- the pair solve under a mask (ics_img_psf_estimate_masked): k_img_ed_rows is k_img_pe_rows of ics_img_psfest.hip with the sharp
// frame's derivative multiplied by mask[y][x] (0 or 1) before the taper, so that the energy S is summed over what remains; the blurred
// frame is untouched.  Same sums in the same order: an all-ones mask gives the bits of the unmasked solve.  Everything after the rows is
// ics_img_psfest.hip's (ics_launch_img_psf_estimate_rows).
#include "ics_img_px.h"
#include "ics_wn_fft.h"

namespace {

#define EDB 32                          // output tile edge of the blocked shock route
#define EDT ICS_IMG_SHOCK_BLOCK         // steps per launch
#define EDS (EDB + 4 * EDT)             // staged tile edge: 48
#define EDN (EDS * EDS)
#define EDSL 512                        // lanes of k_img_ed_shock_block

#define EDB0 11                         // bits of the first select pass
#define EDB1 10                         // ... of the second and third
#define EDBINS (1 << EDB0)
#define EDLANES 256
#define EDPOP 12                        // populations at most: 3 channels x 4 sectors
#define EDSTATE (EDPOP * EDBINS)        // the state block behind the histograms: prefix[12], rank[12], threshold bits[3], kept[3]
#define EDRANK (EDSTATE + EDPOP)
#define EDTHR (EDSTATE + 2 * EDPOP)
#define EDKEPT (EDTHR + 3)
#define EDEMPTY 0xFFFFFFFFu             // rank of a population without keys; threshold of a channel without populations
#define EDHK 4                          // keys per lane and step of the key passes

static_assert(EDB0 + 2 * EDB1 == 31 && EDB1 <= EDB0 && EDBINS % EDLANES == 0 && (1 << EDB1) % EDLANES == 0 && EDS == 48 && EDT >= 1, "layout");

__device__ __forceinline__ int ed_clamp(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }
__device__ __forceinline__ float ed_b121(float l, float c, float r) { return __fmul_rn(__fadd_rn(__fadd_rn(l, r), __fadd_rn(c, c)), 0.25f); }
__device__ __forceinline__ float ed_steer(float l, float r, float u, float d, float c, float inv_flat) {
  const float lap = __fsub_rn(__fadd_rn(__fadd_rn(l, r), __fadd_rn(u, d)), __fmul_rn(4.f, c));
  return fminf(fmaxf(__fmul_rn(lap, inv_flat), -1.f), 1.f);
}
__device__ __forceinline__ float ed_minmod(float p, float q) { return __fmul_rn(p, q) > 0.f ? copysignf(fminf(fabsf(p), fabsf(q)), p) : 0.f; }
// one channel of one pixel: v with its four neighbours, ds = dt * s
__device__ __forceinline__ float ed_step(float v, float l, float r, float u, float d, float ds) {
  const float mx = ed_minmod(__fsub_rn(v, l), __fsub_rn(r, v)), my = ed_minmod(__fsub_rn(v, u), __fsub_rn(d, v));
  const float g = sqrtf(__fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my)));     // (sqrtf: correctly rounded, see ics_img_noise.hip)
  return __fsub_rn(v, __fmul_rn(ds, g));
}

// ---- shock, route 1 ------------------------------------------------------------------------------------------------------------------
// Ys at the picture position (y, x): "vector" ys[0], "channel" ys[0 .. 2]
template <bool VEC>
__device__ __forceinline__ void ed_ys_at(const float* __restrict__ f, int H, int W, int y, int x, float ys[3]) {
  const int yy[3] = {ed_clamp(y - 1, 0, H - 1), y, ed_clamp(y + 1, 0, H - 1)}, xx[3] = {ed_clamp(x - 1, 0, W - 1), x, ed_clamp(x + 1, 0, W - 1)};
  float h[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float* row = f + (long)yy[r] * 3L * W;
    float a[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ld3(row + 3L * xx[k], a[k]);
    if (VEC) h[r][0] = ed_b121(px_luma(a[0]), px_luma(a[1]), px_luma(a[2]));
    else {
#pragma unroll
      for (int c = 0; c < 3; ++c) h[r][c] = ed_b121(a[0][c], a[1][c], a[2][c]);
    }
  }
#pragma unroll
  for (int c = 0; c < (VEC ? 1 : 3); ++c) ys[c] = ed_b121(h[0][c], h[1][c], h[2][c]);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_img_ed_shock(const float* __restrict__ in, float* __restrict__ out, int H, int W, float dt, float inv_flat) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int xl = ed_clamp(x - 1, 0, W - 1), xr = ed_clamp(x + 1, 0, W - 1), yu = ed_clamp(y - 1, 0, H - 1), yd = ed_clamp(y + 1, 0, H - 1);
  const long L = 3L * W;
  float v[3], l[3], r[3], u[3], d[3], sc[3], sl[3], sr[3], su[3], sd[3], o[3];
  ld3(in + y * L + 3L * x, v); ld3(in + y * L + 3L * xl, l); ld3(in + y * L + 3L * xr, r); ld3(in + yu * L + 3L * x, u); ld3(in + yd * L + 3L * x, d);
  ed_ys_at<VEC>(in, H, W, y, x, sc); ed_ys_at<VEC>(in, H, W, y, xl, sl); ed_ys_at<VEC>(in, H, W, y, xr, sr);
  ed_ys_at<VEC>(in, H, W, yu, x, su); ed_ys_at<VEC>(in, H, W, yd, x, sd);
  float ds = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!VEC || c == 0) ds = __fmul_rn(dt, ed_steer(sl[c], sr[c], su[c], sd[c], sc[c], inv_flat));
    o[c] = ed_step(v[c], l[c], r[c], u[c], d[c], ds);
  }
  st3(out + y * L + 3L * x, o);
}

// ---- shock, route 2: n <= EDT steps on an LDS tile -------------------------------------------------------------------------------------
// the positions [lo, lo + m)^2 of the staged tile, a lane each; false where the position lies outside the picture
struct EdPos { int i, il, ir, iu, id; };
__device__ __forceinline__ bool ed_pos(int e, int lo, int m, float inv_m, int y0, int x0, int H, int W, EdPos& p) {
  const int r = (int)(((float)e + 0.5f) * inv_m), ly = lo + r, lx = lo + (e - r * m), y = y0 + ly, x = x0 + lx;
  if (y < 0 || y >= H || x < 0 || x >= W) return false;
  p.i = ly * EDS + lx;
  p.il = ly * EDS + ed_clamp(x - 1, 0, W - 1) - x0; p.ir = ly * EDS + ed_clamp(x + 1, 0, W - 1) - x0;
  p.iu = (ed_clamp(y - 1, 0, H - 1) - y0) * EDS + lx; p.id = (ed_clamp(y + 1, 0, H - 1) - y0) * EDS + lx;
  return true;
}

template <bool VEC>
__global__ __launch_bounds__(EDSL) void k_img_ed_shock_block(const float* __restrict__ in, float* __restrict__ out, int H, int W, int n, float dt,
                                                            float inv_flat) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *cur = lds, *nxt = lds + 3 * EDN, *sy = lds + 6 * EDN, *ss = lds + 7 * EDN;     // planes [c][EDS][EDS] twice, Y, Ys
  const int y0 = blockIdx.y * EDB - 2 * EDT, x0 = blockIdx.x * EDB - 2 * EDT;           // picture coordinates of tile position (0, 0)
  const long L = 3L * W;
  for (int e = threadIdx.x; e < EDN; e += EDSL) {
    const int ly = e / EDS, lx = e - ly * EDS, y = y0 + ly, x = x0 + lx;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;
    float v[3];
    ld3(in + (long)y * L + 3L * x, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) cur[c * EDN + e] = v[c];
  }
  __syncthreads();
  for (int t = EDT - n + 1; t <= EDT; ++t) {
    const int mo = EDS - 4 * t, ms = mo + 2, my = mo + 4;                                // the channels, Ys, Y: edge of the exact square
    const float inv_mo = 1.f / (float)mo, inv_ms = 1.f / (float)ms, inv_my = 1.f / (float)my;
    EdPos p;
    if (VEC) {
      for (int e = threadIdx.x; e < my * my; e += EDSL) {
        if (!ed_pos(e, 2 * t - 2, my, inv_my, y0, x0, H, W, p)) continue;
        const float v[3] = {cur[p.i], cur[EDN + p.i], cur[2 * EDN + p.i]};
        sy[p.i] = px_luma(v);
      }
      __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < (VEC ? 1 : 3); ++c) {
      const float* Y = VEC ? sy : cur + c * EDN;
      for (int e = threadIdx.x; e < ms * ms; e += EDSL) {
        if (!ed_pos(e, 2 * t - 1, ms, inv_ms, y0, x0, H, W, p)) continue;
        const int dl = p.il - p.i, dr = p.ir - p.i;
        ss[p.i] = ed_b121(ed_b121(Y[p.iu + dl], Y[p.iu], Y[p.iu + dr]), ed_b121(Y[p.il], Y[p.i], Y[p.ir]), ed_b121(Y[p.id + dl], Y[p.id], Y[p.id + dr]));
      }
      __syncthreads();
      for (int e = threadIdx.x; e < mo * mo; e += EDSL) {
        if (!ed_pos(e, 2 * t, mo, inv_mo, y0, x0, H, W, p)) continue;
        const float ds = __fmul_rn(dt, ed_steer(ss[p.il], ss[p.ir], ss[p.iu], ss[p.id], ss[p.i], inv_flat));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (!VEC && k != c) continue;
          const float* u = cur + k * EDN;
          nxt[k * EDN + p.i] = ed_step(u[p.i], u[p.il], u[p.ir], u[p.iu], u[p.id], ds);
        }
      }
      __syncthreads();
    }
    float* sw = cur; cur = nxt; nxt = sw;
  }
  for (int e = threadIdx.x; e < EDB * EDB; e += EDSL) {
    const int ly = 2 * EDT + e / EDB, lx = 2 * EDT + e % EDB, i = ly * EDS + lx, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const float v[3] = {cur[i], cur[EDN + i], cur[2 * EDN + i]};
    st3(out + (long)y * L + 3L * x, v);
  }
}

// ---- gradient selection ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ed_sector(float g, float sx, float sy) {
  if (!(g > 0.f)) return 4u;
  const float ax = fabsf(sx), ay = fabsf(sy);
  if (ay <= __fmul_rn(0.41421357f, ax)) return 0u;
  if (ax <= __fmul_rn(0.41421357f, ay)) return 2u;
  return __fmul_rn(sx, sy) > 0.f ? 1u : 3u;
}

// keys (the bits of g) and sectors of the pixel (y, x): one ("vector") or three ("channel")
template <bool VEC>
__device__ __forceinline__ void ed_grad(const float* __restrict__ f, int H, int W, int y, int x, unsigned key[3], unsigned sec[3]) {
  const long L = 3L * W, p = (long)y * L + 3L * x;
  float v[3], r[3], d[3], gx[3], gy[3], q[3];
  ld3(f + p, v);
  if (x + 1 < W) ld3(f + p + 3, r);
  if (y + 1 < H) ld3(f + p + L, d);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gx[c] = x + 1 < W ? __fsub_rn(r[c], v[c]) : 0.f;
    gy[c] = y + 1 < H ? __fsub_rn(d[c], v[c]) : 0.f;
    q[c] = __fadd_rn(__fmul_rn(gx[c], gx[c]), __fmul_rn(gy[c], gy[c]));
  }
  if (VEC) {
    const float g = sqrtf(__fadd_rn(__fadd_rn(q[0], q[1]), q[2]));
    key[0] = __float_as_uint(g);
    sec[0] = ed_sector(g, __fadd_rn(__fadd_rn(gx[0], gx[1]), gx[2]), __fadd_rn(__fadd_rn(gy[0], gy[1]), gy[2]));
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float g = sqrtf(q[c]);
      key[c] = __float_as_uint(g);
      sec[c] = ed_sector(g, gx[c], gy[c]);
    }
  }
}

// one key into the LDS histograms h[npop][EDBINS] if `on`, it has a sector, and its bits above the field equal its population's prefix.
// Called by all lanes of a wave together; a wave whose counted lanes all meet one counter adds its lane count once.
__device__ __forceinline__ void ed_count(unsigned* h, const unsigned* prefix, int chan, unsigned key, unsigned sec, bool on, int shift, int bits) {
  const unsigned pop = 4u * chan + (sec & 3u);
  on = on && sec < 4u && (key >> (shift + bits)) == prefix[pop];
  const unsigned idx = pop * EDBINS + ((key >> shift) & ((1u << bits) - 1u));
  const unsigned long long act = __ballot(on);
  if (!act) return;
  const int lane = threadIdx.x & 63, first = __ffsll((long long)act) - 1;
  const unsigned i0 = __shfl(idx, first);
  if (__ballot(on && idx == i0) == act) {
    if (lane == first) atomicAdd(&h[i0], (unsigned)__popcll(act));
  } else if (on) {
    atomicAdd(&h[idx], 1u);
  }
}

// the start of a counting kernel: the histogram zeroed, the prefixes in LDS
__device__ __forceinline__ void ed_begin(unsigned* h, unsigned* prefix, const unsigned* blk, int npop) {
  for (int i = threadIdx.x; i < npop * EDBINS; i += EDLANES) h[i] = 0u;
  if (threadIdx.x < EDPOP) prefix[threadIdx.x] = blk ? blk[EDSTATE + threadIdx.x] : 0u;
  __syncthreads();
}
// ... and its end: the workgroup's non-empty bins into the global histograms
__device__ __forceinline__ void ed_merge(const unsigned* h, unsigned* blk, int npop) {
  __syncthreads();
  for (int i = threadIdx.x; i < npop * EDBINS; i += EDLANES)
    if (const unsigned v = h[i]) atomicAdd(&blk[i], v);
}

// route 1, every pass
template <bool VEC>
__global__ __launch_bounds__(EDLANES) void k_img_ed_recompute(const float* __restrict__ f, int H, int W, int shift, int bits, unsigned* __restrict__ blk) {
  constexpr int NCH = VEC ? 1 : 3;
  extern __shared__ __attribute__((aligned(16))) unsigned edh[];
  __shared__ unsigned prefix[EDPOP];
  ed_begin(edh, prefix, blk, 4 * NCH);
  const int tx = (W + 63) / 64, tiles = tx * ((H + 3) / 4);
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t / tx, x = (t - ty * tx) * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
    const bool on = x < W && y < H;
    unsigned key[3] = {0u, 0u, 0u}, sec[3] = {4u, 4u, 4u};
    if (on) ed_grad<VEC>(f, H, W, y, x, key, sec);
#pragma unroll
    for (int c = 0; c < NCH; ++c) ed_count(edh, prefix, c, key[c], sec[c], on, shift, bits);
  }
  ed_merge(edh, blk, 4 * NCH);
}

// route 2, first pass: keys[NCH][H W] and sectors secs[NCH][H W] written, the keys counted by their top EDB0 bits
template <bool VEC>
__global__ __launch_bounds__(EDLANES) void k_img_ed_keys(const float* __restrict__ f, int H, int W, unsigned* __restrict__ keys,
                                                        unsigned char* __restrict__ secs, unsigned* __restrict__ blk) {
  constexpr int NCH = VEC ? 1 : 3;
  extern __shared__ __attribute__((aligned(16))) unsigned edh[];
  __shared__ unsigned prefix[EDPOP];
  ed_begin(edh, prefix, nullptr, 4 * NCH);
  const int tx = (W + 63) / 64, tiles = tx * ((H + 3) / 4);
  const long n = (long)H * W;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t / tx, x = (t - ty * tx) * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
    const bool on = x < W && y < H;
    unsigned key[3] = {0u, 0u, 0u}, sec[3] = {4u, 4u, 4u};
    if (on) ed_grad<VEC>(f, H, W, y, x, key, sec);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (on) { keys[c * n + (long)y * W + x] = key[c]; secs[c * n + (long)y * W + x] = (unsigned char)sec[c]; }
      ed_count(edh, prefix, c, key[c], sec[c], on, 31 - EDB0, EDB0);
    }
  }
  ed_merge(edh, blk, 4 * NCH);
}

// route 2, later passes: the stored keys and sectors, EDHK per lane and step
template <bool VEC>
__global__ __launch_bounds__(EDLANES) void k_img_ed_hist(const unsigned* __restrict__ keys, const unsigned char* __restrict__ secs, long n, int shift,
                                                        unsigned* __restrict__ blk) {
  constexpr int NCH = VEC ? 1 : 3;
  extern __shared__ __attribute__((aligned(16))) unsigned edh[];
  __shared__ unsigned prefix[EDPOP];
  ed_begin(edh, prefix, blk, 4 * NCH);
  for (long i0 = (long)blockIdx.x * (EDLANES * EDHK); i0 < n; i0 += (long)gridDim.x * (EDLANES * EDHK)) {
    unsigned key[EDHK][NCH], sec[EDHK][NCH];
#pragma unroll
    for (int k = 0; k < EDHK; ++k) {
      const long i = i0 + k * EDLANES + threadIdx.x;
#pragma unroll
      for (int c = 0; c < NCH; ++c) { key[k][c] = i < n ? keys[c * n + i] : 0u; sec[k][c] = i < n ? secs[c * n + i] : 4u; }
    }
#pragma unroll
    for (int k = 0; k < EDHK; ++k) {
      const bool on = i0 + k * EDLANES + threadIdx.x < n;
#pragma unroll
      for (int c = 0; c < NCH; ++c) ed_count(edh, prefix, c, key[k][c], sec[k][c], on, shift, EDB1);
    }
  }
  ed_merge(edh, blk, 4 * NCH);
}

// between the passes, one workgroup: per population, the bin that holds the rank joins the prefix and the rank drops by the count below
// the bin; the histogram is left zeroed.  first: the rank is set from the population's size, n - k from below, 0 where it holds no
// more than k keys, EDEMPTY where it holds none.  last: the thresholds, the smallest prefix among each channel's populations that
// hold keys (non-negative floats order like their bits), EDEMPTY where none does.
__global__ __launch_bounds__(EDLANES) void k_img_ed_select(unsigned* __restrict__ blk, int npop, int bits, unsigned k, int first, int last) {
  __shared__ unsigned wsum[EDLANES / 64];
  const int per = (1 << bits) / EDLANES, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;        // 8 or 4 bins per lane
  for (int p = 0; p < npop; ++p) {
    unsigned* g = blk + p * EDBINS + threadIdx.x * per;
    unsigned rank = first ? 0u : blk[EDRANK + p];
    const unsigned prefix = first ? 0u : blk[EDSTATE + p];
    unsigned v[EDBINS / EDLANES], s = 0u;
#pragma unroll
    for (int i = 0; i < EDBINS / EDLANES; ++i) {
      v[i] = 0u;
      if (i < per) { v[i] = g[i]; g[i] = 0u; }
      s += v[i];
    }
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned below = incl - s, total = 0u;
    for (int w = 0; w < EDLANES / 64; ++w) { if (w < wave) below += wsum[w]; total += wsum[w]; }
    if (first) {
      rank = total == 0u ? EDEMPTY : (total > k ? total - k : 0u);
      if (total == 0u && threadIdx.x == 0) { blk[EDSTATE + p] = 0u; blk[EDRANK + p] = EDEMPTY; }
    }
    if (rank != EDEMPTY && below <= rank && rank - below < s) {               // exactly one lane: the counts sum to more than the rank
      unsigned c = below;
#pragma unroll
      for (int i = 0; i < EDBINS / EDLANES; ++i) {
        if (i < per && c <= rank && rank - c < v[i]) {
          blk[EDSTATE + p] = (prefix << bits) | (unsigned)(threadIdx.x * per + i);
          blk[EDRANK + p] = rank - c;
        }
        c += v[i];
      }
    }
    __syncthreads();                                                           // wsum is reused by the next population
  }
  if (!last) return;
  __threadfence();
  __syncthreads();
  if ((int)threadIdx.x < npop / 4) {
    unsigned t = EDEMPTY;
    for (int b = 0; b < 4; ++b) {
      const int p = 4 * threadIdx.x + b;
      const unsigned pr = blk[EDSTATE + p];
      if (blk[EDRANK + p] != EDEMPTY && pr < t) t = pr;
    }
    blk[EDTHR + threadIdx.x] = t;
    blk[EDKEPT + threadIdx.x] = 0u;
  }
}

// a lane's kept pixels summed over its wave, one atomic per wave and channel
__device__ __forceinline__ void ed_kept(unsigned* blk, const unsigned mine[3], int nch) {
  for (int c = 0; c < nch; ++c) {
    unsigned v = mine[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&blk[EDKEPT + c], v);
  }
}

// the mask, route 1: g from the frame
template <bool VEC>
__global__ __launch_bounds__(EDLANES) void k_img_ed_mask(const float* __restrict__ f, int H, int W, unsigned* __restrict__ blk, unsigned char* __restrict__ mask) {
  constexpr int NCH = VEC ? 1 : 3;
  float t[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) t[c] = __uint_as_float(blk[EDTHR + c]);
  unsigned mine[3] = {0u, 0u, 0u};
  const int tx = (W + 63) / 64, tiles = tx * ((H + 3) / 4);
  const long n = (long)H * W;
  for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const int ty = tl / tx, x = (tl - ty * tx) * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) continue;
    unsigned key[3], sec[3];
    ed_grad<VEC>(f, H, W, y, x, key, sec);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const bool m = __uint_as_float(key[c]) >= t[c];
      mask[c * n + (long)y * W + x] = m ? 1 : 0;
      mine[c] += m ? 1u : 0u;
    }
  }
  ed_kept(blk, mine, NCH);
}

// the mask, route 2: g from the keys; the sectors in `mask` are overwritten
template <bool VEC>
__global__ __launch_bounds__(EDLANES) void k_img_ed_mask_keys(const unsigned* __restrict__ keys, long n, unsigned* __restrict__ blk, unsigned char* __restrict__ mask) {
  constexpr int NCH = VEC ? 1 : 3;
  float t[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) t[c] = __uint_as_float(blk[EDTHR + c]);
  unsigned mine[3] = {0u, 0u, 0u};
  for (long i = (long)blockIdx.x * EDLANES + threadIdx.x; i < n; i += (long)gridDim.x * EDLANES) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const bool m = __uint_as_float(keys[c * n + i]) >= t[c];
      mask[c * n + i] = m ? 1 : 0;
      mine[c] += m ? 1u : 0u;
    }
  }
  ed_kept(blk, mine, NCH);
}

// ---- the rows of the masked pair solve: grid (6, Py), row blockIdx.y of plane blockIdx.x = 2 c + d ----------------------------------------
__global__ __launch_bounds__(WN_LANES) void k_img_ed_rows(const float* __restrict__ s, const float* __restrict__ b, long pitch, const unsigned char* __restrict__ mask,
                                                          long mask_pitch, long mask_plane, int H, int W, int Py, int Px, int logPx, const float2* __restrict__ tw,
                                                          const float* __restrict__ wy, const float* __restrict__ wx, float2* __restrict__ Z, float* __restrict__ slot) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  __shared__ float red[WN_LANES];
  const int p = blockIdx.x, y = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x, c = p >> 1, d = p & 1;
  float2* o = Z + ((long)p * Py + y) * Px;
  if (y >= H) {                                  // (the whole workgroup)
    for (int j = tid; j < Px; j += nthr) o[j] = make_float2(0.f, 0.f);
    return;
  }
  const long off = (long)y * pitch + c, step = d ? pitch : 3;
  const unsigned char* mrow = mask + c * mask_plane + (long)y * mask_pitch;
  const int xlim = d ? (y < H - 1 ? W : 0) : W - 1;   // the columns that have their neighbour inside the window
  const float wrow = wy[y];
  float acc = 0.f;
  for (int j = tid; j < Px; j += nthr) {
    float2 v = make_float2(0.f, 0.f);
    if (j < xlim) {
      const long at = off + 3L * j;
      const float w = wrow * wx[j], m = mrow[j] ? 1.f : 0.f;
      v = make_float2(w * (m * (s[at + step] - s[at])), w * (b[at + step] - b[at]));
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

struct EdRowsMask { const unsigned char* mask; long pitch, plane; };

}  // namespace

hipError_t ics_launch_img_psf_estimate_masked(const float* sharp, const float* blurred, long pitch, const unsigned char* mask, long mask_pitch, long mask_plane,
                                              int H, int W, int K, float regularisation, int coupling, int Py, int Px, void* workspace, hipStream_t s) {
  if (!mask || mask_pitch < W) return hipErrorInvalidValue;
  if (hipError_t e = wn_raise_lds<k_img_ed_rows>(Py, Px); e != hipSuccess) return e;
  EdRowsMask m = {mask, mask_pitch, mask_plane};
  const auto rows = [](const IcsPeRows& r, void* user, hipStream_t st) -> hipError_t {
    const EdRowsMask* mk = static_cast<const EdRowsMask*>(user);
    hipLaunchKernelGGL(k_img_ed_rows, dim3(6, (unsigned)r.Py), dim3(r.lanes), r.lds, st, r.sharp, r.blurred, r.pitch, mk->mask, mk->pitch, mk->plane, r.H, r.W, r.Py, r.Px,
                       r.logPx, r.twx, r.wy, r.wx, r.Za, r.slot);
    return hipGetLastError();
  };
  return ics_launch_img_psf_estimate_rows(rows, &m, sharp, blurred, pitch, H, W, K, regularisation, coupling, Py, Px, workspace, s);
}

size_t ics_img_shock_block_lds() { return (size_t)8 * EDN * sizeof(float); }

// frames a run borrows: every launch but the last writes one of two
int ics_img_shock_frames(int iterations, int route) {
  const int launches = route == 2 ? (iterations + EDT - 1) / EDT : iterations;
  return launches - 1 < 2 ? (launches - 1 < 0 ? 0 : launches - 1) : 2;
}

hipError_t ics_launch_img_shock(const float* src, int H, int W, int iterations, float dt, float inv_flat, int coupling, int route, float* const tmp[2],
                                float* out, hipStream_t s) {
  if (iterations < 1 || (route != 1 && route != 2) || H < 1 || W < 1) return hipErrorInvalidValue;
  const size_t lds = ics_img_shock_block_lds();
  if (route == 2) {
    const hipError_t e = coupling ? set_dynamic_lds(k_img_ed_shock_block<true>, lds) : set_dynamic_lds(k_img_ed_shock_block<false>, lds);
    if (e != hipSuccess) return e;
  }
  const int per = route == 2 ? EDT : 1, launches = (iterations + per - 1) / per;
  const float* in = src;
  for (int j = 0, done = 0; j < launches; ++j) {
    float* o = j == launches - 1 ? out : tmp[j & 1];
    const int n = iterations - done < per ? iterations - done : per;
    if (route == 1) ICS_LAUNCH_VEC(coupling, k_img_ed_shock, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, s, in, o, H, W, dt, inv_flat);
    else ICS_LAUNCH_VEC(coupling, k_img_ed_shock_block, dim3((W + EDB - 1) / EDB, (H + EDB - 1) / EDB), dim3(EDSL), lds, s, in, o, H, W, n, dt, inv_flat);
    in = o; done += n;
  }
  return hipGetLastError();
}

size_t ics_img_edge_block_words() { return EDKEPT + 3; }
size_t ics_img_edge_result_word() { return EDTHR; }
size_t ics_img_edge_key_words(int H, int W, int coupling, int route) { return route == 2 ? (size_t)(coupling ? 1 : 3) * H * W : 0; }
size_t ics_img_edge_hist_lds(int coupling) { return (size_t)(coupling ? 4 : 12) * EDBINS * sizeof(unsigned); }

hipError_t ics_launch_img_edge_mask(const float* f, int H, int W, unsigned per_sector, int coupling, int route, int cus, unsigned* blk, unsigned* keys,
                                    unsigned char* mask, hipStream_t s) {
  if ((route != 1 && route != 2) || !blk || !mask || (route == 2 && !keys) || H < 1 || W < 1 || per_sector < 1) return hipErrorInvalidValue;
  const int npop = coupling ? 4 : 12;
  const long n = (long)H * W;
  const size_t lds = ics_img_edge_hist_lds(coupling);
  hipError_t e = hipSuccess;
  if (!coupling) {
    e = set_dynamic_lds(k_img_ed_recompute<false>, lds);
    if (e == hipSuccess) e = set_dynamic_lds(k_img_ed_keys<false>, lds);
    if (e == hipSuccess) e = set_dynamic_lds(k_img_ed_hist<false>, lds);
    if (e != hipSuccess) return e;
  }
  // persistent workgroups, as many per CU as their histograms leave room for: 32 KB "vector", 96 KB "channel"
  const int per_cu = coupling ? 4 : 1;
  auto wgs = [&](long units, int k) {
    long grid = (long)(cus > 0 ? cus : 256) * k;
    if (units < grid) grid = units;
    if (const int m = ics_debug().max_wgs.load(std::memory_order_relaxed); m > 0 && grid > m) grid = m;   // test hook: several tiles per workgroup on small frames
    return dim3((unsigned)grid);
  };
  e = hipMemsetAsync(blk, 0, ics_img_edge_block_words() * sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  const long tiles = (long)((W + 63) / 64) * ((H + 3) / 4);
  const int shift[3] = {EDB1 + EDB1, EDB1, 0}, bits[3] = {EDB0, EDB1, EDB1};
  for (int pass = 0; pass < 3; ++pass) {
    if (route == 1) ICS_LAUNCH_VEC(coupling, k_img_ed_recompute, wgs(tiles, per_cu), dim3(EDLANES), lds, s, f, H, W, shift[pass], bits[pass], blk);
    else if (pass == 0) ICS_LAUNCH_VEC(coupling, k_img_ed_keys, wgs(tiles, per_cu), dim3(EDLANES), lds, s, f, H, W, keys, mask, blk);
    else ICS_LAUNCH_VEC(coupling, k_img_ed_hist, wgs((n + EDLANES * EDHK - 1) / (EDLANES * EDHK), per_cu), dim3(EDLANES), lds, s, keys, mask, n, shift[pass], blk);
    hipLaunchKernelGGL(k_img_ed_select, dim3(1), dim3(EDLANES), 0, s, blk, npop, bits[pass], per_sector, pass == 0, pass == 2);
  }
  if (route == 1) ICS_LAUNCH_VEC(coupling, k_img_ed_mask, wgs(tiles, 8), dim3(EDLANES), 0, s, f, H, W, blk, mask);
  else ICS_LAUNCH_VEC(coupling, k_img_ed_mask_keys, wgs((n + EDLANES - 1) / EDLANES, 8), dim3(EDLANES), 0, s, keys, n, blk, mask);
  return hipGetLastError();
}
