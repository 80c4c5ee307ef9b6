// ics_gradk_fft.hip -- transform tiles (ics_fft_tile.h): the PSF gradient, on its own (k_gradk_fft, A12 + A13) and fused with the
// synthesis that feeds it (k_synth_gradk_fft, A11 + A12 + A13), and the reduction of the workgroups' K x K blocks.
#include "ics_fft_tile.h"
#include <climits>

namespace icsfft {

// ---- A12 + A13 (lib/deconvolution.pyx:567-571): the PSF gradient on the same tiles -----------------------------------------------------------
//     gradk[a, b, c] = sum_{y,x} e'[y, x, c] u[y + pad - a, x + pad - b, c]            (u-frame coordinates; e' = 0 outside the M x N interior)
// Per tile of V x V residual pixels with the 128 x 128 window t of u that starts pad pixels up and left of it:
//     g[a][b] = sum_{v,h<V} e'[v][h] t[v + K-1-a][h + K-1-b] = corr(e' zero-padded, t) at lag (K-1-a, K-1-b) < K  (no wrap-around: v + lag <= 127)
// and corr = IDFT( conj(DFT e') . DFT t ).  The two tiles of a pair travel as real and imaginary part as in the convolutions:
// conj(E0 + i E1) (T0 + i T1) = conj(E0) T0 + conj(E1) T1 + i (...), and the transforms of the first two terms are REAL -- the real part of
// the inverse transform is the sum of both tiles' correlations.  The product is linear: a workgroup keeps ONE channel, adds the products
// of all its tile pairs up in the frequency domain (sixteen complex values per thread) and transforms back once at the end -- two forward
// transforms per pair and no inverse; one K x K block per workgroup, added up in double by k_gradk_fft_reduce in a fixed order.
// fp32 throughout.  Against float64 direct sums on the test frames 1 - 3e-7 of max |gradk| (gate 1e-5); the error scales with
// |e'| |u| of a tile rather than with the sums themselves, so a residual that is pure noise uncorrelated with u is the worst case (4e-5
// estimated for sigma 1e-2 at 600 x 700) -- the matrix-core kernel (ics_gradk_mfma.hip) stays behind conv = ICS_CONV_MATRIX.
template <int DUMMY>
__global__ __launch_bounds__(ICS_FFT_THREADS) void k_gradk_fft(IcsFftArgs a, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) v2f lds[];
  v2f* const twl = lds + ICS_FFT_P * ICS_FFT_PITCH;
  const int tid = threadIdx.x;
  if (tid < ICS_FFT_TW_ENTRIES) twl[tid] = tw128((tid / ICS_FFT_TWS) * (tid % ICS_FFT_TWS));
  const Mem mem = make_mem(a, 0);                 // in = u, f = e' (the geometry of mode 0: tiles of the M x N interior)
  const int c = (int)blockIdx.x % 3, slot = (int)blockIdx.x / 3, nslots = (int)gridDim.x / 3, npairs = (a.ntiles + 1) / 2;
  v2f acc[2][8];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[s][k] = (v2f){0.f, 0.f};
  for (int p = slot; p < npairs; p += nslots) {
    const Unit u = decode_unit(a, 3 * p + c);
    v4f pe[2][4], pw[2][4];
    load_image(a, mem, u, opaque(tid), pe);       // the residual tiles, zero beyond V x V and beyond the interior
    lds_barrier();                                // (the previous pair's stage D has read the tile)
    store_window(pe, lds, opaque(tid));
    lds_barrier();
    stage_a(lds, opaque(tid));
    load_window(a, mem, u, opaque(tid), pw, 0, 2, a.lag_y, a.lag_x);      // (behind stage A: registers; tap blocks: the window of this launch's lag block)
    lds_barrier();
    stage_b<1>(lds, opaque(tid));
    lds_barrier();
    stage_c<4>(lds, lds, twl, opaque(tid));
    wave_sync();
    v2f ze[2][8];
    stage_d_forward(lds, opaque(tid), ze);
    lds_barrier();
    store_window(pw, lds, opaque(tid));
    lds_barrier();
    stage_a(lds, opaque(tid));
    lds_barrier();
    stage_b<1>(lds, opaque(tid));
    lds_barrier();
    stage_c<4>(lds, lds, twl, opaque(tid));
    wave_sync();
    v2f zu[2][8];
    stage_d_forward(lds, opaque(tid), zu);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[s][k] += cmulc(zu[s][k], ze[s][k]);     // += DFT(t) conj(DFT(e'))
  }
  lds_barrier();
  stage_d_inverse(acc, lds, opaque(tid));
  wave_sync();
  stage_e(lds, lds, twl, opaque(tid));
  lds_barrier();
  stage_b<-1>(lds, opaque(tid));
  lds_barrier();
  stage_g(lds, opaque(tid));
  lds_barrier();
  const int K = a.c.g.K;
  if (a.blk_k) {   // tap blocks: the blk_k x blk_k lags of this launch's block, in lag order (k_gradk_fft_reduce_blk places them)
    const int Kb = a.blk_k;
    for (int i = tid; i < Kb * Kb; i += ICS_FFT_THREADS) {
      const int ly = i / Kb, lx = i - ly * Kb;
      partial[(size_t)blockIdx.x * Kb * Kb + i] = lds[ly * ICS_FFT_PITCH + lx].x * (1.0f / (ICS_FFT_P * ICS_FFT_P));
    }
    return;
  }
  for (int i = tid; i < K * K; i += ICS_FFT_THREADS) {
    const int aa = i / K, bb = i - aa * K;
    partial[(size_t)blockIdx.x * K * K + i] = lds[(K - 1 - aa) * ICS_FFT_PITCH + (K - 1 - bb)].x * (1.0f / (ICS_FFT_P * ICS_FFT_P));
  }
}

// ---- A11 + A12 + A13 (pyx:555-571) as ONE unit on the tiles: three transforms where k_conv_fft<0> + k_gradk_fft run four -------------------
// Per tile pair and channel, with t = the two 128 x 128 windows of u (real / imaginary part):
//     T = DFT(t)                                          A B C D        kept in registers (sixteen values per thread)
//     r = IDFT(S T);  e' = (r - image) on the valid V x Vy pixels inside the interior, 0 elsewhere       D E F G + row-quad epilogue, IN the tile buffer
//     acc += T conj(DFT(e'))                              A B C D        the workgroup's running sum, as k_gradk_fft
// The residual never leaves the CU (it is stored only under the stop-test window, whose statistics read it: pyx:600-601, 627), the window
// is read once instead of twice and transformed once.  The same stage functions in the same order as the two kernels it replaces and the
// same walk (workgroup = channel blockIdx % 3, pairs slot, slot + nslots, ...): e' and the K x K blocks are bit-identical to theirs.
// Registers (1024 threads: 128): acc and T stay alive through the unit, so the sixteen-point stages run in their lean forms and the
// two prefetches sit beside eight-point stages only: the image quads are requested behind stage G's last LDS write (in flight through the
// barrier), the next unit's window in front of the second stage D.
template <int DUMMY>
__global__ __launch_bounds__(ICS_FFT_THREADS) void k_synth_gradk_fft(IcsFftArgs a, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) v2f lds[];
  v2f* const twl = lds + ICS_FFT_P * ICS_FFT_PITCH;
  const int tid = threadIdx.x;
  if (tid < ICS_FFT_TW_ENTRIES) twl[tid] = tw128((tid / ICS_FFT_TWS) * (tid % ICS_FFT_TWS));
  const Mem mem = make_mem(a, 0);                 // in = u, f = image, out = e' (the geometry of mode 0: tiles of the M x N interior)
  const int c = (int)blockIdx.x % 3, slot = (int)blockIdx.x / 3, nslots = (int)gridDim.x / 3, npairs = (a.ntiles + 1) / 2;
  v2f acc[2][8];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[s][k] = (v2f){0.f, 0.f};
  if (slot < npairs) {
    v4f pw[2][4];
    load_window(a, mem, decode_unit(a, 3 * slot + c), opaque(tid), pw);
    store_window(pw, lds, opaque(tid));
    lds_barrier();
    stage_a(lds, opaque(tid));
  }
  for (int p = slot; p < npairs; p += nslots) {
    const Unit u = decode_unit(a, 3 * p + c);
    lds_barrier();
    stage_b<1>(lds, opaque(tid));
    lds_barrier();
    v2f zu[2][8];
    {
      v2f sp[2][8];
      load_spectrum(mem, c, opaque(tid), sp);
      stage_c<4>(lds, lds, twl, opaque(tid));
      wave_sync();
      stage_d_keep(sp, lds, opaque(tid), zu);
    }
    wave_sync();
    stage_e_lean(lds, lds, twl, opaque(tid));
    lds_barrier();
    stage_b<-1>(lds, opaque(tid));
    lds_barrier();
    stage_g(lds, opaque(tid));
    {
      // the image quads in two halves of two row groups: the first is requested behind stage G's last LDS write (in flight through the
      // barrier), the second in front of the first half's arithmetic -- 96 registers of spectra and image beside the epilogue otherwise
      v4f fimg[2][4];
      load_image_rows(a, mem, u, opaque(tid), fimg, 0, 2);
      lds_barrier();
      load_image_rows(a, mem, u, opaque(tid), fimg, 2, 4);
      QuadOut qo[2];
      const int te = opaque(tid);
#pragma unroll
      for (int t = 0; t < 2; ++t) qo[t].vo = quad_lane(a, u, mem.lay, te, t, qo[t].rows, qo[t].X);
      const bool edge = u.ox[0] < a.ox0 || u.ox[0] + a.V > a.ox1 || u.ox[1] < a.ox0 || u.ox[1] + a.V > a.ox1;
      bool store = a.store_all != 0;
#pragma unroll
      for (int t = 0; t < 2; ++t) store = store || (u.has[t] && u.oy[t] < a.wy1 && u.oy[t] + a.Vy > a.wy0 && u.ox[t] < a.wx1 && u.ox[t] + a.V > a.wx0);   // (uniform)
      if (store) {
#pragma unroll
        for (int i = 0; i < 4; ++i) residual_quads(a, mem, qo, edge, true, lds, te, i, fimg);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) residual_quads(a, mem, qo, edge, false, lds, te, i, fimg);
      }
    }
    lds_barrier();
    stage_a(lds, opaque(tid));
    lds_barrier();
    stage_b<1>(lds, opaque(tid));
    lds_barrier();
    stage_c<4>(lds, lds, twl, opaque(tid));
    wave_sync();
    {
      v4f pw[2][4];
      load_window(a, mem, decode_unit(a, 3 * (p + nslots) + c), opaque(tid), pw);   // next unit (beyond the last one: dropped accesses)
      stage_d_acc(lds, opaque(tid), zu, acc);
      if (p + nslots < npairs) {
        lds_barrier();                              // (every wave has read its rows)
        store_window(pw, lds, opaque(tid));
        lds_barrier();
        stage_a(lds, opaque(tid));
      }
    }
  }
  lds_barrier();
  stage_d_inverse(acc, lds, opaque(tid));
  wave_sync();
  stage_e(lds, lds, twl, opaque(tid));
  lds_barrier();
  stage_b<-1>(lds, opaque(tid));
  lds_barrier();
  stage_g(lds, opaque(tid));
  lds_barrier();
  const int K = a.c.g.K;
  for (int i = tid; i < K * K; i += ICS_FFT_THREADS) {
    const int aa = i / K, bb = i - aa * K;
    partial[(size_t)blockIdx.x * K * K + i] = lds[(K - 1 - aa) * ICS_FFT_PITCH + (K - 1 - bb)].x * (1.0f / (ICS_FFT_P * ICS_FFT_P));
  }
}

// tap blocks: lag (lag_y + ly, lag_x + lx) is tap (K - 1 - lag_y - ly, K - 1 - lag_x - lx) of the gradient; one wave per value as below
__global__ __launch_bounds__(256) void k_gradk_fft_reduce_blk(const float* __restrict__ partial, int nblocks, int K, int Kb, int lag_y, int lag_x, float* __restrict__ gradk) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= 3 * Kb * Kb) return;
  const int c = i % 3, l = i / 3, ly = l / Kb, lx = l - ly * Kb;
  const int aa = K - 1 - lag_y - ly, bb = K - 1 - lag_x - lx;
  if (aa < 0 || bb < 0) return;
  double s = 0.0;
  for (int b = c + 3 * lane; b < nblocks; b += 192) s += (double)partial[(size_t)b * Kb * Kb + l];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) gradk[(aa * K + bb) * 3 + c] = (float)s;
}

// gradk[a][b][c] = sum of the blocks of the workgroups that kept channel c (block % 3 == c), in double.  One wave per value: lane l adds
// blocks c + 3 l, c + 3 (l + 64), ... and the 64 lane sums meet in a fixed butterfly (the same bits run after run).  (One thread per value
// with its 85 serial loads took 27 us, 7 % of the gradient kernel it follows.)
__global__ __launch_bounds__(256) void k_gradk_fft_reduce(const float* __restrict__ partial, int nblocks, int K, float* __restrict__ gradk) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= 3 * K * K) return;
  const int c = i % 3, ab = i / 3;
  double s = 0.0;
  for (int b = c + 3 * lane; b < nblocks; b += 192) s += (double)partial[(size_t)b * K * K + ab];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) gradk[i] = (float)s;
}

}  // namespace icsfft

// ---- launchers -----------------------------------------------------------------------------------------------------------------------------
int ics_gradk_fft_blocks(int cus) { return ics_fft_grid(cus, INT_MAX, true); }

// the arguments of the gradient kernels: in = u, f and out as given (the geometry of mode 0: tiles of the M x N interior)
static IcsFftArgs gradk_args(const float* u, const float* f, float* out, const float* spec, const IcsGeom& g, int blk_n = 0, int blk_k = 0) {
  IcsConvArgs c;
  memset(&c, 0, sizeof c);
  c.g = g; c.in = u; c.f = f; c.out = out; c.u = u; c.ut = u;
  IcsFftArgs a;
  ics_conv_fft_fill_args(0, c, spec, &a, blk_n, blk_k);
  return a;
}
static std::atomic<bool> gradk_configured[ICS_MAX_DEVICES];   // k_gradk_fft<0>: both of its launchers

// A12 + A13 on the transform tiles: u and e = origins of channel-planar mirrors; partial: ics_gradk_fft_blocks() * K * K floats
hipError_t ics_launch_gradk_fft(const float* u, const float* e, const IcsGeom& g, float* partial, float* gradk, hipStream_t s) {
  const IcsFftArgs a = gradk_args(u, e, const_cast<float*>(e), nullptr, g);
  const int grid = ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits, true);
  if (hipError_t err = ics_fft_launch(gradk_configured, icsfft::k_gradk_fft<0>, grid, s, a, partial); err != hipSuccess) return err;
  hipLaunchKernelGGL(icsfft::k_gradk_fft_reduce, dim3((3 * g.K * g.K + 3) / 4), dim3(256), 0, s, partial, grid, g.K, gradk);
  return hipGetLastError();
}
// A11 + A12 + A13 in one kernel: u, f, e = origins of channel-planar mirrors; spec = the convolution orientation's spectrum; the window
// (u-frame coordinates) says which tiles store their residual; partial: ics_gradk_fft_blocks() * K * K floats
hipError_t ics_launch_synth_gradk_fft(const float* u, const float* f, float* e, const float* spec, const IcsGeom& g, int wy0, int wy1, int wx0, int wx1, int store_all,
                                      float* partial, float* gradk, hipStream_t s) {
  IcsFftArgs a = gradk_args(u, f, e, spec, g);
  a.wy0 = wy0; a.wy1 = wy1; a.wx0 = wx0; a.wx1 = wx1; a.store_all = store_all;
  static std::atomic<bool> configured[ICS_MAX_DEVICES];
  const int grid = ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits, true);
  if (hipError_t err = ics_fft_launch(configured, icsfft::k_synth_gradk_fft<0>, grid, s, a, partial); err != hipSuccess) return err;
  hipLaunchKernelGGL(icsfft::k_gradk_fft_reduce, dim3((3 * g.K * g.K + 3) / 4), dim3(256), 0, s, partial, grid, g.K, gradk);
  return hipGetLastError();
}
// A12 + A13 with tap blocks: one launch of k_gradk_fft per block of lags (the residual's transform is repeated per block: the running sums of
// several blocks do not fit the registers); partial: ics_gradk_fft_blocks() * blk_k^2 floats
hipError_t ics_launch_gradk_fft_blk(const float* u, const float* e, const IcsGeom& g, int blk_n, int blk_k, float* partial, float* gradk, hipStream_t s) {
  IcsFftArgs a = gradk_args(u, e, const_cast<float*>(e), nullptr, g, blk_n, blk_k);
  const int grid = ics_fft_grid(ics_device_cus(ics_current_device()), a.nunits, true);
  for (int qy = 0; qy < blk_n; ++qy)
    for (int qx = 0; qx < blk_n; ++qx) {
      a.lag_y = qy * blk_k; a.lag_x = qx * blk_k;
      if (hipError_t err = ics_fft_launch(gradk_configured, icsfft::k_gradk_fft<0>, grid, s, a, partial); err != hipSuccess) return err;
      hipLaunchKernelGGL(icsfft::k_gradk_fft_reduce_blk, dim3((3 * blk_k * blk_k + 3) / 4), dim3(256), 0, s, partial, grid, g.K, blk_k, a.lag_y, a.lag_x, gradk);
    }
  return hipGetLastError();
}
