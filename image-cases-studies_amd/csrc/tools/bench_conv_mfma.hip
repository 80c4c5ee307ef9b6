// bench_conv_mfma.hip -- stand-alone timing harness for the matrix-core convolution (ics_conv_mfma.hip) at
// 4096^2 x 3, 15x15 PSF, the kernels as the library builds them.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I.. bench_conv_mfma.hip -o bench_conv_mfma
#include "../ics_conv_mfma.hip"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv) {
  const int M = argc > 1 ? atoi(argv[1]) : 4096, K = argc > 2 ? atoi(argv[2]) : 15, N = argc > 3 ? atoi(argv[3]) : M;
  IcsGeom g = ics_make_geom(M, N, K);
  const size_t nf = ics_frame_floats(g), org = ics_origin_offset(g);
  std::vector<float> h(nf);
  srand(1);
  for (size_t i = 0; i < nf; ++i) h[i] = (float)rand() / RAND_MAX;
  float *in, *out, *f, *u, *ut; uint32_t* red; void* bt;
  hipMalloc(&in, nf * 4); hipMalloc(&out, nf * 4); hipMalloc(&f, nf * 4); hipMalloc(&u, nf * 4); hipMalloc(&ut, nf * 4);
  hipMalloc(&red, 1024); hipMemset(red, 0, 1024);
  for (float* p : {in, f, u, ut}) hipMemcpy(p, h.data(), nf * 4, hipMemcpyHostToDevice);
  hipMemset(out, 0, nf * 4);
  const size_t tf = ics_conv_mfma_table_floats(K);
  std::vector<_Float16> tab(tf * 2, (_Float16)0.f);
  const int rh = ((2 * (K + 17) + 3) & ~3) / 2;   // halves per weight row (MCfg::WROWB / 2)
  for (int c = 0; c < 3; ++c) for (int a = 0; a < K; ++a) for (int s = 0; s < 2; ++s) for (int hh = 0; hh < rh; ++hh) {
    const int b = hh - 7;
    const float w = (b >= 0 && b < K) ? 16384.f / (K * K) * (1.f + 0.01f * a + 0.02f * b) : 0.f;
    const _Float16 hi = (_Float16)w;
    tab[((size_t)c * K + a) * 2 * rh + 4 * (hh >> 1) + 2 * s + (hh & 1)] = s ? (_Float16)(w - (float)hi) : hi;
  }
  reinterpret_cast<float*>(tab.data())[tf - 4] = 1.f / 16384.f;
  hipMalloc(&bt, tf * 4); hipMemcpy(bt, tab.data(), tf * 4, hipMemcpyHostToDevice);
  IcsConvArgs a = {};
  a.in = in + org; a.out = out + org; a.f = f + org; a.u = u + org; a.ut = ut + org; a.red = red; a.lambd = 1.f; a.bt = bt; a.g = g;
  if (!getenv("ICS_BENCH_NO_ACC")) {   // the image in accumulator order for both tile heights (ics_image_acc.h)
    for (int k = 0; k < 2; ++k) {
      float* p = nullptr;
      hipMalloc(&p, ics_image_acc_floats(g, k ? 4 : 2) * 4);
      ics_launch_image_acc(a.f, g, k ? 4 : 2, p, 0);
      a.facc[k] = p;
    }
  }
  uint32_t* sched = nullptr; hipMalloc(&sched, 64); hipMemset(sched, 0, 64);
  if (!getenv("ICS_BENCH_NO_SCHED")) a.sched = sched;   // dynamic tile claiming as in the library (the launcher decides per launch)
  {
    int nb0 = -1, nb1 = -1;
    if (K == 15) {
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb0, k_conv_mfma<15, 0, 2, 1>, 256, MCfg<15, 2>::LDS_BYTES);
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb1, k_conv_mfma<15, 1, 2, 1>, 256, MCfg<15, 2>::LDS_BYTES);
      printf("occupancy (workgroups per CU) K=15, 32-row tiles: mode 0 %d, mode 1 %d, LDS %zu B\n", nb0, nb1, (size_t)MCfg<15, 2>::LDS_BYTES);
    }
  }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int mode = 0; mode < 2; ++mode) {
    // long runs: the first milliseconds after idle are timed at ramping clocks, and a sustained loop of this kernel sits at
    // the board power cap (1.39 kW, sclk ~2.1 GHz) -- a 20-launch timing ranked the variants differently
    for (int i = 0; i < 200; ++i) if (ics_launch_conv_mfma(mode, a, 0) != hipSuccess) { printf("launch failed\n"); return 1; }
    hipEventRecord(e0);
    const int reps = getenv("ICS_BENCH_REPS") ? atoi(getenv("ICS_BENCH_REPS")) : 2000;   // long runs: sample clocks / power beside it
    for (int i = 0; i < reps; ++i) ics_launch_conv_mfma(mode, a, 0);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("mode %d: %.4f ms\n", mode, ms / reps);
  }
  return 0;
}
