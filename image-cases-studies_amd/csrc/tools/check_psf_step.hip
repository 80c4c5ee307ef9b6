// check_psf_step.hip -- host-only run of ../ics_psf_step.h: the PSF step A14 ... A17 of a blind inner iteration in plain loops, with the
// header's functions and nothing else, beside a restatement of lib/deconvolution.pyx:574-589 written out in this file (float32 throughout,
// no double, the reference's operation order).  The two are compared bit for bit here; tests/test_psf_step_host.py also compares the
// output with the numpy restatement.  `make tools/check_psf_step`, needs no GPU.
//   tools/check_psf_step IN OUT
//   IN  : int32 K, correlation; float32 step; float32 psf [K x K x 3], gradk [K x K x 3]
//   OUT : float32 local psf [K x K x 3], caller's psf [K x K x 3], dtpsf        (from the header's functions)
// Exit status 0: the header and the restatement agree in every bit; 1: they differ (the first difference on stderr); 2: usage / I/O.
#include "../ics_psf_step.h"
#include <cstdio>
#include <cstring>
#include <vector>

// ---- the step with the functions of ics_psf_step.h, the maxima as keys like the kernels take them ----
static float step_header(std::vector<float>& p, std::vector<float>& caller, const std::vector<float>& g, int K, float step, bool correlation) {
  const int KK = K * K, n = 3 * KK;
  uint32_t kp = 0u, kg = 0u;
  for (int i = 0; i < n; ++i) {
    const uint32_t k1 = ics_key_of(p[i]), k2 = ics_key_of(__builtin_fabsf(g[i]));
    kp = kp > k1 ? kp : k1; kg = kg > k2 ? kg : k2;
  }
  const float dtpsf = ics_psf_dt(step, K, ics_key2f(kp), ics_key2f(kg));
  for (int i = 0; i < n; ++i) { p[i] = ics_psf_step_px(p[i], dtpsf, g[i]); caller[i] = p[i]; }
  if (correlation)
    for (int i = 0; i < KK; ++i) { const float m = ics_psf_mean3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); p[3 * i] = p[3 * i + 1] = p[3 * i + 2] = m; }
  for (int i = 0; i < n; ++i) p[i] = ics_psf_clamp(p[i]);
  float sum[3];
  for (int c = 0; c < 3; ++c) sum[c] = ics_psf_channel_sum(p.data(), KK, c);
  for (int i = 0; i < n; ++i) { p[i] = ics_psf_norm(p[i], sum[i % 3]); if (!correlation) caller[i] = p[i]; }
  return dtpsf;
}

// ---- the same step as the reference writes it: psf[i][j][k] arrays, channel-major normalisation (pyx:47-70), no helper of the library ----
static float step_restated(std::vector<float>& psf, std::vector<float>& caller, const std::vector<float>& gradk, int MK, float step_factor, bool correlation) {
  auto at = [MK](int i, int j, int k) { return (size_t)(i * MK + j) * 3 + k; };
  float maxp = psf[0], maxg = gradk[0] < 0.f ? -gradk[0] : gradk[0];
  for (size_t q = 0; q < psf.size(); ++q) {
    const float ag = gradk[q] < 0.f ? -gradk[q] : gradk[q];
    if (psf[q] > maxp) maxp = psf[q];
    if (ag > maxg) maxg = ag;
  }
  const float per_tap = step_factor / (float)MK;               // pyx:574
  const float num = per_tap * (maxp + 0.f);
  const float den = maxg + 1e-15f;
  const float dtpsf = num / den;
  for (int k = 0; k < 3; ++k)                                  // pyx:577-581
    for (int i = 0; i < MK; ++i)
      for (int j = 0; j < MK; ++j) { const float d = dtpsf * gradk[at(i, j, k)]; psf[at(i, j, k)] = psf[at(i, j, k)] - d; }
  caller = psf;
  if (correlation)                                             // pyx:584-585
    for (int i = 0; i < MK; ++i)
      for (int j = 0; j < MK; ++j) {
        float m = psf[at(i, j, 0)] + psf[at(i, j, 1)];
        m = m + psf[at(i, j, 2)];
        m = m / 3.0f;
        for (int k = 0; k < 3; ++k) psf[at(i, j, k)] = m;
      }
  float temp[3] = {0.f, 0.f, 0.f};                              // pyx:47-70
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < MK; ++i)
      for (int j = 0; j < MK; ++j) {
        if (psf[at(i, j, k)] < 0) psf[at(i, j, k)] = 0;
        temp[k] = temp[k] + psf[at(i, j, k)];
      }
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < MK; ++i)
      for (int j = 0; j < MK; ++j) psf[at(i, j, k)] = psf[at(i, j, k)] / temp[k];
  if (!correlation) caller = psf;
  return dtpsf;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b, const char* what) {
  for (size_t i = 0; i < a.size(); ++i)
    if (std::memcmp(&a[i], &b[i], 4) != 0) { std::fprintf(stderr, "%s[%zu]: header %.9g, restated %.9g\n", what, i, (double)a[i], (double)b[i]); return false; }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t hdr[2];
  float step;
  if (std::fread(hdr, 4, 2, in) != 2 || std::fread(&step, 4, 1, in) != 1) { std::fprintf(stderr, "short header\n"); std::fclose(in); return 2; }
  const int K = hdr[0];
  const bool correlation = hdr[1] != 0;
  if (K < 3 || K > 255 || !(K & 1)) { std::fprintf(stderr, "bad PSF size\n"); std::fclose(in); return 2; }
  const size_t n = (size_t)3 * K * K;
  std::vector<float> psf(n), g(n);
  if (std::fread(psf.data(), 4, n, in) != n || std::fread(g.data(), 4, n, in) != n) { std::fprintf(stderr, "short arrays\n"); std::fclose(in); return 2; }
  std::fclose(in);
  std::vector<float> p1 = psf, c1(n), p2 = psf, c2(n);
  const float dt1 = step_header(p1, c1, g, K, step, correlation);
  const float dt2 = step_restated(p2, c2, g, K, step, correlation);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const bool ok = std::fwrite(p1.data(), 4, n, out) == n && std::fwrite(c1.data(), 4, n, out) == n && std::fwrite(&dt1, 4, 1, out) == 1;
  if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "write failed\n"); return 2; }
  if (std::memcmp(&dt1, &dt2, 4) != 0) { std::fprintf(stderr, "dtpsf: header %.9g, restated %.9g\n", (double)dt1, (double)dt2); return 1; }
  return same_bits(p1, p2, "psf") && same_bits(c1, c2, "psf_caller") ? 0 : 1;
}
