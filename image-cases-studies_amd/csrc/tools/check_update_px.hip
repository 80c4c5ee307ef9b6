// check_update_px.hip -- host-only run of ../ics_update.h: the image update A5 + A6 + A8 + A10 value by value in plain loops, with the
// header's functions and nothing else (`make tools/check_update_px`, needs no GPU; tests/test_update_host.py compares the result with
// the numpy restatement bit for bit).
//   tools/check_update_px IN OUT
//   IN  : int32 M, N, pad, blind; float32 step, lambd; float32 u, ut, gradu [(M+2pad) x (N+2pad) x 3]; float32 image [M x N x 3]
//   OUT : float32 new u [(M+2pad) x (N+2pad) x 3]; float32 dt[3]; uint32 DoF min key, max key, NaN flag
#include "../ics_update.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t hdr[4];
  float sc[2];
  if (std::fread(hdr, 4, 4, in) != 4 || std::fread(sc, 4, 2, in) != 2) { std::fprintf(stderr, "short header\n"); return 2; }
  const int M = hdr[0], N = hdr[1], pad = hdr[2];
  const bool blind = hdr[3] != 0;
  const float step = sc[0], lambd = sc[1];
  if (M <= 0 || N <= 0 || pad < 0 || M > 4096 || N > 4096 || pad > 64) { std::fprintf(stderr, "bad sizes\n"); return 2; }
  const int uM = M + 2 * pad, uN = N + 2 * pad;
  const size_t nu = (size_t)uM * uN * 3, nf = (size_t)M * N * 3;
  std::vector<float> u(nu), ut(nu), gr(nu), f(nf);
  if (std::fread(u.data(), 4, nu, in) != nu || std::fread(ut.data(), 4, nu, in) != nu || std::fread(gr.data(), 4, nu, in) != nu ||
      std::fread(f.data(), 4, nf, in) != nf) { std::fprintf(stderr, "short frames\n"); return 2; }
  std::fclose(in);
  // A6 / A7: the maxima as keys, as the kernels take them
  uint32_t kg[3] = {0u, 0u, 0u}, ku[3] = {0u, 0u, 0u};
  for (size_t i = 0; i < nu; ++i) {
    const uint32_t k1 = ics_key_of(__builtin_fabsf(ics_mm_g(lambd, gr[i], u[i], ut[i]))), k2 = ics_key_of(u[i]);
    kg[i % 3] = kg[i % 3] > k1 ? kg[i % 3] : k1; ku[i % 3] = ku[i % 3] > k2 ? ku[i % 3] : k2;
  }
  float dt[3];
  for (int c = 0; c < 3; ++c) dt[c] = ics_step_dt(step, ics_key2f(ku[c]), ics_key2f(kg[c]));
  IcsDofKeys dof = ICS_DOF_NONE;
  std::vector<float> un(nu);
  for (int y = 0; y < uM; ++y)
    for (int x = 0; x < uN; ++x)
      for (int c = 0; c < 3; ++c) {
        const size_t i = ((size_t)y * uN + x) * 3 + c;
        float v = ics_step_u(u[i], dt[c], ics_mm_g(lambd, gr[i], u[i], ut[i]));
        if (y >= pad && y < pad + M && x >= pad && x < pad + N) {
          const float fv = f[((size_t)(y - pad) * N + (x - pad)) * 3 + c];
          const float D = ics_dof_mask(gr[i], fv, lambd, blind);
          v = ics_dof_blend(D, v, fv);
          ICS_DOF_NOTE(dof, D);
        }
        un[i] = v;
      }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const uint32_t keys[3] = {dof.kmin, dof.kmax, dof.knan};
  const bool ok = std::fwrite(un.data(), 4, nu, out) == nu && std::fwrite(dt, 4, 3, out) == 3 && std::fwrite(keys, 4, 3, out) == 3;
  if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "write failed\n"); return 2; }
  return 0;
}
