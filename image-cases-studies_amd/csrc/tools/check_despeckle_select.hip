// check_despeckle_select.hip -- host-only check of the selection networks of ../ics_img_despeckle.hip (ds_sort, ds_median, ds_forget,
// ds_key are __host__ __device__ for this program): `make tools/check_despeckle_select && tools/check_despeckle_select`, needs no GPU,
// a few seconds.  Networks of min / max exchanges obey the 0-1 principle, so all 0-1 inputs decide them: 2^3 and 2^5 for the sorts,
// 2^9 for the 3 x 3 median, 2^25 for the 5 x 5 median; then random keys with and without ties against std::sort, and the key order.
#include "../ics_img_despeckle.hip"
#include <algorithm>
#include <cstdio>
#include <random>

int main() {
  long bad = 0;
  for (int m = 0; m < 8; ++m) {
    unsigned v[3];
    for (int i = 0; i < 3; ++i) v[i] = (m >> i) & 1;
    ds_sort<3>(v);
    for (int i = 0; i < 2; ++i) bad += v[i] > v[i + 1];
  }
  for (int m = 0; m < 32; ++m) {
    unsigned v[5];
    for (int i = 0; i < 5; ++i) v[i] = (m >> i) & 1;
    ds_sort<5>(v);
    for (int i = 0; i < 4; ++i) bad += v[i] > v[i + 1];
  }
  for (int m = 0; m < 512; ++m) {
    unsigned w[3][3];
    for (int i = 0; i < 9; ++i) w[i / 3][i % 3] = (m >> i) & 1;
    for (int j = 0; j < 3; ++j) ds_sort<3>(w[j]);
    bad += ds_median<1>(w) != (unsigned)(__builtin_popcount(m) >= 5);
  }
  for (unsigned m = 0; m < (1u << 25); ++m) {
    unsigned w[5][5];
    for (int i = 0; i < 25; ++i) w[i / 5][i % 5] = (m >> i) & 1;
    for (int j = 0; j < 5; ++j) ds_sort<5>(w[j]);
    bad += ds_median<2>(w) != (unsigned)(__builtin_popcount(m) >= 13);
  }
  std::mt19937 rng(1);
  for (int it = 0; it < 200000; ++it) {
    unsigned w[5][5], f[25];
    for (int i = 0; i < 25; ++i) f[i] = w[i / 5][i % 5] = it % 2 ? rng() % 7u : rng();
    for (int j = 0; j < 5; ++j) ds_sort<5>(w[j]);
    std::sort(f, f + 25);
    bad += ds_median<2>(w) != f[12];
    const unsigned b = rng();
    bad += ds_bits(ds_key(b)) != b;
  }
  // -nan < -inf < -1 < -0 < +0 < 1 < +inf < +nan
  const unsigned order[8] = {0xffc00000u, 0xff800000u, 0xbf800000u, 0x80000000u, 0x00000000u, 0x3f800000u, 0x7f800000u, 0x7fc00000u};
  for (int i = 0; i < 7; ++i) bad += !(ds_key(order[i]) < ds_key(order[i + 1]));
  std::printf("despeckle selection networks: %ld failures\n", bad);
  return bad != 0;
}
