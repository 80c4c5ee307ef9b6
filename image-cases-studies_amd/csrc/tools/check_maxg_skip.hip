// check_maxg_skip.hip -- host-only run of the skip rule of ../ics_maxg_select.h (ics_maxg_tile_skips) on small synthetic "frames": a handful of
// tiles of a few pixels (gradu, u, ut), random and adversarial float32 values -- denormals, values one ulp apart, huge and tiny lambd, zeros,
// either sign, now and then an inf or a NaN.  Per frame it takes Gt per tile, Gmax and Dmax the way the kernels do (integer maxima of the |.|
// bits of the very floats ics_mm_g is fed with) and checks, with the header's functions and nothing else:
//   (a) no pixel of a skipped tile has |g| above lo = fl(fl(|lambd| Gmax) - Dmax), and the pixel that holds Gmax has |g| >= lo;
//   (b) the tile that holds Gmax is never skipped;
//   (c) the key of max |g| over the scanned tiles is, in every bit, the key over all tiles (a NaN as the NaN key, like maxima_keys).
// `make tools/check_maxg_skip` (check_maxg_skip_san: the same under AddressSanitizer + UBSan), needs no GPU.
//   tools/check_maxg_skip [frames [seed]]
// Exit status 0: every frame passes; 1: a violation (the first one on stderr); 2: usage.
#include "../ics_maxg_select.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static uint32_t absbits(float f) { return bits_of(f) & 0x7FFFFFFFu; }
static float unit() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static float ulps(float x, int k) {   // x moved by k ulps (finite x, stays finite or reaches inf)
  if (x != x || std::isinf(x)) return x;
  for (int i = 0; i < (k < 0 ? -k : k); ++i) x = std::nextafterf(x, k < 0 ? -INFINITY : INFINITY);
  return x;
}
static float sign() { return (rnd() & 1) ? -1.f : 1.f; }

// a value of the family `kind` around `base`
static float draw(int kind, float base) {
  switch (kind) {
    case 0: return sign() * base * (0.5f + unit());                          // the frame's scale
    case 1: return sign() * ulps(base, (int)(rnd() % 5) - 2);                // within two ulps of the base: ties everywhere
    case 2: return sign() * from_bits(rnd() & 0x007FFFFFu);                  // denormal
    case 3: return from_bits(rnd());                                         // any bit pattern (NaN and inf included)
    case 4: return 0.f * sign();
    case 5: return sign() * from_bits(0x00800000u + (rnd() & 0xFFu));        // the smallest normals
    case 6: return sign() * from_bits(0x7F7FFFFFu - (rnd() & 0xFFu));        // the largest finite values
    default: return sign() * std::ldexp(1.f + unit(), (int)(rnd() % 253) - 126);
  }
}
static float draw_lambd(int kind) {
  switch (kind) {
    case 0: return 1.f + unit();
    case 1: return 10000.f;                                                  // the drivers' value for the non-blind phase
    case 2: return std::ldexp(1.f + unit(), 100 + (int)(rnd() % 27));        // huge: products overflow
    case 3: return std::ldexp(1.f + unit(), -120 - (int)(rnd() % 29));       // tiny: products underflow
    case 4: return 0.f;
    case 5: return -(1.f + unit());
    case 6: return from_bits(rnd());
    default: return std::ldexp(1.f + unit(), (int)(rnd() % 60) - 30);
  }
}
static uint32_t key_of_bits(uint32_t ag) { return ag > 0x7F800000u ? 0xFFC00000u : ics_f2key(from_bits(ag)); }

int main(int argc, char** argv) {
  if (argc > 3) { fprintf(stderr, "usage: %s [frames [seed]]\n", argv[0]); return 2; }
  const long frames = argc > 1 ? atol(argv[1]) : 2000000L;
  if (argc > 2) rng_state ^= (uint64_t)atoll(argv[2]) * 0xD1342543DE82EF95ull + 1ull;
  constexpr int TILES = 5, PX = 6;
  long skipped = 0, scanned = 0, with_nan = 0;
  for (long f = 0; f < frames; ++f) {
    const float lambd = draw_lambd((int)(rnd() % 8));
    const float gbase = std::ldexp(1.f + unit(), (int)(rnd() % 200) - 100), ubase = std::ldexp(1.f + unit(), (int)(rnd() % 200) - 100);
    // one family per frame and operand most of the time (so that maxima are close calls), any family now and then
    const int gk = (int)(rnd() % 8), uk = (int)(rnd() % 8), mix = (rnd() % 4) == 0;
    float g[TILES][PX], u[TILES][PX], ut[TILES][PX];
    uint32_t gt[TILES], gmax = 0u, dmax = 0u;
    for (int t = 0; t < TILES; ++t) {
      gt[t] = 0u;
      for (int p = 0; p < PX; ++p) {
        g[t][p] = draw(mix ? (int)(rnd() % 8) : gk, gbase);
        u[t][p] = draw(mix ? (int)(rnd() % 8) : uk, ubase);
        ut[t][p] = (rnd() % 3) == 0 ? u[t][p] : ((rnd() & 1) ? ulps(u[t][p], (int)(rnd() % 9) - 4) : draw(mix ? (int)(rnd() % 8) : uk, ubase));
        const float d = ics_maxg_d(u[t][p], ut[t][p]);
        gt[t] = gt[t] > absbits(g[t][p]) ? gt[t] : absbits(g[t][p]);
        dmax = dmax > absbits(d) ? dmax : absbits(d);
      }
      gmax = gmax > gt[t] ? gmax : gt[t];
    }
    const float Gmax = from_bits(gmax), Dmax = from_bits(dmax);
    const float lo = ics_maxg_lo(lambd, Gmax, Dmax);
    uint32_t all = 0u, kept = 0u;
    bool nan_seen = false;
    for (int t = 0; t < TILES; ++t) {
      const bool skip = ics_maxg_tile_skips(lambd, from_bits(gt[t]), Gmax, Dmax);
      if (skip && gt[t] == gmax) { fprintf(stderr, "frame %ld: the tile that holds Gmax is skipped (lambd %a Gmax %a Dmax %a)\n", f, lambd, Gmax, Dmax); return 1; }
      skip ? ++skipped : ++scanned;
      for (int p = 0; p < PX; ++p) {
        const float G = ics_mm_g(lambd, g[t][p], u[t][p], ut[t][p]);
        const uint32_t ab = absbits(G);
        nan_seen |= G != G;
        all = all > ab ? all : ab;
        if (!skip) kept = kept > ab ? kept : ab;
        if (skip && !(__builtin_fabsf(G) <= lo)) {
          fprintf(stderr, "frame %ld: a skipped pixel has |g| = %a above lo = %a (lambd %a gradu %a u %a ut %a Gt %a Gmax %a Dmax %a)\n", f, __builtin_fabsf(G), lo, lambd, g[t][p], u[t][p], ut[t][p],
                  from_bits(gt[t]), Gmax, Dmax);
          return 1;
        }
        if (absbits(g[t][p]) == gmax && lo == lo && !(__builtin_fabsf(G) >= lo)) {
          fprintf(stderr, "frame %ld: the pixel that holds Gmax has |g| = %a below lo = %a (lambd %a gradu %a u %a ut %a Dmax %a)\n", f, __builtin_fabsf(G), lo, lambd, g[t][p], u[t][p], ut[t][p], Dmax);
          return 1;
        }
      }
    }
    with_nan += nan_seen;
    if (key_of_bits(all) != key_of_bits(kept)) {
      fprintf(stderr, "frame %ld: key over the scanned tiles %08x, over all tiles %08x (lambd %a Gmax %a Dmax %a)\n", f, key_of_bits(kept), key_of_bits(all), lambd, Gmax, Dmax);
      return 1;
    }
  }
  printf("check_maxg_skip: %ld frames of %d tiles x %d pixels, %ld tiles skipped, %ld scanned, %ld frames with a NaN in g: no violation\n", frames, TILES, PX, skipped, scanned, with_nan);
  return 0;
}
