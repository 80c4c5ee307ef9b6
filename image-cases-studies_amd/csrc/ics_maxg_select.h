// ics_maxg_select.h -- the maxima of A6 / A7 of a mode-2 tile launch without the epilogue's operand reads (Route::maxg; shipped loop).
//
// The step of an inner iteration needs, per channel, max u and max |g| with g = lambd gradu + (u - ut)/2 (ics_mm_g).  k_conv_fft<2> takes
// both in its epilogue and reads u and ut under every output quad for nothing else.  Here
//   max u   comes from the update pass that WROTE u (k_update_planar has every value in a register), and
//   max |g| from the few tiles that can hold it: k_conv_fft<3> (the operand-free instance) records max |gradu| per tile (Gt) and per channel
//           (Gmax), the update pass recorded Dmax = max |(u - ut)/2| over the frame, and k_maxg_select forms g only on the tiles the skip
//           rule below cannot exclude.
// The g values it forms are the ones the epilogue formed, by the same ics_mm_g; a maximum does not depend on order: keys, dt and every
// frame stay bit for bit.
//
// ---- the skip rule -----------------------------------------------------------------------------------------------------------------------
// Notation: fl() = float32 round-to-nearest of one operation; A(x) = fl(|lambd| x) for x >= 0.  For a pixel p with stored gradient g_p and
// d_p = fl(fl(u_p - ut_p) 0.5), ics_mm_g returns  G_p = fl(fl(lambd g_p) + d_p),  and |fl(lambd g_p)| = A(|g_p|) (rounding is symmetric).
// Gt = max |g_p| over the tile, Gmax = max over the frame (same channel), Dmax = max |d_p| over the frame -- maxima of the very floats the
// selection kernel would read, so |g_p| <= Gt and |d_p| <= Dmax hold exactly, and A is monotone (fl of a product with a fixed factor).
//   (1) every pixel p of the tile:  |fl(lambd g_p) + d_p| <= A(Gt) + Dmax as reals, fl is monotone and fl(|x|) = |fl(x)|, so
//       |G_p| <= hi := fl(A(Gt) + Dmax).
//   (2) the pixel q that holds Gmax:  |fl(lambd g_q) + d_q| >= A(Gmax) - Dmax as reals, so  |G_q| >= lo := fl(A(Gmax) - Dmax)
//       (lo < 0 when Dmax is the larger one: then nothing is skipped, hi >= 0).
//   The tile is skipped iff  hi' < lo  with hi' = fl(fl(hi (1 + 2^-21)) + 2^-125): then |G_p| <= hi <= hi' < lo <= |G_q| for every pixel of the
//   tile, and q lies in a tile that is never skipped (Gt = Gmax gives hi >= lo by monotonicity), so the maximum over the scanned tiles
//   is the maximum over the frame.
// The margin (a relative 2^-21 and an absolute 2^-125, several ulps / several smallest normals) is not needed by (1) and (2) as long as
// every operation is IEEE with denormals, which is how every unit of this library is built; it covers a build that flushes denormal
// results or operands to zero in either kernel (an error below 2^-126 per operation) and costs no measurable number of tiles.
// NaN and inf: the test is ONE ordered comparison, false when either side is NaN.  A NaN in gradu makes Gt and Gmax NaN (integer maximum
// of the |.| bits: every NaN ranks above inf), a NaN in u or ut makes Dmax NaN: every tile is scanned.  Dmax = inf: hi = inf, every tile is
// scanned.  Gmax = inf with finite Dmax: lo = inf, tiles with finite hi' are skipped -- their |G_p| are finite and the tile that holds the
// inf is scanned.  tools/check_maxg_skip.hip draws adversarial triples and checks (1), (2) and the conclusion on the host.
#pragma once
#include "ics_update.h"

// the device words of a run (ics_rl::mgs).  Two sets of everything that one launch writes and the next one reads: launch n uses set n & 1,
// its selection kernel zeroes set (n + 1) & 1 -- already read by launch n - 1, written next by the update pass behind this launch and by
// launch n + 1.  Both sets are zeroed when a run starts.
#define ICS_MGS_UKEY 0      /* + 8 set + c: key of max u_c of the frame the update pass wrote (maxima_keys' ku) */
#define ICS_MGS_DBITS 4     /* + 8 set + c: bits of Dmax_c (a NaN ranks above inf), 0 when the next majoriser aliases u */
#define ICS_MGS_GMAX 16     /* + 4 set + c: bits of Gmax_c of this launch */
#define ICS_MGS_SCANNED 24  /* + set: (tile, channel) pairs the selection kernel of this launch scanned */
#define ICS_MGS_TOTAL 26    /* scanned pairs since the run started */
#define ICS_MGS_LAUNCHES 27 /* selection launches since the run started */
#define ICS_MGS_WORDS 32
#define ICS_MGS_WAVES 16    /* waves of a tile workgroup: the per-launch array of tile maxima is [unit][tile of the pair][wave] */

// d_p: the second term of ics_mm_g as it forms it; lo and hi' of the rule; the rule
ICS_UPD_HD float ics_maxg_d(float u, float ut) { return ICS_FMUL(ICS_FSUB(u, ut), 0.5f); }
ICS_UPD_HD float ics_maxg_lo(float lambd, float gmax, float dmax) { return ICS_FSUB(ICS_FMUL(__builtin_fabsf(lambd), gmax), dmax); }
ICS_UPD_HD float ics_maxg_hi(float lambd, float gt, float dmax) {
  const float hi = ICS_FADD(ICS_FMUL(__builtin_fabsf(lambd), gt), dmax);
  return ICS_FADD(ICS_FMUL(hi, 1.00000048f), 2.4e-38f);
}
ICS_UPD_HD bool ics_maxg_tile_skips(float lambd, float gt, float gmax, float dmax) { return ics_maxg_hi(lambd, gt, dmax) < ics_maxg_lo(lambd, gmax, dmax); }

// the tile grid of mode 2 (ics_conv_fft_fill_args) as the selection kernel needs it, and the planes
struct IcsMaxgSelectArgs {
  const float *gradu, *u, *ut;   // origins of the planar mirrors (plane 0)
  const uint32_t* wkeys;         // [unit][2][ICS_MGS_WAVES]: bits of max |gradu| per wave over the valid pixels of each tile (k_conv_fft<3>)
  uint32_t* state;               // ICS_MGS_* words
  uint32_t* red;                 // the reduction slot of this inner iteration: ICS_RED_MAXG raised, ICS_RED_MAXU copied from the state
  float lambd;
  int set;                       // which set of the state this launch uses
  int ntiles, tiles_x, Vy, V, ext_y, ext_x, uM, uN, ppitch;
  size_t plane;
};
