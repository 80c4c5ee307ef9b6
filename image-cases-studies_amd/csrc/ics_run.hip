// ics_run.hip -- the outer / inner iteration schedule of lib/deconvolution.pyx:460-659 on a job: the launch helpers (do_*), which dispatch
// on the route ics_route.hip resolved, then ics_rl_run and ics_rl_stage of the C ABI (include/ics_hip.h).  Host side only.
// Schedule of one inner iteration (all on one HIP stream, no host round trip):
//   k_conv<mode 0>  A1+A2   error = conv(u, psf) - image
//   k_conv<mode 1>  A3+A7   gradu = corr(error, psf); max|g_k|, max u_k  -> device keys
//   k_update        A5-A10  dt on device from the keys; u update + DoF blend
//   blind only: k_conv<mode 0> (A11), k_gradk + k_gradk_reduce (A13, MFMA), k_psf (A14-A17)
// Once per outer iteration: ut = u (D2D), window statistics + FFT whiteness metric (A18/A19), one
// 64-byte D2H of the scalars, and the stop decision on the host (pyx:643-654).
#include "ics_host.h"
#include "ics_maxg_select.h"

using namespace ics_host;

struct FftScope {   // fft_on for the duration of a run / stage, whatever path leaves it
  ics_rl* j;
  bool back = false;   // ics_rl_run: the mirrors hold newer data than the HWC frames (set once the run has started, cleared by the regular conversion)
  // an error return in the middle of a run: bring u and the residual back from the mirrors as well as the device still allows, so that a
  // later ics_rl_read / stage sees the state the failed run left, not a rotated buffer with stale HWC contents
  ~FftScope() {
    if (!j) return;
    if (j->fft_on && back) {
      if (pl_of(j, j->u)) (void)from_planar(j, j->u, j->ctx->stream);
      if (pl_of(j, j->e)) (void)from_planar(j, j->e, j->ctx->stream);
      (void)hipStreamSynchronize(j->ctx->stream); (void)hipGetLastError();
    }
    j->fft_on = false;
  }
};

// PSF sizes 51 ... 127 on the matrix cores (ICS_CONV_AUTO / ICS_CONV_MATRIX, shipped loop): a convolution is linear in its taps, so
// the K x K PSF is cut into blk_n x blk_n blocks of Kb x Kb taps (Kb odd, <= 33: sizes k_conv_mfma is built for); block (qa, qb) is
//     out_q[y][x] = sum_{a',b' < Kb} W[qa Kb + a'][qb Kb + b'] * in'[y + a' - Kb/2][x + b' - Kb/2],   in' = in shifted by (qa Kb + Kb/2 - pad, ...)
// i.e. the Kb x Kb kernel on a shifted pointer with a geometry that differs in K and pad only (mode 0 tiles start at the kernel's
// own pad: all three pointers move by pad - Kb/2 so that this is the image origin).  The blocks are summed as a chain through the
// kernels' own operand frames, alternating between the result frame and a scratch frame (do_conv_blocks); the maxima of A7 are taken
// over the sum by k_band_reduce.  2048^2, 63 x 63: 1.24 / 1.50 ms (run-time-sized fp32 kernel) -> see NOTES_r03.md 4c.
static int do_conv_blocks(ics_rl* j, int mode, const ics_rl_params* p, int slot, Prof& pr) {
  const IcsGeom& G = j->g;
  const int Kb = j->blk_kb, nb = j->blk_n, padb = Kb / 2, pad = G.pad;
  const size_t tf = ics_conv_mfma_table_floats(Kb);
  float* out = org(j, mode == 1 ? j->gr : j->e);
  const float* in = org(j, mode == 1 ? j->e : j->u);
  const ptrdiff_t oshift = mode == 0 ? (ptrdiff_t)(pad - padb) * (G.pitch + 3) : 0;   // mode 0: the kernel's tile origin (padb, padb) = the image origin
  // Mode 0 (residual = synthesis - image): the blocks form a CHAIN through the kernel's own "- image" operand instead of being added by
  // passes of their own.  With S_q = C_0 + ... + C_q - image, block q stores T_q = s_q S_q = conv(s_q W_q) - T_{q-1}, signs alternating
  // (s_q = -s_{q-1}: the weight tables of the conv orientation carry them, k_pack_blocks) and ending on s_{n-1} = +1; the chain starts from
  // T_{-1} = s_0 * image: the image itself for an odd number of blocks, a negated copy of it (blk_negf) for an even one.  T_q alternates
  // between the result frame and the scratch frame so that the last one lands in the result.  Same sums in the same order as adding the
  // blocks one by one (IEEE negation is exact and rounding is symmetric), one launch and 36 B/px less per block after the first, and no
  // frame of zeros read as the image operand.  (255 x 255 at 2048^2: synthesis 8.8 -> see NOTES_r04.md 4d.)
  const int nq = nb * nb;
  if (mode == 0 && !(nq & 1) && !j->negf_valid) {
    HIPCHK(ics_launch_frame_neg(j->blk_negf, j->f, j->frame_floats, j->ctx->stream));
    j->negf_valid = true;
  }
  RC(pr.begin(mode == 0 ? ICS_K_SYNTH : ICS_K_BACKPROJECT));
  for (int q = 0; q < nq; ++q) {
    const int qa = q / nb, qb = q - qa * nb;
    IcsConvArgs a;
    a.g = G; a.g.K = Kb; a.g.pad = padb;
    a.lambd = p->lambd; a.w = nullptr; a.tv = nullptr; a.tv_kind = 0;
    a.in = in + oshift + (ptrdiff_t)(qa * Kb + padb - pad) * G.pitch + 3 * (qb * Kb + padb - pad);
    if (mode == 0) {
      float* const fr[2] = {out, org(j, j->blk_scr)};            // T_q -> fr[(nq - 1 - q) & 1], read from the other one
      a.out = fr[(nq - 1 - q) & 1] + oshift;
      a.f = (q == 0 ? ((nq & 1) ? org(j, j->f) : org(j, j->blk_negf)) : fr[(nq - q) & 1]) + oshift;
    } else {
      // Mode 1 chains through the epilogue the PAM kinds use: with tv_kind = 2 the kernel stores fl32(double(T) + double(lambd * sums)) for
      // an operand frame T -- lambd = 1 and T = the blocks so far make that T_q = T_{q-1} + C_q, the sum the adding pass formed.  The
      // first block stores its raw sums as before; the maxima of A7 are taken over the finished frame by k_band_reduce below.
      float* const fr[2] = {out, org(j, j->blk_scr)};
      a.out = fr[(nq - 1 - q) & 1];
      a.f = org(j, j->f);                                       // (mode 1 reads no image operand)
      if (q > 0) { a.tv = fr[(nq - q) & 1]; a.tv_kind = ICS_TV_PAM_ISO; a.lambd = 1.0f; }
    }
    a.u = org(j, j->u); a.ut = org(j, ut_of(j));
    a.red = j->blk_red;                                   // (per-block maxima mean nothing)
    a.gr = nullptr; a.u_out = nullptr; a.scal = j->scal; a.dofkeys = dof_of(j);
    a.step = p->step_factor; a.blind = p->blind; a.want_dof = 0;
    a.bt = (mode == 1 ? j->blk_corr : j->blk_conv) + (size_t)q * tf;
    a.facc[0] = a.facc[1] = nullptr;
    a.sched = j->sched;
    HIPCHK(ics_launch_conv_mfma(mode, a, j->ctx->stream));
  }
  if (mode == 1) HIPCHK(ics_launch_band_reduce(out, org(j, j->u), org(j, ut_of(j)), G, p->lambd, 0, G.uM, red_of(j) + slot * ICS_RED_STRIDE, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

static int do_conv_fft(ics_rl* j, int mode, const ics_rl_params* p, int slot, Prof& pr) {
  IcsConvArgs a;
  memset(&a, 0, sizeof a);
  a.g = j->g; a.lambd = p->lambd;
  if (mode == 1) { a.in = porg(j, j->e); a.out = porg(j, j->gr); }
  else { a.in = porg(j, j->u); a.out = porg(j, j->e); }
  a.f = porg(j, j->f); a.u = porg(j, j->u); a.ut = porg(j, ut_of(j));
  a.red = red_of(j) + slot * ICS_RED_STRIDE;
  a.step = p->step_factor; a.blind = p->blind;
  if (p->tv_mode >= ICS_TV_PAM_ISO && mode == 1) {   // PAM kinds: the epilogue takes u and T, stores G = T + lambd gradu
    a.tv = j->tvf ? porg(j, j->tvf) : nullptr; a.tv_kind = p->tv_mode;
    if (!a.tv) return ics_set_error(ICS_ESTATE, "FFT pipeline: the TV frame has no planar mirror");
  }
  if (!a.in || !a.out || !a.f || !a.u || !a.ut) return ics_set_error(ICS_ESTATE, "FFT pipeline: a frame has no planar mirror");
  RC(pr.begin(mode == 0 ? ICS_K_SYNTH : ICS_K_BACKPROJECT));
  if (ics_conv_fft_blk_supported(j->g.K)) {   // 87 ... 255: tap blocks, their products summed in the frequency domain (k_conv_fft_blk)
    int nb, kb;
    ics_conv_fft_blk_shape(j->g.K, &nb, &kb);
    HIPCHK(ics_launch_conv_fft_blk(mode, a, mode == 1 ? j->spec_corr : j->spec_conv, nb, kb, j->ctx->stream));
  } else
  HIPCHK(ics_launch_conv_fft(mode, a, mode == 1 ? j->spec_corr : j->spec_conv, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

// Mode 2 of the tiles: A1 + A2 + A3 in ONE unit per tile pair (k_conv_fft<2>): interior tiles stay in the frequency domain between the two
// convolutions -- one forward and one inverse transform instead of two of each, at 128 - 2 K + 2 valid pixels a side instead of 128 - K + 1,
// which pays for small PSFs.  Inside ics_rl_run only (the residual frame is not produced: the statistics' window of it comes from a
// window-sized launch of mode 0 where the loop does not rewrite it anyway), shipped loop only.
// (Under AUTO up to ICS_CONV2_MAX_K, with the measurements it was set from: ics_route.hip.)
// Route::maxg: behind an update pass of the run (ics_rl::mgs_ready) the launch is the operand-free instance, with k_maxg_select behind it inside
// the same bracket; the first launch of a run has no such pass in front of it and reads its operands like every launch did.
static int do_conv2(ics_rl* j, const Route& r, const ics_rl_params* p, int slot, Prof& pr) {
  if (!j->fspec) RC(dalloc(j->ctx, &j->fspec, ics_conv2_fft_fspec_floats(j->g), false));
  if (!j->fspec_valid) {
    if (!porg(j, j->f)) return ics_set_error(ICS_ESTATE, "FFT pipeline: the image has no planar mirror");
    HIPCHK(ics_launch_fft_image_spectrum(porg(j, j->f), j->g, j->fspec, j->ctx->stream));
    j->fspec_valid = true;
  }
  IcsConvArgs a;
  memset(&a, 0, sizeof a);
  a.g = j->g; a.lambd = p->lambd;
  a.in = porg(j, j->u); a.out = porg(j, j->gr); a.f = porg(j, j->f); a.u = porg(j, j->u); a.ut = porg(j, ut_of(j));
  a.red = red_of(j) + slot * ICS_RED_STRIDE;
  a.step = p->step_factor; a.blind = p->blind;
  if (p->tv_mode >= ICS_TV_PAM_ISO) {   // PAM kinds: the epilogue takes u and T, stores G = T + lambd gradu
    a.tv = j->tvf ? porg(j, j->tvf) : nullptr; a.tv_kind = p->tv_mode;
    if (!a.tv) return ics_set_error(ICS_ESTATE, "FFT pipeline: the TV frame has no planar mirror");
  }
  if (!a.in || !a.out || !a.f || !a.ut) return ics_set_error(ICS_ESTATE, "FFT pipeline: a frame has no planar mirror");
  RC(pr.begin(ICS_K_SYNTH_BACKPROJECT));
  if (r.maxg && j->mgs_ready) {
    IcsMaxgSelectArgs m;
    memset(&m, 0, sizeof m);
    ics_conv2_fft_select_grid(j->g, &m);
    m.gradu = a.out; m.u = a.u; m.ut = a.ut; m.wkeys = j->mgs_wave; m.state = j->mgs; m.red = a.red; m.lambd = p->lambd; m.set = j->mgs_set;
    HIPCHK(ics_launch_conv2_fft(a, j->spec_conv, j->spec_corr, j->fspec, j->ctx->stream, j->mgs_wave, j->mgs + ICS_MGS_GMAX + 4 * j->mgs_set));
    HIPCHK(ics_launch_maxg_select(m, j->ctx->stream));
    j->mgs_set ^= 1;        // (the selection kernel has zeroed the other set: the update pass behind this launch records into it)
    j->mgs_ready = false;
  } else
  HIPCHK(ics_launch_conv2_fft(a, j->spec_conv, j->spec_corr, j->fspec, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}
// A1 + A2 over the stop-test window alone (the tiles that cover image rows [top, bottom) x columns [left, right)): what A18 / A19 read of the
// residual (pyx:600-601, 627) when mode 2 ran the iteration
static int do_conv_fft_window(ics_rl* j, const ics_rl_params* p, Prof& pr) {
  IcsConvArgs a;
  memset(&a, 0, sizeof a);
  a.g = j->g; a.lambd = p->lambd;
  a.in = porg(j, j->u); a.out = porg(j, j->e); a.f = porg(j, j->f); a.u = a.in; a.ut = a.in;
  if (!a.in || !a.out || !a.f) return ics_set_error(ICS_ESTATE, "FFT pipeline: a frame has no planar mirror");
  const int pad = j->g.pad;
  int y0 = p->top + pad, y1 = p->bottom + pad, x0 = p->left + pad, x1 = p->right + pad;
  if (y0 < pad) y0 = pad; if (x0 < pad) x0 = pad; if (y1 > pad + j->g.M) y1 = pad + j->g.M; if (x1 > pad + j->g.N) x1 = pad + j->g.N;
  if (y0 >= y1 || x0 >= x1) return ICS_OK;
  RC(pr.begin(ICS_K_SYNTH));
  HIPCHK(ics_launch_conv_fft_region(a, j->spec_conv, y0, x0, y1, x1, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

static int do_conv(ics_rl* j, const Route& r, int mode, const ics_rl_params* p, int slot, int want_dof, Prof& pr) {
  if (r.tiles && mode != 2) return do_conv_fft(j, mode, p, slot, pr);
  const int fam = mode == 2 ? (ics_big_supported(j->g.K) ? CONV_SIZED : CONV_PACKED) : r.conv;   // (mode 2, the update fused with A1 + A2: fp32 kernels only)
  if (fam == CONV_BLOCKS) return do_conv_blocks(j, mode, p, slot, pr);
  IcsConvArgs a;
  a.g = j->g; a.lambd = p->lambd;
  if (mode == 1) { a.in = org(j, j->e); a.w = j->wcorr; a.out = org(j, j->gr); }
  else { a.in = org(j, j->u); a.w = j->wconv; a.out = org(j, j->e); }
  a.f = org(j, j->f); a.u = org(j, j->u); a.ut = org(j, ut_of(j));
  a.red = red_of(j) + slot * ICS_RED_STRIDE;
  a.gr = org(j, j->gr); a.u_out = org(j, j->u2); a.scal = j->scal; a.dofkeys = dof_of(j);
  a.tv = (p->tv_mode != ICS_TV_SHIPPED && j->tvf) ? org(j, j->tvf) : nullptr; a.tv_kind = a.tv ? p->tv_mode : 0;
  a.step = p->step_factor; a.blind = p->blind; a.want_dof = want_dof;
  const bool matrix = fam == CONV_MATRIX;
  a.bt = matrix ? (mode == 1 ? j->bt_corr : j->bt_conv) : nullptr;
  a.facc[0] = a.facc[1] = nullptr;
  if (matrix && mode == 0 && r.image_acc) {   // the image operand of the residual in accumulator order (ics_image_acc.h)
    const int rs = ics_conv_mfma_rs(j->g.K, j->g);
    if (rs) { RC(ensure_image_acc(j, rs)); a.facc[rs == 2 ? 0 : 1] = j->facc[rs == 2 ? 0 : 1]; }
  }
  a.sched = matrix ? j->sched : nullptr;   // counters of the dynamic tile walk: the launcher decides per launch (ics_conv_mfma.hip)
  RC(pr.begin(mode == 0 ? ICS_K_SYNTH : (mode == 1 ? ICS_K_BACKPROJECT : ICS_K_UPDATE_SYNTH)));
  if (fam == CONV_SIZED) {   // run-time-sized kernels (ics_big.hip); the maxima of A7 as a pass of their own
    HIPCHK(ics_launch_conv_big(mode, a, j->psf, j->ctx->stream));
    if (mode == 1) HIPCHK(ics_launch_band_reduce(a.out, a.u, a.ut, j->g, p->lambd, 0, j->g.uM, a.red, j->ctx->stream));
  } else if (matrix) HIPCHK(ics_launch_conv_mfma(mode, a, j->ctx->stream));
  else HIPCHK(ics_launch_conv(mode, a, j->ctx->stream));
  RC(pr.end());
  if (mode == 2) { float* t = j->u; j->u = j->u2; j->u2 = t; }  // the updated frame is now `u`
  return ICS_OK;
}

// (alias_next: the next back-projection's majoriser will be the frame this pass writes -- the last inner iteration of an outer one)
static int do_update(ics_rl* j, const Route& r, const ics_rl_params* p, int slot, int want_dof, Prof& pr, int alias_next = 0) {
  IcsUpdateArgs a;
  a.u = org(j, j->u); a.ut = org(j, ut_of(j)); a.g = org(j, j->gr); a.f = org(j, j->f);
  a.u_out = org(j, j->ut_is_u ? j->u2 : j->u);
  a.red = red_of(j) + slot * ICS_RED_STRIDE; a.scal = j->scal; a.dofkeys = dof_of(j);
  a.tv = (p->tv_mode != ICS_TV_SHIPPED && j->tvf) ? org(j, j->tvf) : nullptr; a.tv_kind = a.tv ? p->tv_mode : 0; a.f_rw = org(j, j->f);
  a.step = p->step_factor; a.lambd = p->lambd; a.blind = p->blind; a.want_dof = want_dof; a.geo = j->g;
  if (a.tv_kind == ICS_TV_MM_ACTIVE) image_changed(j);          // pyx:547-549: this update also steps the image
  RC(pr.begin(ICS_K_UPDATE));
  if (r.tiles) {   // the same pass on the planar mirrors (bit-identical arithmetic, ics_planar.hip)
    a.u = porg(j, j->u); a.ut = porg(j, ut_of(j)); a.g = porg(j, j->gr); a.f = porg(j, j->f);
    a.u_out = porg(j, j->ut_is_u ? j->u2 : j->u); a.f_rw = nullptr;
    if (!a.u || !a.ut || !a.g || !a.f || !a.u_out) return ics_set_error(ICS_ESTATE, "FFT pipeline: a frame has no planar mirror");
    if (r.maxg) {   // max u and Dmax of the frame this pass writes, for the operand-free mode-2 launch behind it (set mgs_set: zeroed)
      HIPCHK(ics_launch_update_planar_rec(a, j->mgs + 8 * j->mgs_set, alias_next, j->ctx->stream));
      j->mgs_ready = true;
    } else
    HIPCHK(ics_launch_update_planar(a, j->ctx->stream));
  } else
  HIPCHK(ics_launch_update(a, j->ctx->stream));
  RC(pr.end());
  if (j->ktrace && j->ktrace_n < ICS_KEY_TRACE_SLOTS) {   // (debug switch key_trace; outside the bracket: the chain of brackets breaks, as for every unbracketed launch)
    HIPCHK(hipMemcpyAsync(j->ktrace + (size_t)j->ktrace_n++ * ICS_RED_STRIDE, a.red, ICS_RED_STRIDE * 4, hipMemcpyDeviceToDevice, j->ctx->stream));
    pr.unchain();
  }
  if (j->ut_is_u) {  // rotate: the untouched old u is the majoriser now, the stale ut frame becomes the spare
    float* old_ut = j->ut;
    j->ut = j->u; j->u = j->u2; j->u2 = old_ut;
    j->ut_is_u = false;
  }
  return ICS_OK;
}

static int do_tvterm(ics_rl* j, const Route& r, const ics_rl_params* p, int slot, Prof& pr) {
  IcsTvTermArgs a;
  a.u = org(j, j->u); a.ut = org(j, ut_of(j)); a.f = org(j, j->f); a.tv = org(j, j->tvf);
  a.red = red_of(j) + slot * ICS_RED_STRIDE; a.epsilon = p->blind ? 1e-2f : 1e-6f; a.kind = p->tv_mode; a.geo = j->g;
  if (r.tiles) {   // PAM kinds on the planar mirrors (the kernel reads u and writes T; ut and f are not touched by these kinds)
    a.u = porg(j, j->u); a.tv = porg(j, j->tvf); a.planar = 1;
    if (!a.u || !a.tv) return ics_set_error(ICS_ESTATE, "FFT pipeline: a frame has no planar mirror");
  }
  RC(pr.begin(ICS_K_UPDATE));   // accounted with the elementwise class
  HIPCHK(ics_launch_tvterm(a, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

// PSF sizes 33 ... 127: the fp16-split matrix-core gradient is built for up to 31 x 31 taps (2 x 2 blocks of 16; a third block row does
// not fit its registers), the fp32-MFMA kernel that took over above runs at a third of its rate.  The gradient is a sum over pixels
// per tap, so the K x K taps split into blocks of at most 31 x 31 -- rows / columns [0, 31), [31, 62), ... -- each a gradient of its own:
//   gradk[a0 + a'][b0 + b'] = sum E[y][x] * U'[y + pad' - a'][x + pad' - b'],   U' = U shifted by (pad - a0 - pad', pad - b0 - pad')
// i.e. the 31 x 31 (or, for the small corner block, 15 x 15) kernel on a shifted frame pointer with a geometry that differs in K and
// pad only; the frames' aprons (16 * ceil(K / 16) rows / pixels) cover the shifts.  4096^2, 45 x 45: 1.92 -> 1.22 ms.
// (33 ... 49: 2 x 2 blocks; 51 ... 127: up to 5 x 5 -- 2048^2: 63 x 63 0.98 -> 0.8 ms, 65 x 65 3.3 -> 0.8, 127 x 127 16.3 -> 2.3)
static int do_gradk_split(ics_rl* j, bool planar, Prof& pr) {
  const int K = j->g.K, pad = j->g.pad, L = 31, n = (K + L - 1) / L;
  RC(pr.begin(ICS_K_PSF_GRADIENT));
  for (int qa = 0; qa < n; ++qa)
    for (int qb = 0; qb < n; ++qb) {
      const int a0 = qa * L, b0 = qb * L, La = K - a0 < L ? K - a0 : L, Lb = K - b0 < L ? K - b0 : L;
      const int Ks = (La <= 15 && Lb <= 15) ? 15 : 31, pads = Ks / 2, nt = Ks == 15 ? 16 : 32;
      IcsGradkArgs a;
      a.geo = j->g; a.geo.K = Ks; a.geo.pad = pads;
      a.planar = planar ? 1 : 0;
      if (a.planar) { a.e = porg(j, j->e); a.u = porg(j, j->u) + (ptrdiff_t)(pad - a0 - pads) * ics_ppitch(j->g) + (pad - b0 - pads); }
      else { a.e = org(j, j->e); a.u = org(j, j->u) + (ptrdiff_t)(pad - a0 - pads) * j->g.pitch + 3 * (pad - b0 - pads); }
      a.partial = j->partial;
      // as many persistent workgroups per CU as for the sizes the kernel was built for, within what the partial buffer (sized for K) holds
      int nblocks = 2 * j->ctx->cus;                        // (GCfg::WGS of ics_gradk_mfma.hip)
      if (const int mw = ics_debug().max_wgs.load(std::memory_order_relaxed); mw > 0 && nblocks > mw) nblocks = mw;
      const long cap = (long)(j->partial_floats / (3UL * nt * nt));
      if (nblocks > cap) nblocks = (int)cap;
      HIPCHK(ics_launch_gradk_mfma(a, nblocks, j->ctx->stream));
      HIPCHK(ics_launch_gradk_reduce_block(j->partial, nblocks, j->gradk, nt, La, Lb, K, a0, b0, j->ctx->stream));
    }
  RC(pr.end());
  return ICS_OK;
}

// A13 on the route's gradient kernels (a stage of a fused family: the kernel that family fuses with A11)
static int do_gradk(ics_rl* j, const Route& r, Prof& pr) {
  const int fam = r.gradk == GK_FUSED_MATRIX ? GK_MATRIX : (r.gradk == GK_FUSED_TILES ? GK_TILES : r.gradk);
  if (fam == GK_TILES) {   // the FFT-tile pipeline's own PSF gradient (k_gradk_fft): two forward transforms per tile pair, products added up in the frequency domain
    RC(pr.begin(ICS_K_PSF_GRADIENT));
    if (ics_conv_fft_blk_supported(j->g.K)) {   // one launch per block of lags
      int nb, kb;
      ics_conv_fft_blk_shape(j->g.K, &nb, &kb);
      if ((size_t)ics_gradk_fft_blocks(j->ctx->cus) * kb * kb > j->partial_floats) return ics_set_error(ICS_ESTATE, "PSF gradient scratch too small for the lag blocks");
      HIPCHK(ics_launch_gradk_fft_blk(porg(j, j->u), porg(j, j->e), j->g, nb, kb, j->partial, j->gradk, j->ctx->stream));
    } else
    HIPCHK(ics_launch_gradk_fft(porg(j, j->u), porg(j, j->e), j->g, j->partial, j->gradk, j->ctx->stream));
    RC(pr.end());
    return ICS_OK;
  }
  if (fam == GK_SPLIT) return do_gradk_split(j, r.tiles, pr);
  IcsGradkArgs a;
  a.e = org(j, j->e); a.u = org(j, j->u); a.partial = j->partial; a.geo = j->g; a.planar = 0;
  if (r.tiles) { a.e = porg(j, j->e); a.u = porg(j, j->u); a.planar = 1; }
  RC(pr.begin(ICS_K_PSF_GRADIENT));
  if (fam == GK_SIZED) HIPCHK(ics_launch_gradk_big(a, j->gradk_blocks, j->ctx->stream));
  else if (fam == GK_MATRIX) HIPCHK(ics_launch_gradk_mfma(a, j->gradk_blocks, j->ctx->stream));
  else HIPCHK(ics_launch_gradk(a, j->gradk_blocks, j->ctx->stream));
  HIPCHK(ics_launch_gradk_reduce(j->partial, j->gradk_blocks, j->gradk, j->g, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

// A11 + A13 as one three-transform unit on the tiles (k_synth_gradk_fft)
static int do_synth_gradk_fft(ics_rl* j, const ics_rl_params* p, int store_all, Prof& pr) {
  const float *u = porg(j, j->u), *f = porg(j, j->f);
  float* e = porg(j, j->e);
  if (!u || !f || !e) return ics_set_error(ICS_ESTATE, "FFT pipeline: a frame has no planar mirror");
  const int pad = j->g.pad;
  RC(pr.begin(ICS_K_SYNTH_GRADK));
  HIPCHK(ics_launch_synth_gradk_fft(u, f, e, j->spec_conv, j->g, p->top + pad, p->bottom + pad, p->left + pad, p->right + pad, store_all, j->partial, j->gradk, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

// A11 + A13 in one kernel (matrix-core path, MK <= 15): ics_synth_gradk_mfma.hip
static int do_synth_gradk(ics_rl* j, const Route& r, const ics_rl_params* p, int store_all, Prof& pr) {
  IcsFusedArgs a;
  a.u = org(j, j->u); a.f = org(j, j->f); a.e_out = org(j, j->e); a.bt = j->bt_conv; a.partial = j->partial; a.g = j->g;
  a.wy0 = p->top + j->g.pad; a.wy1 = p->bottom + j->g.pad; a.wx0 = p->left + j->g.pad; a.wx1 = p->right + j->g.pad;
  a.store_all = store_all;
  int nblocks;
  ics_synth_gradk_plan(j->g, j->gradk_blocks, j->fused2_blocks, &a.rs, &nblocks);   // tile height and grid
  a.facc = nullptr;
  if (r.image_acc) { RC(ensure_image_acc(j, a.rs)); a.facc = j->facc[a.rs == 2 ? 0 : 1]; }
  RC(pr.begin(ICS_K_SYNTH_GRADK));
  HIPCHK(ics_launch_synth_gradk(a, nblocks, j->ctx->stream));
  HIPCHK(ics_launch_gradk_reduce(j->partial, nblocks, j->gradk, j->g, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

// A14 ... A17 and the weights of the next convolutions.  Route::psf1 (tile runs): one launch, k_psf_spectra, which steps the PSF and builds
// both spectra -- and nothing else: the row-pair tables wconv / wcorr and the fp16 Toeplitz tables bt_conv / bt_corr, which no tile kernel
// reads, stay as the run's first pack_weights left them.  Everything that reads them packs them first: ics_rl_run before its loop, every
// convolution stage of ics_rl_stage (ICS_STAGE_PSF_UPDATE through k_psf itself), ics_rl_upload / ics_rl_write of a PSF, undo() of the
// overlapped loop and the small-frame fallback in RunLoop::body; a run does not leave the tiles half way, and after an error return
// (FftScope) the next run or stage is one of those.
static int do_psf(ics_rl* j, const Route& r, const ics_rl_params* p, Prof& pr) {
  RC(pr.begin(ICS_K_PSF_UPDATE));
  if (r.psf1) {
    IcsPsfSpectraArgs a;
    a.psf = j->psf; a.psf_next = j->psf_next; a.psf_caller = j->psf_caller; a.gradk = j->gradk; a.scal = j->scal; a.frozen = j->flags;
    a.spec_conv = j->spec_conv; a.spec_corr = j->spec_corr; a.step = p->step_factor; a.K = j->g.K; a.correlation = p->correlation;
    if (!a.spec_conv || !a.spec_corr) return ics_set_error(ICS_ESTATE, "FFT pipeline: no weight spectra");
    HIPCHK(ics_launch_psf_spectra(a, j->ctx->stream));
    { float* t = j->psf; j->psf = j->psf_next; j->psf_next = t; }   // what is queued from here on reads the stepped PSF
  } else
  RC(pack_weights(j, 1, p->step_factor, p->correlation, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

static int do_majorize(ics_rl* j, Prof& pr) {
  j->ut_is_u = false;
  RC(pr.begin(ICS_K_MAJORIZE));
  HIPCHK(hipMemcpyAsync(j->ut, j->u, j->frame_floats * 4, hipMemcpyDeviceToDevice, j->ctx->stream));
  RC(pr.end());
  return ICS_OK;
}

static int do_stats(ics_rl* j, const Route& r, const ics_rl_params* p, Prof& pr, int rearm = 0, hipStream_t st = nullptr) {
  if (!st) st = j->ctx->stream;
  if (j->win_empty) {
    static const float nan3[3] = {nanf(""), nanf(""), nanf("")};   // M_r, Hu, varu
    HIPCHK(hipMemcpyAsync(j->scal + ICS_SC_MR, nan3, sizeof nan3, hipMemcpyHostToDevice, j->ctx->stream));
    return ICS_OK;
  }
  if (r.tiles) {   // A18 / A19 read HWC frames: bring the window of e and u over from the mirrors (u-frame rows [top, bottom + 2 pad); to the
                   // frame's end where the u window's stop is negative and numpy counts it from there, ics_stats.hip make_win)
    const int pad2 = 2 * j->g.pad;
    const int y1 = p->bottom < j->g.pad ? j->g.uM : p->bottom + pad2, x1 = p->right < j->g.pad ? j->g.uN : p->right + pad2;
    HIPCHK(ics_launch_planar_convert(false, pl_of(j, j->e), j->e, j->g, false, p->top, y1, p->left, x1, st));
    HIPCHK(ics_launch_planar_convert(false, pl_of(j, j->u), j->u, j->g, false, p->top, y1, p->left, x1, st));
  }
  IcsStatsArgs a;
  a.e = org(j, j->e); a.u = org(j, j->u); a.scal = j->scal; a.dofkeys = dof_of(j); a.dacc = j->dacc; a.ukey = j->ukey;
  a.z = j->z; a.tw = j->tw; a.weights = j->weights;
  a.top = p->top; a.bottom = p->bottom; a.left = p->left; a.right = p->right;
  a.P = j->P; a.logP = j->logP; a.do_mr = p->stop_test != 0; a.geo = j->g;
  a.Py = j->Py; a.Px = j->Px; a.twy = j->tw; a.twx = j->tw + j->Py;
  a.red = red_of(j); a.rearm = rearm;
  RC(pr.begin(ICS_K_STATS));
  HIPCHK(ics_launch_stats(a, st));
  RC(pr.end());
  return ICS_OK;
}

static int reset_dofkeys(ics_rl* j) {
  static const uint32_t init[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
  HIPCHK(hipMemcpyAsync(j->dofkeys, init, sizeof init, hipMemcpyHostToDevice, j->ctx->stream));
  HIPCHK(hipMemcpyAsync(j->dofkeys + 4, init, sizeof init, hipMemcpyHostToDevice, j->ctx->stream));
  return ICS_OK;
}

// pyx:462-589 for one outer iteration: ut = u (the untouched input frame is the majoriser), INNER inner iterations, u2 receives u
static int do_small_iter(ics_rl* j, const ics_rl_params* p, const IcsSmallPlan& pl, int inner, Prof& pr) {
  IcsSmallArgs a;
  memset(&a, 0, sizeof a);
  a.u_in = org(j, j->u); a.u_out = org(j, j->u2); a.f = org(j, j->f); a.e = org(j, j->e);
  a.red = red_of(j); a.dofkeys = dof_of(j); a.scal = j->scal;
  a.psf = j->psf; a.psf_caller = j->psf_caller; a.frozen = j->flags;
  a.psf_bak = j->small_bak ? j->psf_bak : nullptr;
  a.part = j->small_part; a.keys = j->small_keys; a.gradk = j->gradk; a.bar = j->small_bar; a.bar_gen = j->small_gen;
  a.step = p->step_factor; a.lambd = p->lambd; a.blind = p->blind; a.correlation = p->correlation; a.inner = inner;
  a.plan = pl; a.g = j->g;
  const bool trace = ics_debug().small_trace.load(std::memory_order_relaxed) != 0;
  unsigned long long* tr = nullptr;
  if (trace && dalloc(j->ctx, &tr, (size_t)pl.nwg * 64) == ICS_OK) a.trace = tr;
  RC(pr.begin(ICS_K_SMALL_ITER));
  const hipError_t he = ics_debug().fail_small_launch.exchange(0) ? hipErrorCooperativeLaunchTooLarge : ics_launch_small_iter(a, j->ctx->stream);
  RC(pr.end());
  if (he != hipSuccess) {   // (nothing was queued: the bracket does not count as a launch)
    if (pr.on && !j->ev_pairs.empty()) j->ev_pairs.pop_back();
    return ics_set_error(ICS_EHIP, "cooperative launch of the small-frame iteration: %s", hipGetErrorString(he));
  }
  if (tr) {   // phase timeline: per stamp the first and the last workgroup to reach it, in us from the first stamp of the launch (100 MHz clock)
    std::vector<unsigned long long> h((size_t)pl.nwg * 64);
    HIPCHK(hipStreamSynchronize(j->ctx->stream));
    HIPCHK(hipMemcpy(h.data(), tr, h.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull;
    for (int w = 0; w < pl.nwg; ++w) if (h[(size_t)w * 64] && h[(size_t)w * 64] < t0) t0 = h[(size_t)w * 64];
    fprintf(stderr, "small_trace: %d workgroups, stamp: first / last workgroup (us)\n", pl.nwg);
    fprintf(stderr, "  workgroup 0: %llu shader clocks in %.2f us = %.0f MHz\n", h[62], (double)h[63] / 100.0, h[63] ? (double)h[62] / ((double)h[63] / 100.0) : 0.0);
    for (int k = 0; k < 62; ++k) {
      unsigned long long lo = ~0ull, hi = 0;
      for (int w = 0; w < pl.nwg; ++w) { const unsigned long long v = h[(size_t)w * 64 + k]; if (!v) continue; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
      if (!hi) break;
      fprintf(stderr, "  %2d  %7.2f  %7.2f\n", k, (double)(lo - t0) / 100.0, (double)(hi - t0) / 100.0);
    }
    j->ctx->pool.release(tr);
  }
  j->small_gen += (unsigned long long)ics_small_barriers(p->blind, inner);
  j->small_bak = false;
  // as after the first update of an outer iteration (do_update): the untouched old u is the majoriser, the spare holds u
  float* old_ut = j->ut;
  j->ut = j->u; j->u = j->u2; j->u2 = old_ut;
  j->ut_is_u = false;
  return ICS_OK;
}

// ---- ics_rl_run: validate, prepare the route, reset, loop (drained or overlapped), finish --------------------------------------------
// The route of a run, resolved once (again without the tiles if their mirrors do not fit); the other fallbacks edit it, the overlap decision
// stays.  With what it needs before the first launch: the frames on their planar mirrors, mode 2's image spectra, the small-frame scratch.
static int prepare_route(ics_rl* j, const ics_rl_params* p, FftScope& fft_scope, Route* out) {
  hipStream_t s = j->ctx->stream;
  Route r = resolve_route(j, p, true, true);
  if (r.tiles) {   // the frames live as channel-planar mirrors for the duration of the run (ics_planar.hip)
    j->fft_on = true;
    int rc_pl = ensure_planar(j);
    // the mirrors are 7 - 8 more frame-sized buffers: when they do not fit and the tiles were AUTO's choice, the run goes on on the HWC
    // kernels, which need nothing more (an explicit ICS_CONV_FFT, and the PAM kinds' explicit request, report the failure)
    if (rc_pl == ICS_ENOMEM && p->conv == ICS_CONV_AUTO) { j->fft_on = false; (void)hipGetLastError(); r = resolve_route(j, p, true, false); }
    else if (rc_pl != ICS_OK) return rc_pl;
  }
  if (r.tiles) {
    RC(to_planar(j, j->u, s));
    if (!j->plf_valid) { RC(to_planar(j, j->f, s)); j->plf_valid = true; }
    fft_scope.back = true;
    // mode 2's image spectra are 1.6 frames more (128 KB per unit): when they do not fit, the run takes A1 and A3 as two kernels instead
    if (r.conv2 && !j->fspec && dalloc(j->ctx, &j->fspec, ics_conv2_fft_fspec_floats(j->g), false) != ICS_OK) { j->fspec = nullptr; j->conv2_off = true; r.conv2 = false; (void)hipGetLastError(); }
  }
  // the operand-free mode-2 launches: a few state words and the tile maxima of a launch; where they do not fit, the run keeps k_conv_fft<2>
  j->mgs_ready = false; j->mgs_set = 0;
  if (r.maxg && !r.conv2) r.maxg = false;
  if (r.maxg) {
    if (!j->mgs && dalloc(j->ctx, &j->mgs, (size_t)ICS_MGS_WORDS, false) != ICS_OK) { j->mgs = nullptr; r.maxg = false; (void)hipGetLastError(); }
    if (r.maxg && !j->mgs_wave && dalloc(j->ctx, &j->mgs_wave, (size_t)ics_conv2_fft_units(j->g) * 2 * ICS_MGS_WAVES, false) != ICS_OK) { j->mgs_wave = nullptr; r.maxg = false; (void)hipGetLastError(); }
    if (r.maxg) HIPCHK(hipMemsetAsync(j->mgs, 0, (size_t)ICS_MGS_WORDS * sizeof(uint32_t), s));
  }
  if (r.small && ensure_small(j, r.plan) != ICS_OK) { r.small = false; (void)hipGetLastError(); }   // (AUTO's choice: the multi-launch path needs nothing more)
  if (r.small) { HIPCHK(hipMemsetAsync(j->small_bar, 0, (size_t)ICS_SMALL_BAR_WORDS * sizeof(unsigned long long), s)); j->small_gen = 0; j->small_bak = false; }
  *out = r;
  return ICS_OK;
}

namespace {
// The outer loop of one ics_rl_run call (pyx:460) and its state
struct RunLoop {
  static constexpr int INNER = 5;       // pyx:375
  ics_rl* j; const ics_rl_params* p; ics_rl_stats* st;
  Route r;                              // (body() takes `small` back when the runtime refuses the cooperative launch)
  hipStream_t s; bool tv;               // the job's stream; a TV variant (tv_mode != 0)
  Prof pr_on, pr_off;                   // (per-outer kernels are always bracketed when profiling)
  double ms[ICS_KERNEL_COUNT] = {0}; int launches[ICS_KERNEL_COUNT] = {0};
  int it = 0, stop = 0, inner_done = 0; // `it` = outer iterations whose scalars were consumed
  float M_r = 0.f, M_r_prev = 0.f, Hu = 0.f, varu = 0.f, dmin = 0.f, dmax = 0.f;
  hipStream_t st2 = nullptr;            // overlapped loop only: where the statistics run, ...
  size_t npsf = 0, ev_mark[2] = {0, 0}; int enq = 0;   // ... the floats of a PSF, where the brackets of [i & 1] end, the outer iterations queued
  // the launches of one outer iteration (pyx:462-591) ...
  int body() {
    j->ev_chain = -1;
    if (p->fuse) RC(do_majorize(j, pr_on));                   // pyx:462 (explicit copy only for the fused path)
    else j->ut_is_u = true;                                   // pyx:462 without a copy (see ut_of)
    if (r.small) {   // one cooperative launch for the INNER inner iterations (ics_small.hip)
      if (do_small_iter(j, p, r.plan, INNER, p->profile > 0 ? pr_on : pr_off) == ICS_OK) { inner_done += INNER; return ICS_OK; }
      r.small = false; j->small_off = true; (void)hipGetLastError();   // refused by the runtime: this job runs the multi-launch path from here on
      RC(pack_weights(j, 0, 0.f, 0, s));   // (the weight tables of the multi-launch kernels follow the PSF the cooperative launches have stepped so far)
      if (j->small_bak) {   // (the copy of the PSF the refused launch was to take)
        const size_t npsf = (size_t)3 * j->g.K * j->g.K;
        HIPCHK(hipMemcpyAsync(j->psf_bak, j->psf, npsf * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(j->psf_bak + npsf, j->psf_caller, npsf * 4, hipMemcpyDeviceToDevice, s));
        j->small_bak = false;
      }
    }
    const bool fuse = p->fuse != 0;
    const bool fused_gk = r.gradk == GK_FUSED_MATRIX, fused_fft = r.gradk == GK_FUSED_TILES;
    // (mode 2 of the tiles, blind without the fused A11 + A13 unit: A11 rewrites the whole residual frame, nothing more to do; either way the window is there)
    bool have_e = false;  // error already produced by a fused update+synth kernel
    for (int itt = 0; itt < INNER; ++itt) {                   // pyx:473
      const int last = itt == INNER - 1;
      // profile = k: bracket the launches of every k-th inner iteration only (k = 1: all).  Event records
      // between dependent kernels cost ~4 % of a 4096^2 blind iteration, a sample of them does not.
      Prof& pr = (p->profile > 0 && inner_done % p->profile == 0) ? pr_on : pr_off;
      if (r.conv2) {
        if (tv) RC(do_tvterm(j, r, p, itt, pr));              // (PAM kinds: T of u, read by the back-projection's epilogue)
        RC(do_conv2(j, r, p, itt, pr));                       // A1 + A2 + A3 (+A7) in one unit per tile pair; the residual frame is not written ...
        if (!p->blind && last) RC(do_conv_fft_window(j, p, pr));   // ... so the statistics' window of it is (blind: A11 rewrites it, do_synth_gradk_fft)
      } else {
      if (!have_e) RC(do_conv(j, r, 0, p, itt, 0, pr));       // A1+A2
      have_e = false;
      if (tv) RC(do_tvterm(j, r, p, itt, pr));                // pyx:495-496 (live only in tv_mode 1)
      RC(do_conv(j, r, 1, p, itt, 0, pr));                    // A3 (+A7)
      }
      if (p->blind) {                                         // pyx:555
        if (fuse) RC(do_conv(j, r, 2, p, itt, last, pr));     // A5-A10 fused with A11
        else {
          RC(do_update(j, r, p, itt, last, pr, last));
          if (fused_gk) RC(do_synth_gradk(j, r, p, 0, pr));   // A11 + A12 + A13, e' stays on chip
          else if (fused_fft) RC(do_synth_gradk_fft(j, p, 0, pr));   // the same on the transform tiles
          else RC(do_conv(j, r, 0, p, itt, 0, pr));
        }
        if (!(fused_gk || fused_fft)) RC(do_gradk(j, r, pr));   // A12+A13
        RC(do_psf(j, r, p, pr));                              // A14-A17
      } else if (fuse && !last) {
        RC(do_conv(j, r, 2, p, itt, 0, pr));                  // A5-A10 fused with A1+A2 of itt+1
        have_e = true;
      } else {
        RC(do_update(j, r, p, itt, last, pr, last));          // A5,A6,A8,A10 (outer boundary: stats need u and e)
      }
      ++inner_done;
    }
    return ICS_OK;
  }
  // ... and its statistics (A18 + A19) with the copy of the scalars to the pinned host mirror `hs`, on stream `on`
  int stats(hipStream_t on, float* hs, Prof& prs) {
    RC(do_stats(j, r, p, prs, 1, on));
    HIPCHK(hipMemcpyAsync(hs, j->scal, ICS_SC_COUNT * 4, hipMemcpyDeviceToHost, on));
    return ICS_OK;
  }
  // what the host does once the scalars of an outer iteration are in `hs`: traces, stop decision (pyx:643-654), progress callback
  void consume(const float* hs) {
    if (it > 0) M_r_prev = M_r;                               // pyx:623-624
    M_r = p->stop_test ? hs[ICS_SC_MR] : nanf("");
    Hu = hs[ICS_SC_HU]; varu = hs[ICS_SC_VARU];
    dmin = hs[ICS_SC_DOFMIN]; dmax = hs[ICS_SC_DOFMAX];
    if (it < st->trace_cap) {
      if (st->trace_M_r) st->trace_M_r[it] = M_r;
      if (st->trace_Hu) st->trace_Hu[it] = Hu;
      if (st->trace_varu) st->trace_varu[it] = varu;
      if (st->trace_dof_min) st->trace_dof_min[it] = dmin;
      if (st->trace_dof_max) st->trace_dof_max[it] = dmax;
      st->trace_len = it + 1;
    }
    if (it > 1 && p->stop_test == 1) {                        // pyx:643-654 (stop_test 2: evaluate only)
      if (p->blind) { if (M_r > M_r_prev) stop = 1; }
      else { if ((M_r - M_r_prev) / (M_r + M_r_prev) > p->tau) stop = 1; }
    }
    ++it;
    // pyx:593,648,658-659: where the reference prints.  A non-zero return leaves the loop with the state of this outer iteration
    // (deconvolve.py:338-342 keeps the partial result of an interrupted run)
    if (p->progress && p->progress(p->progress_user, it, stop, dmin, dmax, M_r, Hu, varu) != 0 && !stop) stop = 2;
  }
  // a drain at every outer boundary: body, statistics, wait, decide
  int drained() {
    while (it < p->iterations && !stop) {                       // pyx:460
      if (j->win_empty && it > 0) {   // (no statistics kernel re-arms them for an empty window)
        HIPCHK(hipMemsetAsync(j->red, 0, 8 * ICS_RED_STRIDE * sizeof(uint32_t), s));
        RC(reset_dofkeys(j));
      }
      RC(body());
      RC(stats(s, j->h_scal, pr_on));
      // (the wait's wake-up is not what the device idles on here: an event before the statistics + polling through them measured the
      //  same iteration time, 0.8178 vs 0.8185 ms at 4096^2 and 0.1573 vs 0.1562 at 2048^2 non-blind)
      HIPCHK(hipStreamSynchronize(s));
      RC(pr_on.collect(ms, launches));
      consume(j->h_scal);
    }
    return ICS_OK;
  }
  // overlapped loop: drops iteration enq - 1 (queued, possibly running)
  int undo() {
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipStreamSynchronize(st2));
    { float* t = j->u; j->u = j->ut; j->ut = t; }           // the majoriser frame of the dropped iteration is u of the one before
    { float* t = j->e; j->e = j->e2; j->e2 = t; }
    if (p->blind) {
      HIPCHK(hipMemcpyAsync(j->psf, j->psf_bak, npsf * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(j->psf_caller, j->psf_bak + npsf, npsf * 4, hipMemcpyDeviceToDevice, s));
      RC(pack_weights(j, 0, 0.f, 0, s));
    }
    inner_done -= INNER;
    // the dropped iteration's event brackets do not enter ms_kernel[] / launches[] (they describe iterations that count); its device time
    // stays inside ms_total, which is the span of the whole call
    if (enq >= 2 && j->ev_pairs.size() > ev_mark[(enq - 2) & 1]) j->ev_pairs.resize(ev_mark[(enq - 2) & 1]);
    return ICS_OK;
  }
  // ---- statistics of iteration i on a second stream, iteration i + 1 already running on the job's stream (round 4) -------------------
  // The stop decision of iteration i needs M_r(i) on the host, so until round 3 the device drained at every outer boundary: five
  // small dependent kernels (0.06 ms) and a round trip with nothing else in flight -- a quarter of a 512^2 step, 7 % at 2048^2.
  // Now iteration i + 1 is queued before M_r(i) is known.  What that needs: iteration i + 1 may not touch what the statistics of i
  // read or re-arm -- the residual frame ping-pongs (e / e2), the reduction slots and DoF keys come in two sets (i & 1), u(i) is
  // the untouched majoriser of i + 1 anyway (frame rotation) -- and, if the stop test fires at i (or the callback asks to stop),
  // iteration i + 1 is undone: its u is dropped for the majoriser frame (= u(i)), the PSF comes back from the copy taken when i + 1
  // started.  At most one outer iteration is ever ahead, and only the run's last decision costs a wasted one.
  int overlapped() {
    ics_ctx* c = j->ctx;
    if (!c->stream2) {   // lowest priority: the statistics take what the iteration's kernels leave free
      int lo = 0, hi = 0;
      HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIPCHK(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo));
    }
    if (!j->ev_body[0])
      for (int i = 0; i < 2; ++i) { HIPCHK(hipEventCreateWithFlags(&j->ev_body[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&j->ev_stats[i], hipEventDisableTiming)); }
    if (!j->e2) RC(dalloc(c, &j->e2, j->frame_floats));
    if (r.tiles) RC(ensure_planar(j));                       // (a mirror for e2 as well)
    npsf = (size_t)3 * j->g.K * j->g.K;
    if (p->blind && !j->psf_bak) RC(dalloc(c, &j->psf_bak, 2 * npsf, false));
    st2 = c->stream2;
    Prof pr_s2{j, p->profile != 0, st2};
    size_t ev_done = 0;
    while (enq < p->iterations && !stop) {                    // pyx:460
      j->par = enq & 1;
      if (enq > 0) {
        { float* t = j->e; j->e = j->e2; j->e2 = t; }         // the statistics of the previous iteration read the other frame
        if (p->blind && r.small) j->small_bak = true;           // (the cooperative kernel takes the copy itself: two launches and a queue switch less per outer iteration)
        else if (p->blind) {
          HIPCHK(hipMemcpyAsync(j->psf_bak, j->psf, npsf * 4, hipMemcpyDeviceToDevice, s));
          HIPCHK(hipMemcpyAsync(j->psf_bak + npsf, j->psf_caller, npsf * 4, hipMemcpyDeviceToDevice, s));
        }
      }
      RC(body());
      HIPCHK(hipEventRecord(j->ev_body[enq & 1], s));
      HIPCHK(hipStreamWaitEvent(st2, j->ev_body[enq & 1], 0));
      RC(stats(st2, j->h_scal + (enq & 1) * (ICS_SC_COUNT + 4), pr_s2));
      HIPCHK(hipEventRecord(j->ev_stats[enq & 1], st2));
      ev_mark[enq & 1] = j->ev_pairs.size();
      j->ev_chain = -1;
      ++enq;
      if (enq >= 2) {                                         // the scalars of the iteration BEFORE the one just queued
        HIPCHK(hipEventSynchronize(j->ev_stats[(enq - 2) & 1]));
        RC(pr_on.collect_range(ms, launches, ev_done, ev_mark[(enq - 2) & 1]));
        consume(j->h_scal + ((enq - 2) & 1) * (ICS_SC_COUNT + 4));
        if (stop) RC(undo());
      }
    }
    if (!stop && enq > it) {                                  // the last iteration's scalars (nothing is ahead of it)
      HIPCHK(hipEventSynchronize(j->ev_stats[(enq - 1) & 1]));
      consume(j->h_scal + ((enq - 1) & 1) * (ICS_SC_COUNT + 4));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipStreamSynchronize(st2));
    RC(pr_on.collect_range(ms, launches, ev_done, j->ev_pairs.size()));
    j->ev_used = 0; j->ev_pairs.clear(); j->ev_chain = -1;
    j->par = 0;
    return ICS_OK;
  }
};
}  // namespace

extern "C" int ics_rl_run(ics_rl* j, const ics_rl_params* p, ics_rl_stats* st) {
  if (!st) return ics_set_error(ICS_EINVAL, "stats is NULL");
  if (p && p->struct_size == sizeof(ics_rl_params) && st->struct_size != sizeof(ics_rl_stats))
    return ics_set_error(ICS_EINVAL, "ics_rl_stats.struct_size = %u but this library (ABI %d) expects %zu", st->struct_size, ICS_ABI_VERSION, sizeof(ics_rl_stats));
  RC(check_params(j, p));
  if (st->trace_cap < 0) return ics_set_error(ICS_EINVAL, "ics_rl_stats.trace_cap = %d", st->trace_cap);
  if (!j->uploaded) return ics_set_error(ICS_ESTATE, "ics_rl_run before ics_rl_upload");
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  RC(ensure_window(j, p));
  const bool tv = p->tv_mode != ICS_TV_SHIPPED;
  if (tv) RC(ensure_tv(j));
  // whatever path leaves this function: the statistics' stream is drained before the caller can release or reuse the job's buffers (an
  // error return inside the overlapped loop used to skip the drain), and the FFT pipeline's flag is cleared
  struct Drain { ics_ctx* c; ~Drain() { if (c->stream2) (void)hipStreamSynchronize(c->stream2); } } drain{j->ctx};
  FftScope fft_scope{j};
  Route r;
  RC(prepare_route(j, p, fft_scope, &r));
  {  // everything but the caller's in-fields is overwritten
    ics_rl_stats in = *st;
    memset(st, 0, sizeof *st);
    st->struct_size = in.struct_size; st->trace_cap = in.trace_cap;
    st->trace_M_r = in.trace_M_r; st->trace_Hu = in.trace_Hu; st->trace_varu = in.trace_varu; st->trace_dof_min = in.trace_dof_min; st->trace_dof_max = in.trace_dof_max;
  }
  j->ut_is_u = false;
  j->ktrace_n = 0;
  if (ics_debug().key_trace.load(std::memory_order_relaxed)) {
    if (!j->ktrace) RC(dalloc(j->ctx, &j->ktrace, (size_t)ICS_KEY_TRACE_SLOTS * ICS_RED_STRIDE));
  } else if (j->ktrace) { j->ctx->pool.release(j->ktrace); j->ktrace = nullptr; }
  RunLoop run{j, p, st, r, s, tv, Prof{j, p->profile != 0}, Prof{j, false}};
  j->ev_used = 0; j->ev_pairs.clear(); j->ev_chain = -1;
  {   // the job's small state in one launch: flags, the tile counters (the kernels re-arm them; an aborted launch must not leak a count), the
      // accumulators of the window statistics (likewise re-armed by their last kernel), both sets of reduction slots and DoF keys (later
      // outer iterations: re-armed on the device by the kernel that writes the scalars), and the scalars: a run that writes no dtpsf (non-blind)
      // reports 0 for it on a job whose last run was blind as on a fresh one (tests/test_gpu_job_reuse.py)
    IcsRunResetArgs ra;
    ra.flags = j->flags; ra.sched = j->sched; ra.dacc = j->dacc; ra.ukey = j->ukey; ra.red = j->red; ra.nred = 2 * 8 * ICS_RED_STRIDE; ra.dofkeys = j->dofkeys;
    ra.scal = j->scal;
    HIPCHK(ics_launch_run_reset(ra, s));
  }
  // the caller's psf array is the local psf when the call starts (pyx:341)
  HIPCHK(hipMemcpyAsync(j->psf_caller, j->psf, (size_t)3 * j->g.K * j->g.K * 4, hipMemcpyDeviceToDevice, s));
  RC(pack_weights(j, 0, 0.f, 0, s));
  HIPCHK(hipEventRecord(j->ev_begin, s));
  j->par = 0;
  RC(run.r.overlap ? run.overlapped() : run.drained());
  if (run.r.tiles) { RC(from_planar(j, j->u, s)); RC(from_planar(j, j->e, s)); fft_scope.back = false; }   // the HWC frames are the job's state between calls
  HIPCHK(ics_launch_hasnan(org(j, j->u), j->g, j->flags + 1, s));
  HIPCHK(hipEventRecord(j->ev_end, s));
  int hflags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hflags, j->flags, sizeof hflags, hipMemcpyDeviceToHost, s));
  uint32_t hmgs[4] = {0u, 0u, 0u, 0u};   // (Route::maxg: the selection kernel's counts, reported through the debug interface)
  if (run.r.maxg) HIPCHK(hipMemcpyAsync(hmgs, j->mgs + ICS_MGS_SCANNED, sizeof hmgs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (run.r.maxg) {
    IcsDebug& d = ics_debug();
    IcsMaxgSelectArgs m;
    ics_conv2_fft_select_grid(j->g, &m);
    d.maxg_scanned.store(hmgs[3] ? (int)hmgs[j->mgs_set ^ 1] : -1, std::memory_order_relaxed);      // (the set of the last launch: do_conv2 has moved on)
    d.maxg_pairs.store(3 * m.ntiles, std::memory_order_relaxed);
    d.maxg_total.store((int)hmgs[2], std::memory_order_relaxed); d.maxg_launches.store((int)hmgs[3], std::memory_order_relaxed);
  } else if (run.r.conv2) {   // (a mode-2 run on the operand-reading launches)
    IcsDebug& d = ics_debug();
    d.maxg_scanned.store(-1, std::memory_order_relaxed); d.maxg_total.store(0, std::memory_order_relaxed); d.maxg_launches.store(0, std::memory_order_relaxed);
  }
  float total = 0.f;
  HIPCHK(hipEventElapsedTime(&total, j->ev_begin, j->ev_end));
  st->iterations_done = run.it; st->stopped = run.stop; st->has_nan = hflags[1];
  st->M_r = run.M_r; st->Hu = run.Hu; st->varu = run.varu; st->dof_min = run.dmin; st->dof_max = run.dmax;
  st->ms_total = total; st->inner_iterations = run.inner_done;
  for (int k = 0; k < ICS_KERNEL_COUNT; ++k) {
    st->launches[k] = run.launches[k];
    st->ms_kernel[k] = run.launches[k] ? (float)(run.ms[k] / run.launches[k]) : 0.f;
  }
  return ICS_OK;
}

extern "C" int ics_rl_stage(ics_rl* j, int stage, const ics_rl_params* p) {
  RC(check_params(j, p));
  if (p->conv == ICS_CONV_FFT && p->tv_mode != ICS_TV_SHIPPED)
    return ics_set_error(ICS_ENOSUP, "ICS_CONV_FFT with tv_mode %d: single stages of the PAM kinds run on the HWC kernels (the tiles serve ics_rl_run)", p->tv_mode);
  j->par = 0;
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  Prof pr{j, false};
  HIPCHK(hipMemsetAsync(j->sched, 0, 16 * sizeof(uint32_t), s));
  // conv = ICS_CONV_FFT through the stage API (tests): the stage runs on the mirrors, every frame is copied over before and the frames a
  // stage writes are copied back after -- slow and simple; ics_rl_run converts at its boundaries only
  FftScope fft_scope{j};
  const bool tile_stage = stage == ICS_STAGE_SYNTH_RESIDUAL || stage == ICS_STAGE_BACKPROJECT || stage == ICS_STAGE_UPDATE || stage == ICS_STAGE_PSF_GRADIENT ||
                          stage == ICS_STAGE_PSF_UPDATE || stage == ICS_STAGE_SYNTH_GRADK || stage == ICS_STAGE_SYNTH_BACKPROJECT;
  const Route r = resolve_route(j, p, false, tile_stage);
  if (r.tiles) {
    j->fft_on = true;
    RC(ensure_planar(j));
    for (float* h : {j->u, j->ut, j->gr, j->f, j->e}) RC(to_planar(j, h, s));
    j->plf_valid = true;
  }
  struct StageBack {   // (runs before fft_scope clears the flag: declared after it)
    ics_rl* j; bool on; hipStream_t s;
    ~StageBack() { if (on) { for (float* h : {j->u, j->gr, j->e}) (void)from_planar(j, h, s); (void)hipStreamSynchronize(s); } }
  } stage_back{j, r.tiles, s};
  switch (stage) {
    case ICS_STAGE_SYNTH_RESIDUAL:
      RC(pack_weights(j, 0, 0.f, 0, s));
      RC(do_conv(j, r, 0, p, 0, 0, pr));
      break;
    case ICS_STAGE_BACKPROJECT:
      RC(pack_weights(j, 0, 0.f, 0, s));
      // (in tv_mode 1 ICS_STAGE_TVTERM runs first and owns the reset: its keys live in the same slot)
      if (p->tv_mode == ICS_TV_SHIPPED) HIPCHK(hipMemsetAsync(j->red, 0, 8 * ICS_RED_STRIDE * sizeof(uint32_t), s));
      else RC(ensure_tv(j));
      RC(do_conv(j, r, 1, p, 0, 0, pr));
      break;
    case ICS_STAGE_UPDATE:
      RC(reset_dofkeys(j));
      RC(do_update(j, r, p, 0, 1, pr));
      break;
    case ICS_STAGE_TVTERM:
      if (p->tv_mode == ICS_TV_SHIPPED) return ics_set_error(ICS_EINVAL, "ICS_STAGE_TVTERM needs tv_mode != ICS_TV_SHIPPED");
      RC(ensure_tv(j));
      HIPCHK(hipMemsetAsync(j->red, 0, 8 * ICS_RED_STRIDE * sizeof(uint32_t), s));
      RC(do_tvterm(j, r, p, 0, pr));
      break;
    case ICS_STAGE_UPDATE_SYNTH:
      RC(pack_weights(j, 0, 0.f, 0, s));
      RC(reset_dofkeys(j));
      RC(do_conv(j, r, 2, p, 0, 1, pr));
      break;
    case ICS_STAGE_PSF_GRADIENT: RC(do_gradk(j, r, pr)); break;
    case ICS_STAGE_BAND_REDUCE:
      if (p->tv_mode != ICS_TV_SHIPPED) return ics_set_error(ICS_ENOSUP, "row bands are built for the shipped loop (tv_mode 0)");
      if (p->band_row0 < 0 || p->band_row1 > j->g.uM || p->band_row0 >= p->band_row1) return ics_set_error(ICS_EINVAL, "band rows [%d, %d) outside the %d u rows", p->band_row0, p->band_row1, j->g.uM);
      HIPCHK(hipMemsetAsync(j->red, 0, ICS_RED_STRIDE * sizeof(uint32_t), s));
      HIPCHK(ics_launch_band_reduce(org(j, j->gr), org(j, j->u), org(j, ut_of(j)), j->g, p->lambd, p->band_row0, p->band_row1, j->red, s));
      break;
    case ICS_STAGE_BAND_MASK_E:
      if (p->band_row0 < 0 || p->band_row1 > j->g.M || p->band_row0 > p->band_row1) return ics_set_error(ICS_EINVAL, "band rows [%d, %d) outside the %d image rows", p->band_row0, p->band_row1, j->g.M);
      HIPCHK(ics_launch_band_mask_e(org(j, j->e), j->g, p->band_row0, p->band_row1, s));
      break;
    case ICS_STAGE_SYNTH_GRADK:
      if (r.tiles && !ics_conv_fft_supported(j->g.K)) return ics_set_error(ICS_ENOSUP, "ICS_STAGE_SYNTH_GRADK on the tiles: the fused unit is built for PSF sizes that fit one tile (<= 85); above, A11 and A13 run as tap blocks");
      if (r.tiles) {   // conv = ICS_CONV_FFT: the fused unit of the transform tiles, every tile stores its residual
        RC(pack_weights(j, 0, 0.f, 0, s));
        RC(do_synth_gradk_fft(j, p, 1, pr));
        break;
      }
      if (!ics_synth_gradk_supported(j->g.K) || !j->bt_conv) return ics_set_error(ICS_ENOSUP, "ICS_STAGE_SYNTH_GRADK is built for PSF sizes <= 15");
      RC(pack_weights(j, 0, 0.f, 0, s));
      RC(do_synth_gradk(j, r, p, 1, pr));
      break;
    case ICS_STAGE_SYNTH_BACKPROJECT:
      if (!r.tiles || p->tv_mode != ICS_TV_SHIPPED || !ics_conv2_fft_supported(j->g))
        return ics_set_error(ICS_ENOSUP, "ICS_STAGE_SYNTH_BACKPROJECT needs params.conv = ICS_CONV_FFT, tv_mode 0 and a PSF of at most 57 x 57");
      RC(pack_weights(j, 0, 0.f, 0, s));
      HIPCHK(hipMemsetAsync(j->red, 0, 8 * ICS_RED_STRIDE * sizeof(uint32_t), s));
      RC(do_conv2(j, r, p, 0, pr));
      break;
    case ICS_STAGE_PSF_UPDATE: RC(do_psf(j, r, p, pr)); break;
    case ICS_STAGE_MAJORIZE: RC(do_majorize(j, pr)); break;
    case ICS_STAGE_STATS:
      HIPCHK(hipMemsetAsync(j->dacc, 0, 8 * sizeof(double), s));
      HIPCHK(hipMemsetAsync(j->ukey, 0, 2 * sizeof(uint32_t), s));
      RC(ensure_window(j, p));
      RC(do_stats(j, r, p, pr));
      break;
    default: return ics_set_error(ICS_EINVAL, "unknown stage %d", stage);
  }
  if (!(p->flags & ICS_FLAG_STAGE_ASYNC)) HIPCHK(hipStreamSynchronize(s));
  return ICS_OK;
}
