// ics_route.hip -- which kernels a run or a stage launches: the parameter checks, the routing table (resolve_route; ics_host.h Route) and
// the entries of the C ABI (include/ics_hip.h) that report it.  The only unit that reads the routing switches; it makes no HIP call.
#include "ics_host.h"

using namespace ics_host;

// -------------------------------------------------------------------------------------------------
// PSF sizes 129 ... ICS_PSF_MAX: only as tap blocks on the matrix cores -- convolutions as blocks of <= 33 x 33 taps (do_conv_blocks), the
// gradient as blocks of <= 31 x 31 (do_gradk_split); the run-time-sized fp32 kernels of ics_big.hip (ICS_CONV_VECTOR) stop at 127.
bool ics_host::psf_blocks_only(int K) { return K > 127 && K <= ICS_PSF_MAX && (K & 1); }
bool ics_host::psf_supported(int K) { return ics_conv_supported(K) || ics_big_supported(K) || psf_blocks_only(K); }

// ---- routing ------------------------------------------------------------------------------------------------------------------------
// Which kernels a run or a stage launches is decided in ONE place, resolve_route (below check_params), from the geometry, the parameters,
// the weight tables the job owns, its sticky fallbacks and the routing switches (ics_common.h IcsDebug: conv_path, fused_gradk,
// planar_image, fft_gradk, fft_fused, fft_conv2, fft_psf1, fft_maxg, small_iter, overlap -- read nowhere else).  ics_rl_run and ics_rl_stage resolve it once and
// hand it to the do_* helpers, which dispatch on it; ics_rl_describe copies it.  Family numbers: those of ics_rl_route (include/ics_hip.h); the Route itself: ics_host.h.

// The FFT-tile pipeline (ics_conv_fft.hip; round 5): A1 / A3 / A11 as LDS-resident 128 x 128 overlap-save transforms on planar mirrors,
// fp32 throughout, with the update pass and the matrix-core PSF gradient on the mirrors as well.  Shipped loop only (tv_mode 0, fuse 0),
// PSF sizes 3 ... 65.  Explicit: conv = ICS_CONV_FFT (also through the stage API); under ICS_CONV_AUTO inside ics_rl_run where it measured
// ahead of the matrix-core kernels (fft_preferred); ICS_CONV_PATH=fft|matrix|vector overrides AUTO.
// (PSF sizes 67 ... 97, opened to the tiles late in round 6 -- the stage functions never depended on the size, only the valid part of a tile
//  shrinks: 62 pixels a side at 67, 32 at 97 -- against the matrix cores' tap blocks, profiles/r06_ab_fft_bigk.txt, non-blind / blind:
//  1024^2 67: 0.659 -> 0.160 / 1.270 -> 0.332;  2048^2 67: 1.894 -> 0.333 / 3.621 -> 0.609;  97: 2.455 -> 0.793 / 5.182 -> 1.494;
//  4096^2 67: 6.774 -> 1.059 / 12.78 -> 1.746;  85: 7.822 -> 1.676 / 14.43 -> 2.895;  97: 9.011 -> 2.848 / 18.46 -> 4.989)
static constexpr int ICS_FFT_AUTO_MAX_K = 85;
static constexpr long ICS_FFT_BLK_MIN_PX = 500000L;
static bool fft_preferred(const IcsGeom& g, bool blind) {
  // measured on MI355X (NOTES_r05.md): per-pass time of the transform tiles is set by the tile count (128 - K + 1 valid pixels a side),
  // the Toeplitz matrix-core kernels pay K^2.  scripts/ab_fft.py at the end of round 5, ms per inner iteration, matrix cores -> tiles
  // (non-blind / blind):  1024^2 31: 0.118 -> 0.146 / 0.251 -> 0.192;  1448^2 21: 0.162 -> 0.149 / 0.272 -> 0.252;  31: 0.198 -> 0.131 / 0.331 -> 0.248;
  // 2048^2 17: 0.168 -> 0.183 / level;  19: 0.257 -> 0.181 / 0.427 -> 0.324;  4096^2 15: level / 0.848 -> 0.944 (the fused A11 + A13 kernel);
  // 17: 0.616 -> 0.599 / 1.104 -> 0.937;  19: 0.901 -> 0.597 / 1.545 -> 0.936;  6144^2 17: 1.285 -> 1.233 / 2.388 -> 1.836.
  // Round 6, with A11 + A13 fused into one three-transform unit (k_synth_gradk_fft), scripts/ab_fft.py, matrix cores -> tiles (non-blind / blind):
  // 2048^2 15: 0.164 -> 0.185 / 0.237 -> 0.284 (three rounds of units where 2.004 would do);  17: 0.170 -> 0.183 / 0.315 -> 0.286;  1448^2 17: blind 0.195 -> 0.187;
  // 2900^2 15: level / 0.455 -> 0.431;  17: 0.341 -> 0.311 / 0.576 -> 0.433;  4096^2 9: 0.512 -> 0.574 / 0.730 -> 0.764;  13: level / 0.790 -> 0.766;
  // 15: 0.593 -> 0.579 / 0.834 -> 0.785;  6144^2 15: 1.262 -> 1.199 / 1.835 -> 1.680;  8192^2 15: level / 3.256 -> 2.947.
  // ... and with A1 + A3 as one unit per tile pair as well (mode 2, PSF sizes <= 25), profiles/r06_ab_fft.txt (a slow box: the matrix-core blind 4096^2 / 15 line is 0.851 there):
  // 1448^2 15: 0.097 -> 0.114 / 0.154 -> 0.165;  17: level / 0.195 -> 0.156;  2048^2 9: 0.141 -> 0.158 / 0.210 -> 0.230;  13: level / level;  15: 0.169 -> 0.154 / 0.237 -> 0.250;
  // 17: 0.170 -> 0.151 / 0.315 -> 0.248;  2900^2 9: 0.286 -> 0.265 / 0.403 -> 0.363;  15: 0.332 -> 0.296 / 0.457 -> 0.400;  4096^2 5: level / 0.683 -> 0.643;  9: 0.532 -> 0.479 /
  // 0.732 -> 0.662;  15: 0.627 -> 0.526 / 0.851 -> 0.716;  6144^2 9: 1.140 -> 0.999 / 1.622 -> 1.365;  15: 1.256 -> 1.122 / 1.821 -> 1.502.
  const long px = (long)g.uM * g.uN;
  if (g.K > ICS_FFT_AUTO_MAX_K) return ics_conv_fft_blk_supported(g.K) && px >= ICS_FFT_BLK_MIN_PX;      // tap blocks on the tiles
  if (g.K >= 51) return px >= 500000L;
  if (g.K >= 19) return px >= (blind ? 1000000L : 1500000L);
  if (g.K == 17) return px >= (blind ? 2000000L : 4000000L);
  if (g.K == 15) return px >= (blind ? 6000000L : 4000000L);
  if (g.K >= 9) return px >= 6000000L;
  return px >= 12000000L;
}
// The tile kernels address a channel-planar mirror through ONE raw buffer resource with 32-bit byte offsets (ics_conv_fft.hip make_gbuf:
// num_records 2^31 - 1).  A mirror's rows are padded to 64 floats per plane, so for some shapes it is a little LARGER than the HWC frame it
// mirrors: a frame accepted just under the 2 GiB frame limit can have a mirror whose last plane ends beyond 2^31 bytes -- loads there
// would read 0, stores would be dropped, silently (e.g. 18784 x 9256 with a 33 x 33 PSF).  Such shapes never take the tiles.
static bool fft_mirror_fits(const IcsGeom& g) { return ics_planar_floats(g) * sizeof(float) < 0x7FFFFFFFull; }

// Mode 2 of the tiles (A1 + A2 + A3 in one unit per tile pair, do_conv2 in ics_run.hip) pays for small PSFs: up to this size under AUTO.
// scripts/ab_conv2.py on MI355X, ms per inner iteration, two kernels -> one unit (non-blind / blind): 1024^2 9: 0.093 -> 0.080 / 0.144 -> 0.125;  15: 0.101 -> 0.085 /
// 0.156 -> 0.136;  25: 0.109 -> 0.100 / 0.172 -> 0.161;  2048^2 15: 0.186 -> 0.154 / 0.293 -> 0.250;  21: 0.187 -> 0.178 / 0.294 -> 0.281;  25: 0.201 -> 0.175 / 0.319 -> 0.283;
// 31: 0.184 -> 0.230 / 0.306 -> 0.351;  4096^2 9: 0.572 -> 0.470 / 0.775 -> 0.668;  15: 0.581 -> 0.518 / 0.797 -> 0.714 (another box: 0.576 -> 0.485 / 0.794 -> 0.686);
// 21: 0.600 -> 0.561 / 0.828 -> 0.774;  25: level / 0.867 -> 0.859;  31: 0.636 -> 0.735 / 0.909 -> 0.990.
static constexpr int ICS_CONV2_MAX_K = 25;
static constexpr long ICS_MAXG_MIN_PX = 6000000L;   // mode 2 without the epilogue's operand reads (Route::maxg): u-frame pixels from which it is the default

int ics_host::check_params(ics_rl* j, const ics_rl_params* p) {
  if (!p) return ics_set_error(ICS_EINVAL, "params is NULL");
  if (p->struct_size != sizeof(ics_rl_params))   // first of all: nothing else of *p may be trusted otherwise
    return ics_set_error(ICS_EINVAL, "ics_rl_params.struct_size = %u but this library (ABI %d) expects %zu: the caller was built against another include/ics_hip.h",
                p->struct_size, ICS_ABI_VERSION, sizeof(ics_rl_params));
  if (!j) return ics_set_error(ICS_EINVAL, "job is NULL");
  if (p->tv_mode < ICS_TV_SHIPPED || p->tv_mode > ICS_TV_PAM_COLLAB)
    return ics_set_error(ICS_ENOSUP, "tv_mode %d not implemented (0 shipped, 1 active MM-TV, 2 PAM isotropic, 3 PAM collaborative)", p->tv_mode);
  if (p->tv_mode != ICS_TV_SHIPPED && p->fuse) return ics_set_error(ICS_ENOSUP, "fuse = 1 is only available with ICS_TV_SHIPPED");
  if (p->conv < ICS_CONV_AUTO || p->conv > ICS_CONV_FFT) return ics_set_error(ICS_EINVAL, "conv = %d is not an ICS_CONV_* value", p->conv);
  if (p->conv == ICS_CONV_FFT && (!(ics_conv_fft_supported(j->g.K) || (ics_conv_fft_blk_supported(j->g.K) && p->tv_mode == ICS_TV_SHIPPED)) || p->tv_mode == ICS_TV_MM_ACTIVE || p->fuse))
    return ics_set_error(ICS_ENOSUP, "ICS_CONV_FFT: the transform-tile pipeline is built for PSF sizes 3 ... 85 (the shipped loop and the PAM kinds: tv_mode 0, 2, 3; fuse 0) and, as tap blocks, 87 ... 255 (the shipped loop)");
  if (p->conv == ICS_CONV_FFT && !fft_mirror_fits(j->g))
    return ics_set_error(ICS_ENOSUP, "ICS_CONV_FFT: the channel-planar mirror of a %d x %d frame with a %d x %d PSF is %zu bytes, beyond the 2^31 - 1 the tile kernels address "
                "(ICS_CONV_AUTO runs such a frame on the matrix cores)", j->g.M, j->g.N, j->g.K, j->g.K, ics_planar_floats(j->g) * sizeof(float));
  if (p->conv == ICS_CONV_MATRIX && !j->bt_conv && !j->blk_conv) return ics_set_error(ICS_ENOSUP, "ICS_CONV_MATRIX: no matrix-core path for this PSF size");
  if (p->conv == ICS_CONV_MATRIX && !j->bt_conv && p->tv_mode != ICS_TV_SHIPPED)   // (the tap-block path has no TV epilogue; never run the fp32 kernels under an explicit MATRIX request)
    return ics_set_error(ICS_ENOSUP, "ICS_CONV_MATRIX with tv_mode %d: PSF sizes above 49 run on the matrix cores as tap blocks, which exist for the shipped loop only", p->tv_mode);
  if (p->conv == ICS_CONV_VECTOR && psf_blocks_only(j->g.K))
    return ics_set_error(ICS_ENOSUP, "ICS_CONV_VECTOR: PSF sizes above 127 only run as tap blocks on the matrix cores (ICS_CONV_AUTO / ICS_CONV_MATRIX)");
  if (p->fuse && j->g.K > 31) return ics_set_error(ICS_ENOSUP, "fuse = 1 is only built for PSF sizes <= 31");
  if (p->tv_mode != ICS_TV_SHIPPED && j->g.K > 63) return ics_set_error(ICS_ENOSUP, "tv_mode %d is only built for PSF sizes <= 63 (the shipped loop runs to 255)", p->tv_mode);
  if (p->blind && p->channels != 3) return ics_set_error(ICS_ENOSUP, "blind deconvolution requires C == 3 (pyx:557,570 leave gradk undefined otherwise)");
  return ICS_OK;
}

// The routing table (see "routing" above).  in_run: ics_rl_run / ics_rl_describe rather than a single stage.  tiles_allowed = false: the
// mirrors did not fit the device (ics_rl_run), or a stage that does not run on them (ics_rl_stage).
Route ics_host::resolve_route(const ics_rl* j, const ics_rl_params* p, bool in_run, bool tiles_allowed) {
  const IcsDebug& d = ics_debug();
  auto sw = [](const std::atomic<int>& v) { return v.load(std::memory_order_relaxed); };
  // ICS_CONV_PATH: what ICS_CONV_AUTO resolves to, 0 default, 1 vector, 2 matrix, 3 fft (where the tiles do not run -- single stages, tv_mode 1,
  // PSF sizes above 65 -- what AUTO would take)
  const int path = sw(d.conv_path), small_sw = sw(d.small_iter), conv2_sw = sw(d.fft_conv2), overlap_sw = sw(d.overlap);
  const bool fused_sw = sw(d.fused_gradk) != 0, fft_gradk_sw = sw(d.fft_gradk) != 0, fft_fused_sw = sw(d.fft_fused) != 0, planar_sw = sw(d.planar_image) != 0;
  const IcsGeom& g = j->g;
  const int K = g.K;
  const int cus = j->ctx ? j->ctx->cus : 256;   // (no HIP call on this path: ics_describe has no context and assumes an MI355X's 256 CUs)
  const long px = (long)g.uM * g.uN;
  const bool blind = p->blind != 0, fuse = p->fuse != 0, autoc = p->conv == ICS_CONV_AUTO, vector = p->conv == ICS_CONV_VECTOR, matrix_req = p->conv == ICS_CONV_MATRIX;
  const bool shipped = p->tv_mode == ICS_TV_SHIPPED, pam = p->tv_mode == ICS_TV_PAM_ISO || p->tv_mode == ICS_TV_PAM_COLLAB;
  Route r{};

  // The transform tiles: the shipped loop (87 ... 255: tap blocks on the tiles) and, inside ics_rl_run, the PAM kinds -- TV term, back-projection
  // epilogue and update on the mirrors too (single stages of the TV variants run on the HWC kernels).  Never fused, never beyond the mirrors' 2 GiB.
  const bool tiles_built = shipped ? ics_conv_fft_supported(K) || ics_conv_fft_blk_supported(K) : pam && in_run && ics_conv_fft_supported(K);
  if (tiles_allowed && tiles_built && !fuse && fft_mirror_fits(g)) {
    if (p->conv == ICS_CONV_FFT) r.tiles = true;
    // PAM kinds: bench.py --tv-mode 2, ICS_CONV_PATH=matrix -> fft (measured with the convolutions and the gradient on the tiles only), ms per inner iteration: 1448^2 / 31 blind 0.357 -> 0.297; 2048^2 / 21 blind 0.470 -> 0.396,
    // non-blind 0.271 -> 0.259; 4096^2 / 19 blind 1.563 -> 1.132; 1100^2 / 45 blind 0.432 -> 0.310
    // round 6: the shipped loop's thresholds -- the same kernels but for the epilogue's operands -- except below 6 Mpx at 15 x 15 and less, where the
    // TV term's own pass on the planes tips it back (bench.py --tv-mode 2, ms per inner iteration, matrix cores -> tiles: 4096^2 / 15 blind 0.873 -> 0.780,
    // tv_mode 3 0.869 -> 0.794; 2048^2 / 15 non-blind 0.176 -> 0.190, blind 0.261 -> 0.293)
    else if (autoc && in_run) r.tiles = path == 3 || (path == 0 && fft_preferred(g, blind) && (!pam || K >= 17 || px >= 6000000L));
  }
  r.conv2 = r.tiles && conv2_sw != 0 && !j->conv2_off && ics_conv2_fft_supported(g) && (conv2_sw == 2 || K <= ICS_CONV2_MAX_K);

  // Modes 0 / 1 on the HWC frames.  ICS_CONV_AUTO: the matrix-core kernels where they exist and win (ics_conv_mfma_preferred); PSF sizes 51 ... 127 as
  // tap blocks on them (do_conv_blocks; 129 ... 255: no other path, ICS_CONV_PATH does not apply), shipped loop.  The run-time-sized fp32 kernels
  // (ics_big.hip) are the only ones above 63, and under ICS_CONV_AUTO they take over from the packed-fp32 kernels compiled per size wherever the
  // matrix-core kernels are not built or not chosen (51 .. 63; 39 .. 49 with ICS_CONV_PATH=...): they beat them (shipped loop, 2048^2 non-blind,
  // ms per pass, compiled -> run-time-sized): synthesis 39: 0.626 -> 0.594, 45: 0.829 -> 0.756, 55: 1.238 -> 1.013, 63: 1.71 -> 1.27;
  // back-projection (incl. the separate maxima pass) 39: 0.975 -> 0.716, 45: 1.348 -> 0.915, 55: 2.109 -> 1.233, 63: 2.88 -> 1.52.
  // ICS_CONV_VECTOR keeps the compiled kernels (tests/test_gpu_stages.py drives them at every size).
  const bool matrix = j->bt_conv && !vector && (matrix_req || path == 2 || ((path == 0 || path == 3) && ics_conv_mfma_preferred(K)));
  if (j->blk_conv && shipped && !vector && (psf_blocks_only(K) || matrix_req || path != 1)) r.conv = CONV_BLOCKS;
  else if (matrix) r.conv = CONV_MATRIX;
  else if (ics_big_supported(K) || (autoc && shipped && K >= 39 && path != 1)) r.conv = CONV_SIZED;
  else r.conv = CONV_PACKED;

  // The PSF gradient has its own choice: the matrix-core kernel wins at every size it is built for (K <= 31; at K = 19, 21, where AUTO keeps the
  // packed-fp32 convolutions, 0.35 vs 0.97 ms at 4096^2), and the tile pipeline's gradient reads the mirrors: matrix-core kernel only.  Fused with
  // A11 where that exists (k_synth_gradk: matrix-core path, K <= 15; k_synth_gradk_fft: the tiles), from 33 on as 31 x 31 blocks (do_gradk_split).
  const bool matrix_gk = ics_gradk_mfma_supported(K) && !vector && (matrix_req || r.tiles || path != 1);
  const bool fusable = !fuse && !(p->flags & ICS_FLAG_NO_FUSED_GRADK), fft_gk = r.tiles && fft_gradk_sw;
  if (fusable && !r.tiles && ics_synth_gradk_supported(K) && fused_sw && matrix && matrix_gk) r.gradk = GK_FUSED_MATRIX;
  else if (fusable && fft_gk && ics_conv_fft_supported(K) && fft_fused_sw) r.gradk = GK_FUSED_TILES;
  else if (fft_gk) r.gradk = GK_TILES;
  else if (K >= 33 && !vector && (psf_blocks_only(K) || r.tiles || matrix_req || path != 1)) r.gradk = GK_SPLIT;
  else if (ics_big_supported(K)) r.gradk = GK_SIZED;
  else r.gradk = matrix_gk ? GK_MATRIX : GK_FP32;

  // The PSF step of a blind inner iteration on the tiles as ONE launch behind the fused A11 + A13 unit (k_psf_spectra, ics_conv_fft.hip): inside
  // ics_rl_run, shipped loop, PSF sizes the tiles take whole.  Tap blocks, the two-kernel gradient, the PAM kinds, single stages and every other
  // route keep k_psf + k_fft_spectrum; ICS_FFT_PSF1=0 restores that pair here too.
  r.psf1 = in_run && r.tiles && shipped && r.gradk == GK_FUSED_TILES && ics_conv_fft_supported(K) && sw(d.fft_psf1) != 0;

  // Mode 2 of the tiles without the epilogue's operand reads (ics_maxg_select.h): inside ics_rl_run, shipped loop -- the update pass in front of a
  // launch records max u and max |(u - ut)/2|, the launch is the operand-free instance k_conv_fft<3>, and k_maxg_select behind it takes max |g| on the
  // tiles that can hold it.  The PAM kinds, single stages and every other route keep k_conv_fft<2>; ICS_FFT_MAXG=0 restores it here too.
  // By default from 6 Mpx on, where the launch is short of bytes: bench.py, parent -> this route, ms per inner iteration, 4096^2 / 15 blind 0.643 -> 0.613,
  // non-blind 0.452 -> 0.425; at 2048^2 / 15 (--conv fft, blind) the launch is two and a half rounds of units and gains 1 us, the recording update pass
  // costs 3.5 us more than k_update_planar: 0.237 -> 0.239.  ICS_FFT_MAXG=2: wherever mode 2 runs (the tests' small frames).
  const int maxg_sw = sw(d.fft_maxg);
  r.maxg = in_run && r.conv2 && shipped && !fuse && (maxg_sw == 2 || (maxg_sw == 1 && px >= ICS_MAXG_MIN_PX));

  // Small frames (ics_small.hip): every (tile, channel) of the u-frame on a compute unit of its own, the operands of the five inner iterations
  // resident in LDS, ONE cooperative launch per outer iteration instead of 25 - 30.  What ICS_CONV_AUTO picks for the shipped loop when the
  // frame is small enough (3 x tiles of 32 or 64 <= compute units, operands <= 160 KB of LDS: up to ~290^2 at 31 x 31, ~570^2 at 15 x 15);
  // an explicit ICS_CONV_* request, ICS_CONV_PATH or the debug switch `small_iter` = 0 keep the multi-launch families.
  // Non-blind (two convolutions and two barriers per inner iteration): measured level with the multi-launch path at 255^2 for PSF sizes up to 15 (0.029 ms
  // either way), ahead of it from 17 x 17 (255^2 / 23: 0.057 -> 0.041) and on frames up to ~160^2 at every size (128^2 / 7: 0.022 -> 0.018).
  r.small = autoc && shipped && !fuse && !r.tiles && !j->small_off && path == 0 && small_sw != 0 && (blind || K >= 17 || px <= 26000L) &&
            ics_small_plan(g, cus, &r.plan, small_sw == 2);

  // tv_mode 1 rewrites the image in every inner iteration (pyx:547-549 live): a copy would have to be rebuilt each time
  r.image_acc = p->tv_mode != ICS_TV_MM_ACTIVE && planar_sw;
  r.acc_order = !r.small && r.image_acc && ((!r.tiles && r.conv == CONV_MATRIX && ics_conv_mfma_rs(K, g, cus) != 0) || (blind && r.gradk == GK_FUSED_MATRIX));

  // Statistics of outer iteration i overlapped with iteration i + 1 (ics_rl_run).  Not with the opt-in fused update + convolution (its
  // own u ping-pong), not with tv_mode 1 (the image is stepped too: nothing to fall back on), not with an empty window, not for a
  // single iteration.  Debug switch `overlap` = 0 restores the drain at every outer boundary.
  // Measured (MI355X, ms per inner iteration, drained -> overlapped): non-blind 512^2 / 9x9 0.044 -> 0.040 (0.060 -> 0.040 after a long run of
  // small launches, when the device has clocked down), non-blind 2048^2 / 15x15 0.160 -> 0.152; blind 4096^2 / 15x15 0.808 -> 0.804 without
  // and 0.810 -> 0.821 with event brackets in the timed region: on frames that fill the device the statistics' small kernels only compete
  // with the persistent workgroups of the convolutions.
  // Re-measured at the end of round 4 on two boxes, drained -> overlapped: non-blind 512^2 0.045 -> 0.040, 1024^2 0.080 -> 0.073, 1448^2 0.103 -> 0.096,
  // 2048^2 level, 2560^2 0.218 -> 0.223, 2900^2 0.270 -> 0.277, 3072^2 0.320 -> 0.333; blind 255^2 0.066 -> 0.066 ... 0.070 (the copies of the PSF
  // and the event bubble of an outer boundary weigh as much as the drain they replace), 512^2 0.073 -> 0.077, 1024^2 0.114 -> 0.111, 1536^2
  // level, 2048^2 0.227 -> 0.232, 2560^2 0.333 -> 0.341.  Hence by default (switch = 1): non-blind up to 4.5 Mpx, blind between 0.6 and 2.5 Mpx;
  // everywhere with switch = 2.  (Round 6: on the transform tiles -- one persistent 1024-thread workgroup per CU -- the statistics' small kernels
  // fit beside the iteration's at every size: 4096^2 / 15, drained -> second stream: blind 0.6713 -> 0.6591 ms, non-blind 0.4734 -> 0.4629; the
  // cooperative iteration kernel of small frames leaves room beside it as well: blind 255^2 / 15 0.060 -> 0.052 ms.)
  if (!fuse && p->tv_mode != ICS_TV_MM_ACTIVE && !j->win_empty && p->iterations >= 2)
    r.overlap = overlap_sw == 2 || (overlap_sw == 1 && (r.tiles || r.small || (blind ? px >= 600000L && px <= 2500000L : px <= 4500000L)));
  return r;
}

// ics_rl_describe / ics_describe: the route ics_rl_run resolves for these parameters
static int describe_impl(ics_rl* j, const ics_rl_params* p, ics_rl_route* r) {
  if (!r) return ics_set_error(ICS_EINVAL, "route is NULL");
  if (r->struct_size != sizeof(ics_rl_route)) return ics_set_error(ICS_EINVAL, "ics_rl_route.struct_size = %u, expected %zu", r->struct_size, sizeof(ics_rl_route));
  RC(check_params(j, p));
  const Route rt = resolve_route(j, p, true, true);
  memset(r, 0, sizeof *r);   // (graph: always 0)
  r->struct_size = sizeof(ics_rl_route);
  r->conv_family = rt.small ? CONV_SMALL : (rt.tiles ? CONV_TILES : rt.conv);
  r->conv_fp16_split = r->conv_family == CONV_MATRIX || r->conv_family == CONV_BLOCKS;
  if (p->blind) {
    r->gradk_family = rt.small ? GK_SMALL : rt.gradk;
    r->gradk_fp16_split = r->gradk_family <= GK_SPLIT;
  }
  r->image_in_accumulator_order = rt.acc_order;
  return ICS_OK;
}
extern "C" int ics_rl_describe(ics_rl* j, const ics_rl_params* p, ics_rl_route* r) { return describe_impl(j, p, r); }
// the same for a shape alone: no device, no job (the predicates read the geometry and which weight tables a job of this PSF size owns)
extern "C" unsigned long long ics_rl_frame_bytes(int M, int N, int MK) {
  if (M < 1 || N < 1 || MK < 3 || !(MK & 1) || !psf_supported(MK)) return 0ull;
  return (unsigned long long)ics_frame_floats(ics_make_geom(M, N, MK)) * 4ull;
}

// for the tests, beside ics_debug_set and like it outside the public header: the work units of mode 2 of the tiles (A1 + A3 in one unit per tile
// pair) on such a frame = the blocks of its image spectra; 0 where mode 2 is not built.  No device needed.
extern "C" int ics_debug_conv2_units(int M, int N, int MK) {
  if (M < 1 || N < 1 || MK < 3 || !(MK & 1) || !psf_supported(MK)) return 0;
  const IcsGeom g = ics_make_geom(M, N, MK);
  if (!ics_conv_fft_supported(MK) || !ics_conv2_fft_supported(g)) return 0;
  return (int)(ics_conv2_fft_fspec_floats(g) / ((size_t)8 * 1024 * 4));
}

extern "C" int ics_describe(int M, int N, int MK, const ics_rl_params* p, ics_rl_route* r) {
  if (M < 1 || N < 1 || MK < 3 || !(MK & 1)) return ics_set_error(ICS_EINVAL, "bad shape: M=%d N=%d MK=%d (MK odd >= 3)", M, N, MK);
  if (!psf_supported(MK)) return ics_set_error(ICS_ENOSUP, "PSF size %d not supported (odd sizes 3..%d)", MK, ICS_PSF_MAX);
  ics_rl shell{};
  shell.g = ics_make_geom(M, N, MK);
  float dummy = 0.f;                                               // non-NULL markers only: nothing is dereferenced
  if (ics_conv_mfma_supported(MK)) shell.bt_conv = shell.bt_corr = &dummy;
  if (MK >= 51) shell.blk_conv = shell.blk_corr = &dummy;
  return describe_impl(&shell, p, r);
}
