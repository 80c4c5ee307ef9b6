// ics_job.hip -- the device-resident Richardson-Lucy job (ics_host.h ics_rl) of the C ABI (include/ics_hip.h): creation and
// teardown, every host / device transfer, the rank exchange and all-reduce entries, and what a job allocates on first use (the stop
// test's window, planar mirrors, accumulator-order image, TV frame, small-frame scratch) with the weight packing and the conversions
// between the HWC frames and their mirrors.  Host side only.
#include "ics_host.h"

using namespace ics_host;

// one launch for the zero-fill of everything dalloc collected in `zl` (ics_host.h ZeroList)
static int flush_zero(ics_ctx* c, ZeroList& zl) {
  size_t i = 0;
  while (i < zl.items.size()) {
    IcsZeroArgs a{};
    unsigned long long run = 0;
    for (; a.count < ICS_ZERO_MAX && i < zl.items.size(); ++i) {
      a.p[a.count] = zl.items[i].first;
      run += (zl.items[i].second + 15) / 16;        // (pool blocks are multiples of 8 KiB: the rounding stays inside the block)
      a.end16[a.count++] = run;
    }
    HIPCHK(ics_launch_zero_many(a, c->stream));
  }
  zl.items.clear();
  return ICS_OK;
}

extern "C" void ics_rl_destroy(ics_rl* j) {
  if (!j) return;
  hipSetDevice(j->ctx->device);
  hipStreamSynchronize(j->ctx->stream);
  void* ptrs[] = {j->facc[0], j->facc[1], j->tvf, j->u, j->u2, j->ut, j->gr, j->f, j->e, j->psf, j->psf_next, j->gradk, j->wconv, j->wcorr, j->bt_conv, j->bt_corr, j->psf_caller, j->partial, j->psf_work, j->blk_conv, j->blk_corr, j->blk_scr, j->blk_negf, j->blk_red,
                  j->red, j->dofkeys, j->sched, j->scal, j->dacc, j->ukey, j->flags, j->z, j->tw, j->weights, j->gradk64, j->e2, j->psf_bak, j->small_part, j->small_bar, j->small_keys};
  if (j->ctx->stream2) hipStreamSynchronize(j->ctx->stream2);   // (the statistics' stream uses the job's buffers as well: drain it before they are recycled)
  for (void* p : ptrs) if (p) j->ctx->pool.release(p);   // (recycled by the context: ordered on its stream, no hipFree synchronisation)
  for (int i = 0; i < j->ntwins; ++i) if (j->twins[i].pl) j->ctx->pool.release(j->twins[i].pl);
  if (j->spec_conv) j->ctx->pool.release(j->spec_conv);
  if (j->spec_corr) j->ctx->pool.release(j->spec_corr);
  if (j->fspec) j->ctx->pool.release(j->fspec);
  if (j->mgs) j->ctx->pool.release(j->mgs);
  if (j->mgs_wave) j->ctx->pool.release(j->mgs_wave);
  if (j->ktrace) j->ctx->pool.release(j->ktrace);
  for (int i = 0; i < 2; ++i) { if (j->ev_body[i]) hipEventDestroy(j->ev_body[i]); if (j->ev_stats[i]) hipEventDestroy(j->ev_stats[i]); }
  if (j->h_scal) hipHostFree(j->h_scal);
  for (hipEvent_t e : j->ev) hipEventDestroy(e);
  if (j->ev_begin) hipEventDestroy(j->ev_begin);
  if (j->ev_end) hipEventDestroy(j->ev_end);
  delete j;
}

extern "C" int ics_rl_create(ics_ctx* c, int M, int N, int MK, ics_rl** out) {
  if (!c || !out) return ics_set_error(ICS_EINVAL, "NULL argument");
  *out = nullptr;
  if (M < 1 || N < 1) return ics_set_error(ICS_EINVAL, "image size %dx%d", M, N);
  if (MK < 3 || !(MK & 1)) return ics_set_error(ICS_EINVAL, "MK must be odd and >= 3 (got %d)", MK);
  if (!psf_supported(MK)) return ics_set_error(ICS_ENOSUP, "PSF size %d not supported (odd sizes 3..%d)", MK, ICS_PSF_MAX);
  HIPCHK(hipSetDevice(c->device));
  ics_rl* j = new ics_rl();  // value-initialised: every pointer/flag starts at 0
  j->ctx = c;
  j->g = ics_make_geom(M, N, MK);
  j->frame_floats = ics_frame_floats(j->g);
  j->origin = ics_origin_offset(j->g);
  // the matrix-core kernels address a frame through a raw buffer descriptor with 32-bit byte offsets
  if (j->frame_floats * 4 >= (size_t)ICS_FRAME_LIMIT_BYTES) {
    delete j;
    return ics_set_error(ICS_ENOSUP, "a %d x %d frame with a %d x %d PSF takes %.2f GB; frames are limited to 2 GiB (about 13000 x 13000 px)", M, N, MK, MK,
                (double)ics_frame_floats(ics_make_geom(M, N, MK)) * 4e-9);
  }
  const size_t n = (size_t)3 * MK * MK;
  const int nt = 16 * ((MK + 15) / 16);
  j->gradk_blocks = ics_gradk_blocks(j->g, c->cus);
  j->fused2_blocks = 3 * c->cus;
  if (const int mw = ics_debug().max_wgs.load(std::memory_order_relaxed); mw > 0 && j->fused2_blocks > mw) j->fused2_blocks = mw;
  int rc;
#define TRY(x) if ((rc = (x)) != ICS_OK) { ics_rl_destroy(j); return rc; }
  hipStream_t s = c->stream;
  ZeroList zl;
  TRY(dalloc(c, &j->u, j->frame_floats, &zl)); TRY(dalloc(c, &j->u2, j->frame_floats, &zl)); TRY(dalloc(c, &j->ut, j->frame_floats, &zl)); TRY(dalloc(c, &j->gr, j->frame_floats, &zl));
  TRY(dalloc(c, &j->f, j->frame_floats, &zl)); TRY(dalloc(c, &j->e, j->frame_floats, &zl));
  TRY(dalloc(c, &j->psf, n, &zl)); TRY(dalloc(c, &j->psf_next, n, &zl)); TRY(dalloc(c, &j->gradk, n, &zl)); TRY(dalloc(c, &j->psf_caller, n, &zl));
  if (MK > 63) TRY(dalloc(c, &j->psf_work, n, &zl));   // (k_psf<BIG>)
  if (MK >= 51) {   // tap blocks: the fewest blocks of a size the matrix-core convolution is built for (odd, <= 33)
    j->blk_n = (MK + 32) / 33;
    j->blk_kb = ((MK + j->blk_n - 1) / j->blk_n) | 1;
    const size_t tf = ics_conv_mfma_table_floats(j->blk_kb);
    TRY(dalloc(c, &j->blk_conv, tf * j->blk_n * j->blk_n, &zl)); TRY(dalloc(c, &j->blk_corr, tf * j->blk_n * j->blk_n, &zl));
    TRY(dalloc(c, &j->blk_scr, j->frame_floats, &zl));
    if (!(j->blk_n & 1)) TRY(dalloc(c, &j->blk_negf, j->frame_floats, &zl));
    TRY(dalloc(c, &j->blk_red, (size_t)ICS_RED_STRIDE, &zl));
  }
  TRY(dalloc(c, &j->wconv, (size_t)(MK + 1) * j->g.wrow, &zl)); TRY(dalloc(c, &j->wcorr, (size_t)(MK + 1) * j->g.wrow, &zl));
  if (ics_conv_mfma_supported(MK)) { TRY(dalloc(c, &j->bt_conv, ics_conv_mfma_table_floats(MK), &zl)); TRY(dalloc(c, &j->bt_corr, ics_conv_mfma_table_floats(MK), &zl)); }
  // (129 ...: the gradient only ever runs as 31 x 31 blocks -- 2 * CUs workgroups of 3 x 32 x 32 partial sums each, do_gradk_split)
  j->partial_floats = psf_blocks_only(MK) ? (size_t)2 * c->cus * 3 * 32 * 32
                                          : (size_t)(j->gradk_blocks > j->fused2_blocks ? j->gradk_blocks : j->fused2_blocks) * 3 * nt * nt;
  TRY(dalloc(c, &j->partial, j->partial_floats, &zl));
  TRY(dalloc(c, &j->red, (size_t)2 * 8 * ICS_RED_STRIDE, &zl)); TRY(dalloc(c, &j->dofkeys, (size_t)2 * 4, &zl)); TRY(dalloc(c, &j->sched, (size_t)16, &zl));   // (two sets: ics_rl::par)
  TRY(dalloc(c, &j->scal, (size_t)ICS_SC_COUNT, &zl)); TRY(dalloc(c, &j->dacc, (size_t)8, &zl)); TRY(dalloc(c, &j->ukey, (size_t)2, &zl)); TRY(dalloc(c, &j->flags, (size_t)4, &zl));
  TRY(flush_zero(c, zl));
#undef TRY
  hipError_t e = hipHostMalloc((void**)&j->h_scal, 2 * (ICS_SC_COUNT + 4) * sizeof(float), hipHostMallocDefault);   // (one mirror per set)
  if (e != hipSuccess) { ics_rl_destroy(j); return ics_set_error(ICS_ENOMEM, "hipHostMalloc: %s", hipGetErrorString(e)); }
  hipEventCreate(&j->ev_begin); hipEventCreate(&j->ev_end);
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) { ics_rl_destroy(j); return ics_set_error(ICS_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(e)); }
  *out = j;
  return ICS_OK;
}

static int copy_in(ics_rl* j, float* frame, const float* host, int rows, int cols_px, int oy, int ox) {
  float* dst = org(j, frame) + (ptrdiff_t)oy * j->g.pitch + 3 * ox;
  HIPCHK(hipMemcpy2DAsync(dst, (size_t)j->g.pitch * 4, host, (size_t)cols_px * 12, (size_t)cols_px * 12, rows,
                          hipMemcpyHostToDevice, j->ctx->stream));
  return ICS_OK;
}
static int copy_out(ics_rl* j, float* frame, float* host, int rows, int cols_px, int oy, int ox) {
  const float* src = org(j, frame) + (ptrdiff_t)oy * j->g.pitch + 3 * ox;
  HIPCHK(hipMemcpy2DAsync(host, (size_t)cols_px * 12, src, (size_t)j->g.pitch * 4, (size_t)cols_px * 12, rows,
                          hipMemcpyDeviceToHost, j->ctx->stream));
  return ICS_OK;
}

// (re)build the accumulator-order image for tile height 16 * RS if it is missing or stale; queued on the job's stream
int ics_host::ensure_image_acc(ics_rl* j, int RS) {
  const int k = RS == 2 ? 0 : 1;
  if (!j->facc[k]) {
    hipError_t e = j->ctx->pool.alloc((void**)&j->facc[k], ics_image_acc_floats(j->g, RS) * sizeof(float));
    if (e != hipSuccess) { (void)hipGetLastError(); j->facc[k] = nullptr; return ics_set_error(ICS_ENOMEM, "accumulator-order image: %s", hipGetErrorString(e)); }
    j->facc_valid[k] = false;
  }
  if (!j->facc_valid[k]) {
    hipError_t e = ics_launch_image_acc(j->f + j->origin, j->g, RS, j->facc[k], j->ctx->stream);
    if (e != hipSuccess) return ics_set_error(ICS_EHIP, "k_image_acc: %s", hipGetErrorString(e));
    j->facc_valid[k] = true;
  }
  return ICS_OK;
}

int ics_host::pack_weights(ics_rl* j, int do_step, float step, int correlation, hipStream_t s) {
  IcsPsfArgs a;
  a.psf = j->psf; a.gradk = j->gradk; a.wconv = j->wconv; a.wcorr = j->wcorr; a.bt_conv = j->bt_conv; a.bt_corr = j->bt_corr; a.psf_caller = j->psf_caller; a.work = j->psf_work;
  a.scal = j->scal; a.frozen = j->flags; a.step = step; a.K = j->g.K; a.wrow = j->g.wrow;
  a.correlation = correlation; a.do_step = do_step;
  HIPCHK(ics_launch_psf(a, s));
  if (j->blk_conv) HIPCHK(ics_launch_pack_blocks(j->psf, j->g.K, j->blk_kb, j->blk_n, j->blk_conv, j->blk_corr, ics_conv_mfma_table_floats(j->blk_kb), s));
  if (j->fft_on) {   // conj(DFT2(W)) / 128^2 of both orientations (PSF sizes above 85: of every tap block)
    int nb = 0, kb = 0;
    if (ics_conv_fft_blk_supported(j->g.K)) ics_conv_fft_blk_shape(j->g.K, &nb, &kb);
    HIPCHK(ics_launch_fft_spectrum(j->psf, j->g.K, j->spec_conv, j->spec_corr, s, nb, kb));
  }
  return ICS_OK;
}

// ---- FFT-tile pipeline: mirrors ---------------------------------------------------------------------------------------------------------
// every HWC frame buffer the pipeline touches gets a planar mirror (zero-filled: the aprons of a mirror are never written either)
int ics_host::ensure_planar(ics_rl* j) {
  float* want[] = {j->u, j->u2, j->ut, j->gr, j->f, j->e, j->e2, j->tvf};
  for (float* h : want) {
    if (!h || pl_of(j, h)) continue;
    if (j->ntwins >= 8) return ics_set_error(ICS_ESTATE, "planar mirror table full");
    float* pl = nullptr;
    RC(dalloc(j->ctx, &pl, ics_planar_floats(j->g)));
    j->twins[j->ntwins].hwc = h; j->twins[j->ntwins].pl = pl; ++j->ntwins;
    if (h == j->f) j->plf_valid = false;
  }
  int nb = 1, kb = 0;
  if (ics_conv_fft_blk_supported(j->g.K)) ics_conv_fft_blk_shape(j->g.K, &nb, &kb);      // (one spectrum per tap block and orientation)
  if (!j->spec_conv) RC(dalloc(j->ctx, &j->spec_conv, (size_t)nb * nb * ics_conv_fft_spectrum_floats()));
  if (!j->spec_corr) RC(dalloc(j->ctx, &j->spec_corr, (size_t)nb * nb * ics_conv_fft_spectrum_floats()));
  return ICS_OK;
}
// whole-buffer copies HWC -> mirror / mirror -> HWC (run and stage boundaries), and the stop-test window mirror -> HWC
int ics_host::to_planar(ics_rl* j, float* hwc, hipStream_t s) {
  HIPCHK(ics_launch_planar_convert(true, hwc, pl_of(j, hwc), j->g, true, 0, 0, 0, 0, s));
  return ICS_OK;
}
int ics_host::from_planar(ics_rl* j, float* hwc, hipStream_t s) {   // the u-frame only: the aprons of both stay zero
  HIPCHK(ics_launch_planar_convert(false, pl_of(j, hwc), hwc, j->g, false, 0, j->g.uM, 0, j->g.uN, s));
  return ICS_OK;
}

extern "C" int ics_rl_upload(ics_rl* j, const float* image, const float* u, const float* psf) {
  if (!j) return ics_set_error(ICS_EINVAL, "job is NULL");
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  const IcsGeom& g = j->g;
  int rc;
  if (image) image_changed(j);
  if (image && (rc = copy_in(j, j->f, image, g.M, g.N, g.pad, g.pad)) != ICS_OK) return rc;
  if (u && (rc = copy_in(j, j->u, u, g.uM, g.uN, 0, 0)) != ICS_OK) return rc;
  if (psf) {
    const size_t n = (size_t)3 * g.K * g.K * 4;
    HIPCHK(hipMemcpyAsync(j->psf, psf, n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(j->psf_caller, psf, n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(j->flags, 0, 4 * sizeof(int), s));
    if ((rc = pack_weights(j, 0, 0.f, 0, s)) != ICS_OK) return rc;
  }
  HIPCHK(hipStreamSynchronize(s));
  if (image && u && psf) j->uploaded = true;
  return ICS_OK;
}

extern "C" int ics_rl_download(ics_rl* j, float* u, float* psf_local, float* psf_caller) {
  if (!j) return ics_set_error(ICS_EINVAL, "job is NULL");
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  const IcsGeom& g = j->g;
  int rc;
  if (u && (rc = copy_out(j, j->u, u, g.uM, g.uN, 0, 0)) != ICS_OK) return rc;
  const size_t n = (size_t)3 * g.K * g.K * 4;
  if (psf_local) HIPCHK(hipMemcpyAsync(psf_local, j->psf, n, hipMemcpyDeviceToHost, s));
  if (psf_caller) HIPCHK(hipMemcpyAsync(psf_caller, j->psf_caller, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ICS_OK;
}

static int frame_of(ics_rl* j, int which, float** frame, int* rows, int* cols, int* oy, int* ox) {
  const IcsGeom& g = j->g;
  switch (which) {
    case ICS_BUF_U: *frame = j->u; break;
    case ICS_BUF_UT: *frame = j->ut; break;
    case ICS_BUF_GRADU: *frame = j->gr; break;
    case ICS_BUF_IMAGE: *frame = j->f; break;
    case ICS_BUF_ERROR: *frame = j->e; break;
    case ICS_BUF_TV: if (!j->tvf) return -1; *frame = j->tvf; break;
    default: return -1;
  }
  if (which == ICS_BUF_IMAGE || which == ICS_BUF_ERROR) { *rows = g.M; *cols = g.N; *oy = g.pad; *ox = g.pad; }
  else { *rows = g.uM; *cols = g.uN; *oy = 0; *ox = 0; }
  return 0;
}

extern "C" int ics_rl_read(ics_rl* j, int which, float* host, size_t count) {
  if (!j || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  const size_t n = (size_t)3 * j->g.K * j->g.K;
  float* frame; int rows, cols, oy, ox;
  if (frame_of(j, which, &frame, &rows, &cols, &oy, &ox) == 0) {
    if (count != (size_t)rows * cols * 3) return ics_set_error(ICS_EINVAL, "buffer %d holds %zu floats, got %zu", which, (size_t)rows * cols * 3, count);
    int rc = copy_out(j, frame, host, rows, cols, oy, ox);
    if (rc != ICS_OK) return rc;
  } else if (which == ICS_BUF_PSF || which == ICS_BUF_GRADK) {
    if (count != n) return ics_set_error(ICS_EINVAL, "buffer %d holds %zu floats, got %zu", which, n, count);
    HIPCHK(hipMemcpyAsync(host, which == ICS_BUF_PSF ? j->psf : j->gradk, n * 4, hipMemcpyDeviceToHost, s));
  } else if (which == ICS_BUF_SCALARS) {
    if (count != ICS_SC_COUNT) return ics_set_error(ICS_EINVAL, "scalars hold %d floats", ICS_SC_COUNT);
    HIPCHK(hipMemcpyAsync(host, j->scal, ICS_SC_COUNT * 4, hipMemcpyDeviceToHost, s));
  } else if (which == ICS_BUF_RED) {
    if (count != ICS_RED_STRIDE) return ics_set_error(ICS_EINVAL, "the reduction slot holds %d words", ICS_RED_STRIDE);
    HIPCHK(hipMemcpyAsync(host, j->red, 12 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(host + 12, j->dofkeys, 4 * 4, hipMemcpyDeviceToHost, s));   // [12] min key, [13] max key, [14] NaN flag of the DoF mask
  } else {
    return ics_set_error(ICS_EINVAL, "unknown buffer %d", which);
  }
  HIPCHK(hipStreamSynchronize(s));
  return ICS_OK;
}

// for the tests, beside ics_debug_set and like it outside the public header: the reduction keys (ICS_RED_STRIDE words per slot) the update
// passes of the last ics_rl_run read, inner iteration by inner iteration, while the debug switch key_trace was on.  Returns the number of
// slots written to `host` (at most `slots`), or a negative error code.
extern "C" int ics_debug_key_trace(ics_rl* j, uint32_t* host, int slots) {
  if (!j || !host || slots < 0) { (void)ics_set_error(ICS_EINVAL, "NULL argument"); return -1; }
  int n = j->ktrace_n < ICS_KEY_TRACE_SLOTS ? j->ktrace_n : ICS_KEY_TRACE_SLOTS;
  if (n > slots) n = slots;
  if (!j->ktrace || n == 0) return 0;
  if (hipSetDevice(j->ctx->device) != hipSuccess || hipStreamSynchronize(j->ctx->stream) != hipSuccess ||
      hipMemcpy(host, j->ktrace, (size_t)n * ICS_RED_STRIDE * 4, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); (void)ics_set_error(ICS_EHIP, "key trace: copy failed"); return -1; }
  return n;
}

extern "C" int ics_rl_write(ics_rl* j, int which, const float* host, size_t count) {
  if (!j || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  const size_t n = (size_t)3 * j->g.K * j->g.K;
  float* frame; int rows, cols, oy, ox;
  if (frame_of(j, which, &frame, &rows, &cols, &oy, &ox) == 0) {
    if (count != (size_t)rows * cols * 3) return ics_set_error(ICS_EINVAL, "buffer %d holds %zu floats, got %zu", which, (size_t)rows * cols * 3, count);
    if (which == ICS_BUF_IMAGE) image_changed(j);
    int rc = copy_in(j, frame, host, rows, cols, oy, ox);
    if (rc != ICS_OK) return rc;
  } else if (which == ICS_BUF_PSF || which == ICS_BUF_GRADK) {
    if (count != n) return ics_set_error(ICS_EINVAL, "buffer %d holds %zu floats, got %zu", which, n, count);
    HIPCHK(hipMemcpyAsync(which == ICS_BUF_PSF ? j->psf : j->gradk, host, n * 4, hipMemcpyHostToDevice, s));
    if (which == ICS_BUF_PSF) { int rc = pack_weights(j, 0, 0.f, 0, s); if (rc != ICS_OK) return rc; }
  } else if (which == ICS_BUF_RED) {
    if (count != ICS_RED_STRIDE) return ics_set_error(ICS_EINVAL, "the reduction slot holds %d words", ICS_RED_STRIDE);
    HIPCHK(hipMemcpyAsync(j->red, host, ICS_RED_STRIDE * 4, hipMemcpyHostToDevice, s));
  } else {
    return ics_set_error(ICS_EINVAL, "buffer %d is not writable", which);
  }
  HIPCHK(hipStreamSynchronize(s));
  return ICS_OK;
}

static int rows_io(ics_rl* j, int which, int row0, int nrows, float* host, bool to_host) {
  if (!j || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(j->ctx->device));
  float* frame; int rows, cols, oy, ox;
  if (frame_of(j, which, &frame, &rows, &cols, &oy, &ox) != 0) return ics_set_error(ICS_EINVAL, "buffer %d is not a frame", which);
  if (row0 < 0 || nrows < 1 || row0 + nrows > rows) return ics_set_error(ICS_EINVAL, "rows [%d, %d) outside the %d rows of buffer %d", row0, row0 + nrows, rows, which);
  float* dev = org(j, frame) + (ptrdiff_t)(oy + row0) * j->g.pitch + 3 * ox;
  if (!to_host && which == ICS_BUF_IMAGE) image_changed(j);
  if (to_host) HIPCHK(hipMemcpy2DAsync(host, (size_t)cols * 12, dev, (size_t)j->g.pitch * 4, (size_t)cols * 12, nrows, hipMemcpyDeviceToHost, j->ctx->stream));
  else HIPCHK(hipMemcpy2DAsync(dev, (size_t)j->g.pitch * 4, host, (size_t)cols * 12, (size_t)cols * 12, nrows, hipMemcpyHostToDevice, j->ctx->stream));
  HIPCHK(hipStreamSynchronize(j->ctx->stream));
  return ICS_OK;
}
extern "C" int ics_rl_read_rows(ics_rl* j, int which, int row0, int nrows, float* host) { return rows_io(j, which, row0, nrows, host, true); }
extern "C" int ics_rl_write_rows(ics_rl* j, int which, int row0, int nrows, const float* host) { return rows_io(j, which, row0, nrows, const_cast<float*>(host), false); }

// device-to-device rows between two jobs (lib/banded.py: halo exchange, stop-test gather).  Ordering: the source stream is
// drained, the copy runs on the destination stream and is waited for -- the band driver is host-synchronous per stage anyway.
extern "C" int ics_rl_copy_rows(ics_rl* dst, int dst_which, int dst_row0, ics_rl* src, int src_which, int src_row0, int nrows) {
  if (!dst || !src) return ics_set_error(ICS_EINVAL, "NULL argument");
  float *df, *sf; int drows, dcols, doy, dox, srows, scols, soy, sox;
  if (frame_of(dst, dst_which, &df, &drows, &dcols, &doy, &dox) != 0) return ics_set_error(ICS_EINVAL, "buffer %d is not a frame", dst_which);
  if (frame_of(src, src_which, &sf, &srows, &scols, &soy, &sox) != 0) return ics_set_error(ICS_EINVAL, "buffer %d is not a frame", src_which);
  if (dcols != scols) return ics_set_error(ICS_EINVAL, "row length %d (destination) != %d (source)", dcols, scols);
  if (nrows < 1 || dst_row0 < 0 || dst_row0 + nrows > drows || src_row0 < 0 || src_row0 + nrows > srows)
    return ics_set_error(ICS_EINVAL, "rows [%d, %d) of %d <- rows [%d, %d) of %d", dst_row0, dst_row0 + nrows, drows, src_row0, src_row0 + nrows, srows);
  if (dst_which == ICS_BUF_IMAGE) image_changed(dst);
  const int dd = dst->ctx->device, sd = src->ctx->device;
  if (dd != sd) {
    int can = 0;
    HIPCHK(hipDeviceCanAccessPeer(&can, dd, sd));
    if (!can) return ics_set_error(ICS_ENOSUP, "device %d cannot access device %d: no peer path", dd, sd);
    HIPCHK(hipSetDevice(dd));
    hipError_t pe = hipDeviceEnablePeerAccess(sd, 0);
    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) return ics_set_error(ICS_EHIP, "hipDeviceEnablePeerAccess(%d): %s", sd, hipGetErrorString(pe));
    (void)hipGetLastError();
  }
  HIPCHK(hipSetDevice(sd));
  HIPCHK(hipStreamSynchronize(src->ctx->stream));
  HIPCHK(hipSetDevice(dd));
  const float* sp = org(src, sf) + (ptrdiff_t)(soy + src_row0) * src->g.pitch + 3 * sox;
  float* dp = org(dst, df) + (ptrdiff_t)(doy + dst_row0) * dst->g.pitch + 3 * dox;
  HIPCHK(hipMemcpy2DAsync(dp, (size_t)dst->g.pitch * 4, sp, (size_t)src->g.pitch * 4, (size_t)dcols * 12, nrows,
                          dd == sd ? hipMemcpyDeviceToDevice : hipMemcpyDefault, dst->ctx->stream));
  HIPCHK(hipStreamSynchronize(dst->ctx->stream));
  return ICS_OK;
}

// Rows of a frame buffer to / from the same buffer of band jobs on OTHER RANKS (one process per GPU, RCCL point-to-point over xGMI):
// the halo exchange and the stop-test gather of lib/banded.py in rank mode.  Whole pitch rows travel (the apron columns are
// zero on both sides).  ics_group_sendrecv_device: ics_group.hip.
extern "C" int ics_rl_exchange_rows(ics_rl* j, ics_group* g, int which, int send_row0, int send_rows, int send_peer, int recv_row0, int recv_rows, int recv_peer) {
  if (!j || !g) return ics_set_error(ICS_EINVAL, "NULL argument");
  float* frame; int rows, cols, oy, ox;
  if (frame_of(j, which, &frame, &rows, &cols, &oy, &ox) != 0) return ics_set_error(ICS_EINVAL, "buffer %d is not a frame", which);
  if (send_peer >= 0 && (send_row0 < 0 || send_rows < 1 || send_row0 + send_rows > rows)) return ics_set_error(ICS_EINVAL, "send rows [%d, %d) of %d", send_row0, send_row0 + send_rows, rows);
  if (recv_peer >= 0 && (recv_row0 < 0 || recv_rows < 1 || recv_row0 + recv_rows > rows)) return ics_set_error(ICS_EINVAL, "receive rows [%d, %d) of %d", recv_row0, recv_row0 + recv_rows, rows);
  HIPCHK(hipSetDevice(j->ctx->device));
  HIPCHK(hipStreamSynchronize(j->ctx->stream));          // what is sent has been produced
  if (recv_peer >= 0 && which == ICS_BUF_IMAGE) image_changed(j);
  const size_t pitch = (size_t)j->g.pitch;
  // row r of the buffer = frame row oy + r; a pitch row starts ax pixels left of the frame origin
  float* base = frame;                                  // allocation start of the frame (origin = base + ay rows + ax pixels)
  const float* sp = base + (size_t)(j->g.ay + oy + (send_peer >= 0 ? send_row0 : 0)) * pitch;
  float* rp = base + (size_t)(j->g.ay + oy + (recv_peer >= 0 ? recv_row0 : 0)) * pitch;
  return ics_group_sendrecv_device(g, sp, send_peer >= 0 ? (size_t)send_rows * pitch : 0, send_peer, rp, recv_peer >= 0 ? (size_t)recv_rows * pitch : 0, recv_peer);
}

// -------------------------------------------------------------------------------------------------
// stop-test scratch: Gaussian window weights (pyx:393-404), twiddles, P x P x 3 complex buffer (2 x 3 x H x Px on the long-line path)
int ics_host::ensure_window(ics_rl* j, const ics_rl_params* p) {
  const int H = p->bottom - p->top, W = p->right - p->left;
  // an empty window: the reference slices error[top:bottom, left:right] into an empty array and every statistic is NaN
  // (numpy warns, pyx:600-601,627-638 do not raise); the stop test then never fires.  Decided BEFORE the cache check: jobs are
  // reused across calls (lib/deconvolution.py keeps them), and window W -> empty window -> W must not leave the flag set.
  j->win_empty = (H < 1 || W < 1);
  if (j->win_empty) return ICS_OK;
  if (j->z && j->wt == p->top && j->wb == p->bottom && j->wl == p->left && j->wr == p->right) return ICS_OK;
  if (p->top < 0 || p->left < 0 || p->bottom > j->g.M || p->right > j->g.N)
    return ics_set_error(ICS_EINVAL, "stats window [%d:%d, %d:%d] outside the %dx%d image", p->top, p->bottom, p->left, p->right, j->g.M, j->g.N);
  const int need = 2 * (H > W ? H : W) - 1;
  int P = 2, logP = 1;
  while (P < need) { P <<= 1; ++logP; }
  // a side above 4096 px: the long-line path of ics_stats.hip, transform sizes per axis (an 8300 x 200 window must not take 32768^2)
  const bool big = P > 8192;
  int Py = 0, Px = 0;
  if (big) {
    Py = 64; Px = 64;
    while (Py < 2 * H - 1) Py <<= 1;
    while (Px < 2 * W - 1) Px <<= 1;
    // a frame below 2 GiB has sides below 13 377 px: 2 * 13 376 - 1 < 32768, so no job gets here
    if (Py > 32768 || Px > 32768) return ics_set_error(ICS_ENOSUP, "stats window %dx%d needs a %dx%d-point FFT (max 32768 a side)", H, W, Py, Px);
  }
  // The cached key goes first: if an allocation below fails (z alone is 1.6 GB at P = 8192) the job must not keep the old key with
  // freed or half-built buffers -- jobs are reused (lib/deconvolution.py), and the next run with the previous window would pass the
  // cache check and launch the statistics kernels on them.
  auto drop = [&]() {
    j->wt = j->wb = j->wl = j->wr = -1; j->P = 0; j->logP = 0; j->Py = j->Px = 0;
    if (j->z) { j->ctx->pool.release(j->z); j->z = nullptr; }
    if (j->tw) { j->ctx->pool.release(j->tw); j->tw = nullptr; }
    if (j->weights) { j->ctx->pool.release(j->weights); j->weights = nullptr; }
  };
  drop();
  int rc;
  const int fail_at = ics_debug().fail_window_alloc.exchange(0, std::memory_order_relaxed);   // test hook: the fail_at-th allocation fails once
  // long-line path: z holds the H rows that carry data, [3][H][Px], and their transpose (ics_stats.hip); tw = the full tables of both
  // axes, [Py] then [Px]
  const size_t nz = big ? (size_t)6 * H * Px : (size_t)3 * P * P, ntw = big ? (size_t)Py + Px : (size_t)P / 2 + 1;
  if ((rc = fail_at == 1 ? ics_set_error(ICS_ENOMEM, "stats window: allocation of %zu bytes failed (test hook)", nz * sizeof(float2)) : dalloc(j->ctx, &j->z, nz, false)) != ICS_OK) { drop(); return rc; }
  if ((rc = fail_at == 2 ? ics_set_error(ICS_ENOMEM, "stats window: allocation of %zu bytes failed (test hook)", ntw * sizeof(float2)) : dalloc(j->ctx, &j->tw, ntw, false)) != ICS_OK) { drop(); return rc; }
  if ((rc = fail_at == 3 ? ics_set_error(ICS_ENOMEM, "stats window: allocation of %zu bytes failed (test hook)", (size_t)H * W * sizeof(float)) : dalloc(j->ctx, &j->weights, (size_t)H * W, false)) != ICS_OK) { drop(); return rc; }
  std::vector<float2> tw(ntw);
  if (big) {   // each entry from its own angle in double, stored as float (no recurrence)
    for (int k = 0; k < Py; ++k) { const double ang = -2.0 * M_PI * (double)k / (double)Py; tw[k] = make_float2((float)cos(ang), (float)sin(ang)); }
    for (int k = 0; k < Px; ++k) { const double ang = -2.0 * M_PI * (double)k / (double)Px; tw[Py + k] = make_float2((float)cos(ang), (float)sin(ang)); }
  } else {
    for (int k = 0; k < P / 2; ++k) {
      const double ang = -2.0 * M_PI * (double)k / (double)P;
      tw[k] = make_float2((float)cos(ang), (float)sin(ang));
    }
    tw[P / 2] = make_float2(0.f, 0.f);
  }
  // np.linspace(-1., 1., num, dtype=float32) then gaussian_weight(x, 0, 1) in float (pyx:35-36,397-401)
  auto serie = [](int num, std::vector<float>& out) {
    out.resize(num);
    const double step = num > 1 ? 2.0 / (double)(num - 1) : 0.0;
    const float PI = 3.141592653589793f;
    for (int i = 0; i < num; ++i) {
      double y = (double)i * step + (-1.0);
      if (num > 1 && i == num - 1) y = 1.0;
      const float x = (float)y;
      out[i] = expf(-powf(x - 0.f, 2.f) / (2 * powf(1.f, 2.f))) / (1.f * powf(2 * PI, 0.5f));
    }
  };
  std::vector<float> wi, he, w((size_t)H * W);
  serie(H, wi); serie(W, he);
  double sum = 0.0;
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) { w[(size_t)r * W + c] = sqrtf(wi[r] * he[c]); sum += w[(size_t)r * W + c]; }
  const float fs = (float)sum;
  for (auto& v : w) v = v / fs;
  HIPCHK(hipMemcpyAsync(j->tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, j->ctx->stream));
  HIPCHK(hipMemcpyAsync(j->weights, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, j->ctx->stream));
  HIPCHK(hipStreamSynchronize(j->ctx->stream));  // tw / w are stack-owned host vectors
  j->P = P; j->logP = logP; j->Py = Py; j->Px = Px; j->wt = p->top; j->wb = p->bottom; j->wl = p->left; j->wr = p->right;
  return ICS_OK;
}

// ---- row bands over several ranks: the two per-iteration reductions, in place on the device (lib/banded.py rank mode) -----------
extern "C" int ics_rl_allreduce_keys(ics_rl* j, ics_group* g) {
  if (!j || !g) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (!ics_group_info_local(g) && ics_group_device(g) != j->ctx->device)   // (the collective runs on the job's stream with the group's communicator)
    return ics_set_error(ICS_EINVAL, "the job lives on device %d, the group's communicator on device %d", j->ctx->device, ics_group_device(g));
  if (j->par != 0) return ics_set_error(ICS_ESTATE, "ics_rl_allreduce_keys acts on reduction set 0 (stage API); the job is inside an overlapped run");
  HIPCHK(hipSetDevice(j->ctx->device));
  return ics_group_allreduce_device(g, j->red, 6, 0, j->ctx->stream);      // slot 0: [0..2] max|g_k|, [3..5] max u_k
}
extern "C" int ics_rl_allreduce_gradk(ics_rl* j, ics_group* g) {
  if (!j || !g) return ics_set_error(ICS_EINVAL, "NULL argument");
  int rank = 0, world = 1;
  RC(ics_group_info(g, &rank, &world));
  if (world == 1 && ics_group_info_local(g)) return ICS_OK;
  if (!ics_group_info_local(g) && ics_group_device(g) != j->ctx->device)
    return ics_set_error(ICS_EINVAL, "the job lives on device %d, the group's communicator on device %d", j->ctx->device, ics_group_device(g));
  HIPCHK(hipSetDevice(j->ctx->device));
  const size_t n = (size_t)3 * j->g.K * j->g.K;
  if (!j->gradk64) RC(dalloc(j->ctx, &j->gradk64, n, false));
  HIPCHK(ics_launch_f32_to_f64(j->gradk, j->gradk64, (long)n, j->ctx->stream));
  RC(ics_group_allreduce_device(g, j->gradk64, n, 1, j->ctx->stream));
  HIPCHK(ics_launch_f64_to_f32(j->gradk64, j->gradk, (long)n, j->ctx->stream));
  return ICS_OK;
}

// ---- allocated by the first run or stage that needs them: the TV term's frame, the small-frame iteration's scratch ----------------
int ics_host::ensure_tv(ics_rl* j) {
  if (j->tvf) return ICS_OK;
  int rc = dalloc(j->ctx, &j->tvf, j->frame_floats);
  return rc;
}

int ics_host::ensure_small(ics_rl* j, const IcsSmallPlan& pl) {
  if (!j->small_part) RC(dalloc(j->ctx, &j->small_part, (size_t)pl.nwg * j->g.K * j->g.K));
  if (!j->small_bar) RC(dalloc(j->ctx, &j->small_bar, (size_t)ICS_SMALL_BAR_WORDS));
  if (!j->small_keys) RC(dalloc(j->ctx, &j->small_keys, (size_t)8 * pl.nwg));
  return ICS_OK;
}

// richardson_lucy_MM(image[iy:iy+M, ix:ix+N], u[uy:uy+uM, ux:ux+uN], psf, ...) with both arrays on the device
// (deconvolve.py:277-313 passes such window views)
extern "C" int ics_rl_upload_img(ics_rl* j, const ics_img* image, int iy, int ix, const ics_img* u, int uy, int ux, const float* psf) {
  if (!j || !image || !u || !psf) return ics_set_error(ICS_EINVAL, "NULL argument");
  const IcsGeom& g = j->g;
  if (image->ctx != j->ctx || u->ctx != j->ctx) return ics_set_error(ICS_EINVAL, "images of another context");
  if (!rect_ok(image, iy, ix, g.M, g.N)) return ics_set_error(ICS_EINVAL, "image window [%d:%d, %d:%d] outside a %d x %d image", iy, iy + g.M, ix, ix + g.N, image->H, image->W);
  if (!rect_ok(u, uy, ux, g.uM, g.uN)) return ics_set_error(ICS_EINVAL, "u window [%d:%d, %d:%d] outside a %d x %d image", uy, uy + g.uM, ux, ux + g.uN, u->H, u->W);
  HIPCHK(hipSetDevice(j->ctx->device));
  hipStream_t s = j->ctx->stream;
  image_changed(j);
  float* df = org(j, j->f) + (ptrdiff_t)g.pad * g.pitch + 3 * g.pad;
  HIPCHK(hipMemcpy2DAsync(df, (size_t)g.pitch * 4, image->d + ((size_t)iy * image->W + ix) * 3, (size_t)image->W * 12, (size_t)g.N * 12, g.M, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpy2DAsync(org(j, j->u), (size_t)g.pitch * 4, u->d + ((size_t)uy * u->W + ux) * 3, (size_t)u->W * 12, (size_t)g.uN * 12, g.uM, hipMemcpyDeviceToDevice, s));
  const size_t n = (size_t)3 * g.K * g.K * 4;
  HIPCHK(hipMemcpyAsync(j->psf, psf, n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(j->psf_caller, psf, n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(j->flags, 0, 4 * sizeof(int), s));
  RC(pack_weights(j, 0, 0.f, 0, s));
  HIPCHK(hipStreamSynchronize(s));   // psf is a host buffer
  j->uploaded = true;
  return ICS_OK;
}
// the whole u frame (the reference updates the caller's `u` view in place, border ring included) -> dst[y:y+uM, x:x+uN]
extern "C" int ics_rl_download_img(ics_rl* j, ics_img* dst, int y, int x) {
  if (!j || !dst) return ics_set_error(ICS_EINVAL, "NULL argument");
  const IcsGeom& g = j->g;
  if (dst->ctx != j->ctx) return ics_set_error(ICS_EINVAL, "image of another context");
  if (!rect_ok(dst, y, x, g.uM, g.uN)) return ics_set_error(ICS_EINVAL, "u window [%d:%d, %d:%d] outside a %d x %d image", y, y + g.uM, x, x + g.uN, dst->H, dst->W);
  HIPCHK(hipSetDevice(j->ctx->device));
  HIPCHK(hipMemcpy2DAsync(dst->d + ((size_t)y * dst->W + x) * 3, (size_t)dst->W * 12, org(j, j->u), (size_t)g.pitch * 4, (size_t)g.uN * 12, g.uM,
                          hipMemcpyDeviceToDevice, j->ctx->stream));
  return ICS_OK;
}
