// ics_images.hip -- the ics_img_* entries of the C ABI (include/ics_hip.h).  Host side only; kernels live in ics_img.hip / ics_img_filters.hip /
// ics_img_tvdenoise.hip / ics_img_wavelet.hip / ics_img_noise.hip / ics_img_despeckle.hip / ics_img_blurwidth.hip / ics_img_blurmap.hip / ics_img_mask.hip / ics_img_guided.hip / ics_img_llf.hip (what these ten share: ics_img_px.h) / ics_img_wiener.hip / ics_img_tvdeconv.hip / ics_img_tvmdeconv.hip / ics_img_psfest.hip / ics_img_edges.hip / ics_img_align.hip / ics_resize.hip.
#include "ics_host.h"

using namespace ics_host;

// ================================================================================================
// Device-resident images (ics_host.h ics_img): the frames deconvolve.py keeps between two richardson_lucy_MM calls (pyramid levels, blind ->
// non-blind phase) stay in HBM; every operation is queued on the context's stream, only ics_img_download synchronises.
// ================================================================================================
static int img_new(ics_ctx* c, int H, int W, ics_img** out) {
  if (!c || !out) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (H < 1 || W < 1) return ics_set_error(ICS_EINVAL, "bad image size %d x %d", H, W);
  HIPCHK(hipSetDevice(c->device));
  ics_img* m = new (std::nothrow) ics_img{c, H, W, nullptr};
  if (!m) return ics_set_error(ICS_ENOMEM, "host allocation failed");
  hipError_t e = c->pool.alloc((void**)&m->d, (size_t)H * W * 3 * 4);
  if (e != hipSuccess) { delete m; return ics_set_error(ICS_ENOMEM, "device allocation of a %d x %d image: %s", H, W, hipGetErrorString(e)); }
  *out = m;
  return ICS_OK;
}

extern "C" int ics_img_create(ics_ctx* c, int H, int W, ics_img** out) { return img_new(c, H, W, out); }
extern "C" void ics_img_destroy(ics_img* m) {
  if (!m) return;
  m->ctx->pool.release(m->d);   // (operations on the image are queued on the context's stream; so is whatever reuses the block)
  delete m;
}

namespace {
// An entry that makes a new image: *out, up to four pool temporaries and the ev0 / ev1 bracket around its kernels.  *out is NULL from
// the start and stays NULL unless finish() returns ICS_OK; whatever is still held when the scope ends, on any return, goes back to
// the pool (queued work of a context runs on its one stream: so does whatever reuses the blocks).  out == nullptr: an entry that
// makes no image (ics_img_noise_estimate).
struct ImgOp {
  ics_ctx* c; ics_img** out; const char* name;
  void* tmp[4] = {nullptr, nullptr, nullptr, nullptr};
  int ntmp = 0;
  bool bracket = false, ok = false;
  ImgOp(ics_ctx* ctx, ics_img** o, const char* entry) : c(ctx), out(o), name(entry) {}   // (*out: cleared by check_new)
  ImgOp(const ImgOp&) = delete;
  ~ImgOp() { release(); if (!ok && out) { ics_img_destroy(*out); *out = nullptr; } }
  void release() { for (int i = 0; i < ntmp; ++i) c->pool.release(tmp[i]); ntmp = 0; }
  hipError_t alloc(void** p, size_t bytes) {
    if (ntmp == 4) return hipErrorInvalidValue;
    hipError_t e = c->pool.alloc(p, bytes);
    if (e == hipSuccess) tmp[ntmp++] = *p;
    return e;
  }
  hipError_t begin() { bracket = true; return hipEventRecord(c->ev0, c->stream); }
  hipError_t end() {   // closes the bracket before finish(): for an entry that queues something behind its kernels
    const hipError_t e = hipEventRecord(c->ev1, c->stream);
    if (e == hipSuccess) c->ev_pending = true;
    bracket = false;
    return e;
  }
  int finish(hipError_t e) {
    if (bracket && e == hipSuccess) e = end();
    release();
    ok = e == hipSuccess;   // (otherwise the destructor destroys *out)
    return ok ? ICS_OK : ics_set_error(e == hipErrorOutOfMemory ? ICS_ENOMEM : ICS_EHIP, "%s: %s", name, hipGetErrorString(e));
  }
};
int check_new(const void* src, ics_img** out) {   // the arguments every such entry has; *out is NULL from here on unless the entry succeeds
  if (out) *out = nullptr;
  return src && out ? ICS_OK : ics_set_error(ICS_EINVAL, "NULL argument");
}
int check_coupling(int coupling) {
  return coupling == 0 || coupling == 1 ? ICS_OK : ics_set_error(ICS_EINVAL, "coupling %d (0 = channel, 1 = vector)", coupling);
}
int check_route(int route, const char* one, const char* two) {
  return route >= 0 && route <= 2 ? ICS_OK : ics_set_error(ICS_EINVAL, "route %d (0 = auto, 1 = %s, 2 = %s)", route, one, two);
}
}  // namespace

extern "C" int ics_img_shape(const ics_img* m, int* H, int* W) {
  if (!m) return ics_set_error(ICS_EINVAL, "image is NULL");
  if (H) *H = m->H;
  if (W) *W = m->W;
  return ICS_OK;
}
extern "C" int ics_img_upload(ics_img* m, const float* host) {
  if (!m || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  HIPCHK(hipMemcpyAsync(m->d, host, (size_t)m->H * m->W * 12, hipMemcpyHostToDevice, m->ctx->stream));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));   // the host buffer may be released by the caller
  return ICS_OK;
}
extern "C" int ics_img_upload_int(ics_img* m, const void* host, int bytes_per_value) {
  if (!m || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (bytes_per_value != 1 && bytes_per_value != 2) return ics_set_error(ICS_EINVAL, "bytes_per_value = %d (1: uint8, 2: uint16)", bytes_per_value);
  ics_ctx* c = m->ctx;
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)m->H * m->W * 3;
  void* raw = nullptr;
  if (hipError_t e = c->pool.alloc(&raw, n * bytes_per_value); e != hipSuccess) return ics_set_error(ICS_ENOMEM, "img_upload_int: %s", hipGetErrorString(e));
  hipError_t e = hipMemcpyAsync(raw, host, n * bytes_per_value, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = ics_launch_int_to_f32(raw, bytes_per_value, m->d, (long)n, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the host buffer may be released by the caller
  c->pool.release(raw);                                       // (everything of a context runs on its one stream: a recycled block needs no more)
  if (e != hipSuccess) return ics_set_error(ICS_EHIP, "img_upload_int: %s", hipGetErrorString(e));
  return ICS_OK;
}
extern "C" int ics_img_download(const ics_img* m, float* host) {
  if (!m || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  HIPCHK(hipMemcpyAsync(host, m->d, (size_t)m->H * m->W * 12, hipMemcpyDeviceToHost, m->ctx->stream));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  return ICS_OK;
}
extern "C" int ics_img_pad_edge(const ics_img* src, int top, int bottom, int left, int right, ics_img** out) {
  RC(check_new(src, out));
  if (top < 0 || bottom < 0 || left < 0 || right < 0) return ics_set_error(ICS_EINVAL, "negative padding");
  ImgOp op(src->ctx, out, "img_pad_edge");
  RC(img_new(src->ctx, src->H + top + bottom, src->W + left + right, out));
  return op.finish(ics_launch_img_pad_edge(src->d, src->H, src->W, (*out)->d, top, bottom, left, right, src->ctx->stream));
}

extern "C" int ics_img_crop(const ics_img* src, int y0, int x0, int H, int W, ics_img** out) {
  RC(check_new(src, out));
  if (!rect_ok(src, y0, x0, H, W)) return ics_set_error(ICS_EINVAL, "crop [%d:%d, %d:%d] outside a %d x %d image", y0, y0 + H, x0, x0 + W, src->H, src->W);
  ImgOp op(src->ctx, out, "img_crop");
  RC(img_new(src->ctx, H, W, out));
  return op.finish(hipMemcpy2DAsync((*out)->d, (size_t)W * 12, src->d + ((size_t)y0 * src->W + x0) * 3, (size_t)src->W * 12, (size_t)W * 12, H,
                                    hipMemcpyDeviceToDevice, src->ctx->stream));
}
extern "C" int ics_img_paste(ics_img* dst, int y0, int x0, const ics_img* src) {
  if (!src || !dst) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (src->ctx != dst->ctx) return ics_set_error(ICS_EINVAL, "images of different contexts");
  if (!rect_ok(dst, y0, x0, src->H, src->W)) return ics_set_error(ICS_EINVAL, "paste of %d x %d at (%d, %d) outside a %d x %d image", src->H, src->W, y0, x0, dst->H, dst->W);
  HIPCHK(hipSetDevice(dst->ctx->device));
  HIPCHK(hipMemcpy2DAsync(dst->d + ((size_t)y0 * dst->W + x0) * 3, (size_t)dst->W * 12, src->d, (size_t)src->W * 12, (size_t)src->W * 12, src->H,
                          hipMemcpyDeviceToDevice, dst->ctx->stream));
  return ICS_OK;
}
extern "C" int ics_img_gamma(ics_img* m, float div, float exponent, float mul, int clip01) {
  if (!m) return ics_set_error(ICS_EINVAL, "image is NULL");
  HIPCHK(hipSetDevice(m->ctx->device));
  HIPCHK(ics_launch_img_gamma(m->d, (long)m->H * m->W * 3, div, exponent, mul, clip01, m->ctx->stream));
  return ICS_OK;
}
// deconvolve.py:245-249 on a device image: float64 inside (as skimage / scipy compute), rounded to float32 like the
// reference's `.astype(np.float32)`
extern "C" int ics_img_resize(const ics_img* src, int OH, int OW, ics_img** out) {
  RC(check_new(src, out));
  if (OH < 1 || OW < 1 || src->H < 2 || src->W < 2) return ics_set_error(ICS_EINVAL, "bad sizes");
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int H = src->H, W = src->W;
  if (H == OH && W == OW) return ics_img_crop(src, 0, 0, H, W, out);
  ImgOp op(c, out, "img_resize");
  RC(img_new(c, OH, OW, out));
  auto weights = [](double sigma, std::vector<double>& w) {
    const int r = (int)(4.0 * sigma + 0.5);
    w.resize(2 * r + 1);
    double sum = 0.0;
    for (int k = -r; k <= r; ++k) { w[k + r] = exp(-0.5 / (sigma * sigma) * (double)k * (double)k); sum += w[k + r]; }
    for (double& v : w) v /= sum;
    return r;
  };
  const double sy = fmax(0.0, ((double)H / OH - 1.0) / 2.0), sx = fmax(0.0, ((double)W / OW - 1.0) / 2.0);
  std::vector<double> hwy, hwx;
  int ry = 0, rx = 0;
  if (sy > 1e-15) ry = weights(sy, hwy);
  if (sx > 1e-15) rx = weights(sx, hwx);
  double *scr = nullptr, *dw = nullptr;          // (the float32 frames are read and written by the float64 pipeline's first and last pass)
  hipError_t e = op.alloc((void**)&scr, ics_resize_scratch_doubles(H, W, 3) * 8);
  if (e == hipSuccess) e = op.alloc((void**)&dw, (hwy.size() + hwx.size() + 1) * 8);
  const size_t nw = hwy.size() + hwx.size();
  bool staged = false;
  if (e == hipSuccess && nw) {
    if (nw <= ics_ctx::PIN_DOUBLES) {          // through the context's pinned staging area: nothing to wait for afterwards
      if (!c->pin) { e = hipHostMalloc((void**)&c->pin, ics_ctx::PIN_DOUBLES * 8, hipHostMallocDefault); if (e == hipSuccess) e = hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming); }
      if (e == hipSuccess && c->pin_used) e = hipEventSynchronize(c->pin_ev);
      if (e == hipSuccess) {
        memcpy(c->pin, hwy.data(), hwy.size() * 8);
        memcpy(c->pin + hwy.size(), hwx.data(), hwx.size() * 8);
        e = hipMemcpyAsync(dw, c->pin, nw * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(c->pin_ev, s);
        c->pin_used = true; staged = true;
      }
    } else {
      if (!hwy.empty()) e = hipMemcpyAsync(dw, hwy.data(), hwy.size() * 8, hipMemcpyHostToDevice, s);
      if (e == hipSuccess && !hwx.empty()) e = hipMemcpyAsync(dw + hwy.size(), hwx.data(), hwx.size() * 8, hipMemcpyHostToDevice, s);
    }
  }
  if (e == hipSuccess) e = ics_launch_resize_f32(src->d, H, W, 3, hwy.empty() ? nullptr : dw, ry, hwx.empty() ? nullptr : dw + hwy.size(), rx, scr, (*out)->d, OH, OW, s);
  if (e == hipSuccess && nw && !staged) e = hipStreamSynchronize(s);   // pageable host vectors are released below
  return op.finish(e);
}

// ---- lib/utils.py filters on device images (csrc/ics_img_filters.hip) ----------------------------------------------------------
// convolve2d(mode="same", boundary="symm") per channel [+ USM epilogue]; the kernels take the taps reversed (ics_img_filters.hip)
static int img_conv_common(const ics_img* src, const float* kern, int KH, int KW, int usm, float amount, ics_img** out) {
  RC(check_new(src, out));
  if (!kern) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (KH < 1 || KW < 1) return ics_set_error(ICS_EINVAL, "bad kernel size %d x %d", KH, KW);
  ics_ctx* c = src->ctx;
  const int H = src->H, W = src->W;
  // rank-1 test on the float32 taps: an outer product rounded to float32 entry by entry is one to 4 x 2^-24 of its largest product
  std::vector<double> kd(kern, kern + (size_t)KH * KW), col, row;
  const bool sep = rank1_factors(kd.data(), KH, KW, col, row, 0x1p-21);
  const bool cols_only = !sep && KW == 1 && KH > 1;
  if (sep ? (ics_img_conv_rows_lds(1, KW) > 160 * 1024 || ics_img_conv_cols_lds(KH) > 160 * 1024)
          : (cols_only ? ics_img_conv_cols_lds(KH) > 160 * 1024 : ics_img_conv_rows_lds(KH, KW) > 160 * 1024))
    return ics_set_error(ICS_ENOSUP, "kernel %d x %d (%s) too large for the LDS tile (rank 1: up to 129 x 764; otherwise (15 + KH) * (260 + 12 * ceil(KW / 4)) floats within 160 KB)",
                KH, KW, sep ? "rank 1" : "not rank 1");
  std::vector<float> t;
  if (sep) {   // [KW row taps][KH column taps], both reversed
    for (int u = 0; u < KW; ++u) t.push_back((float)row[KW - 1 - u]);
    for (int v = 0; v < KH; ++v) t.push_back((float)col[KH - 1 - v]);
  } else {
    for (int v = 0; v < KH; ++v) for (int u = 0; u < KW; ++u) t.push_back(kern[(size_t)(KH - 1 - v) * KW + (KW - 1 - u)]);
  }
  ImgOp op(c, out, "img_convolve");
  RC(img_new(c, H, W, out));
  hipStream_t s = c->stream;
  float *dk = nullptr, *tmp = nullptr;
  hipError_t e = op.alloc((void**)&dk, t.size() * 4);
  if (e == hipSuccess && sep) e = op.alloc((void**)&tmp, (size_t)H * W * 12);
  if (e == hipSuccess) e = put_table(c, dk, t);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) {
    if (sep) {   // rows (1 x KW), then columns (KH x 1) with the USM epilogue against the original frame
      e = ics_launch_img_conv_rows(src->d, H, W, dk, 1, KW, tmp, src->d, 0, 0.f, s);
      if (e == hipSuccess) e = ics_launch_img_conv_cols(tmp, H, W, dk + KW, KH, (*out)->d, src->d, usm, amount, s);
    } else if (cols_only) {
      e = ics_launch_img_conv_cols(src->d, H, W, dk, KH, (*out)->d, src->d, usm, amount, s);
    } else {
      e = ics_launch_img_conv_rows(src->d, H, W, dk, KH, KW, (*out)->d, src->d, usm, amount, s);
    }
  }
  return op.finish(e);
}
extern "C" int ics_img_convolve(const ics_img* src, const float* kern, int KH, int KW, ics_img** out) {
  return img_conv_common(src, kern, KH, KW, 0, 0.f, out);
}
extern "C" int ics_img_usm(const ics_img* src, const float* kern, int KH, int KW, float amount, ics_img** out) {
  return img_conv_common(src, kern, KH, KW, 1, amount, out);
}

extern "C" int ics_img_bilateral(const ics_img* src, int radius, float std_i, float std_s, ics_img** out) {
  RC(check_new(src, out));
  if (radius < 0) return ics_set_error(ICS_EINVAL, "radius %d", radius);
  if (!(std_i > 0.f) || !(std_s > 0.f)) return ics_set_error(ICS_EINVAL, "std_i = %g, std_s = %g (both must be positive)", (double)std_i, (double)std_s);
  if (radius > 4096 || ics_img_bilateral_lds(radius) > 160 * 1024) return ics_set_error(ICS_ENOSUP, "radius %d too large for the LDS tile (up to 34)", radius);
  ics_ctx* c = src->ctx;
  const int H = src->H, W = src->W, D = 2 * radius + 1;
  std::vector<float> ws((size_t)D * D);   // x offset j slow, y offset i fast: the reference's offset order
  for (int j = -radius; j <= radius; ++j)
    for (int i = -radius; i <= radius; ++i) ws[(size_t)(j + radius) * D + (i + radius)] = (float)exp((double)(i * i + j * j) * (-1.0 / (2.0 * (double)std_s * (double)std_s)));
  ImgOp op(c, out, "img_bilateral");
  RC(img_new(c, H, W, out));
  float* dws = nullptr;
  hipError_t e = op.alloc((void**)&dws, ws.size() * 4);
  if (e == hipSuccess) e = put_table(c, dws, ws);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_bilateral(src->d, H, W, radius, (float)(-1.0 / (2.0 * (double)std_i * (double)std_i)), dws, (*out)->d, c->stream);
  return op.finish(e);
}

// ---- TV denoising of a device image (csrc/ics_img_tvdenoise.hip) ---------------------------------------------------------------
// route 0: the blocked route from 512^2 pixels on.  Measured ("TV denoise"; 50 iterations, channel / vector): at 512^2 it
// takes 0.205 / 0.192 ms against 0.232 / 0.231 and its lead grows with the frame; at 256^2 it is 0.186 / 0.171 against 0.157 - 0.19:
// one 32 x 32 tile per workgroup leaves three quarters of the compute units idle there.
static const long TV_BLOCK_MIN_PIXELS = 512L * 512L;
extern "C" int ics_img_tv_denoise(const ics_img* src, float weight, int iterations, int coupling, int route, ics_img** out) {
  RC(check_new(src, out));
  if (!(weight > 0.f) || !std::isfinite(weight)) return ics_set_error(ICS_EINVAL, "weight = %g (must be positive and finite)", (double)weight);
  if (iterations < 0) return ics_set_error(ICS_EINVAL, "iterations = %d", iterations);
  RC(check_coupling(coupling));
  RC(check_route(route, "per iteration", "blocked"));
  ics_ctx* c = src->ctx;
  const int H = src->H, W = src->W;
  if (route == 0) route = (long)H * W >= TV_BLOCK_MIN_PIXELS ? 2 : 1;
  ImgOp op(c, out, "img_tv_denoise");
  RC(img_new(c, H, W, out));
  hipStream_t s = c->stream;
  float* q[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  const int frames = iterations ? 2 * ics_img_tv_pairs(iterations, route) : 0;
  for (int i = 0; i < frames && e == hipSuccess; ++i) e = op.alloc((void**)&q[i], (size_t)H * W * 12);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) {
    if (iterations == 0) e = hipMemcpyAsync((*out)->d, src->d, (size_t)H * W * 12, hipMemcpyDeviceToDevice, s);
    else e = ics_launch_img_tv_denoise(src->d, H, W, weight, iterations, coupling, route, q, (*out)->d, s);
  }
  return op.finish(e);
}

// ---- wavelet equaliser of a device image (csrc/ics_img_wavelet.hip) -------------------------------------------------------------
// route 0: the per-scale route at every size.  The fused route moves 10 frame transits instead of 18 at J = 5 ("Wavelet
// equaliser"), but no kernel times of the two routes exist yet, and a crossover is not to be guessed: scripts/filters_timing.py prints
// the table (routes alternating) from which a size rule is to be set here.  Both routes are callable through `route`.
extern "C" int ics_img_wavelet_equalize(const ics_img* src, int scales, const float* gains, const float* thresholds, float residual, int coupling,
                                        int route, ics_img** out) {
  RC(check_new(src, out));
  if (scales < 1 || scales > ICS_IMG_WAVELET_MAX_SCALES) return ics_set_error(ICS_EINVAL, "scales = %d (1 .. %d)", scales, ICS_IMG_WAVELET_MAX_SCALES);
  if (!gains) return ics_set_error(ICS_EINVAL, "gains is NULL");
  for (int j = 0; j < scales; ++j) {
    if (!std::isfinite(gains[j])) return ics_set_error(ICS_EINVAL, "gains[%d] = %g (must be finite)", j, (double)gains[j]);
    if (thresholds && (!std::isfinite(thresholds[j]) || thresholds[j] < 0.f))
      return ics_set_error(ICS_EINVAL, "thresholds[%d] = %g (must be finite and >= 0)", j, (double)thresholds[j]);
  }
  if (!std::isfinite(residual)) return ics_set_error(ICS_EINVAL, "residual = %g (must be finite)", (double)residual);
  RC(check_coupling(coupling));
  RC(check_route(route, "per scale", "first scales fused"));
  ics_ctx* c = src->ctx;
  const int H = src->H, W = src->W;
  if (route == 0) route = 1;
  ImgOp op(c, out, "img_wavelet_equalize");
  RC(img_new(c, H, W, out));
  float* tmp[2] = {nullptr, nullptr};
  hipError_t e = hipSuccess;
  const int frames = ics_img_wavelet_frames(scales, route);
  for (int i = 0; i < frames && e == hipSuccess; ++i) e = op.alloc((void**)&tmp[i], (size_t)H * W * 12);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_wavelet(src->d, H, W, scales, gains, thresholds, residual, coupling, route, tmp, (*out)->d, c->stream);
  return op.finish(e);
}

// ---- noise estimate of a device image (csrc/ics_img_noise.hip) -------------------------------------------------------------------
// route 0: the keys route at every size.  Measured ("Noise estimate on a resident frame"; channel / vector): at 4096^2 it
// takes 0.34 / 0.17 ms against 0.64 / 0.62, at 1024^2 0.073 / 0.055 against 0.103 / 0.078, and at 128^2, where the seven launches
// are all there is, 0.046 / 0.031 against 0.045 / 0.031: no crossover.  It borrows 12 / 4 bytes per pixel from the pool; route 1 needs
// nothing but the 24 KB block and stays callable.
extern "C" int ics_img_noise_estimate(const ics_img* src, int coupling, int route, float median[3], float level[3], float sigma[3]) {
  if (!src) return ics_set_error(ICS_EINVAL, "src is NULL");
  if (!median) return ics_set_error(ICS_EINVAL, "median is NULL");
  if (!level) return ics_set_error(ICS_EINVAL, "level is NULL");
  if (!sigma) return ics_set_error(ICS_EINVAL, "sigma is NULL");
  RC(check_coupling(coupling));
  RC(check_route(route, "recompute", "keys"));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int H = src->H, W = src->W;
  if (route == 0) route = 2;
  ImgOp op(c, nullptr, "img_noise_estimate");
  unsigned *blk = nullptr, *keys = nullptr, bits[3] = {0u, 0u, 0u};
  hipError_t e = op.alloc((void**)&blk, ics_img_noise_block_words() * sizeof(unsigned));
  if (const size_t words = ics_img_noise_key_words(H, W, coupling, route); e == hipSuccess && words) e = op.alloc((void**)&keys, words * sizeof(unsigned));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_noise(src->d, H, W, coupling, route, c->cus, blk, keys, c->stream);
  if (e == hipSuccess) e = op.end();
  if (e == hipSuccess) e = hipMemcpyAsync(bits, blk + ics_img_noise_result_word(), sizeof(bits), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  RC(op.finish(e));
  static const double E[] = ICS_IMG_NOISE_E;
  const double kappa = coupling ? 1.5381722544550522 / sqrt(3.0) : 0.6744897501960817, per_channel = coupling ? sqrt(3.0) * E[0] : E[0];
  for (int i = 0; i < 3; ++i) {
    float m;
    memcpy(&m, &bits[coupling ? 0 : i], sizeof(m));
    const double lv = (double)m / kappa;
    median[i] = m; level[i] = (float)lv; sigma[i] = (float)(lv / per_channel);
  }
  return ICS_OK;
}

// ---- despeckle of a device image (csrc/ics_img_despeckle.hip) ----------------------------------------------------------------------
// route 0: the tile route at every radius and size ("Despeckle on a resident frame": the timing table and the rule).
extern "C" int ics_img_despeckle(const ics_img* src, int radius, const float threshold[3], int coupling, int route, ics_img** out, unsigned replaced[3]) {
  RC(check_new(src, out));
  if (!threshold) return ics_set_error(ICS_EINVAL, "threshold is NULL");
  if (radius < 1 || radius > ICS_IMG_DESPECKLE_MAX_RADIUS) return ics_set_error(ICS_EINVAL, "radius = %d (1 .. %d)", radius, ICS_IMG_DESPECKLE_MAX_RADIUS);
  RC(check_coupling(coupling));
  for (int i = 0; i < (coupling ? 1 : 3); ++i)
    if (!std::isfinite(threshold[i]) || !(threshold[i] >= 0.f))
      return ics_set_error(ICS_EINVAL, "threshold[%d] = %g (must be finite and >= 0)", i, (double)threshold[i]);
  RC(check_route(route, "windows from the frame", "tiles in LDS"));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int H = src->H, W = src->W;
  if (route == 0) route = 2;
  ImgOp op(c, out, "img_despeckle");
  RC(img_new(c, H, W, out));
  const float t[3] = {threshold[0], coupling ? threshold[0] : threshold[1], coupling ? threshold[0] : threshold[2]};
  unsigned *cnt = nullptr, got[3] = {0u, 0u, 0u};
  hipError_t e = op.alloc((void**)&cnt, sizeof(got));
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof(got), c->stream);     // (before the bracket: last_kernel_ms is the kernel alone)
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_despeckle(src->d, H, W, radius, t, coupling, route, (*out)->d, cnt, c->stream);
  if (e == hipSuccess && replaced) {                 // the counters and nothing else: the frame stays where it is
    e = op.end();
    if (e == hipSuccess) e = hipMemcpyAsync(got, cnt, sizeof(got), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  RC(op.finish(e));
  if (replaced) { replaced[0] = got[0]; replaced[1] = coupling ? 0u : got[1]; replaced[2] = coupling ? 0u : got[2]; }
  return ICS_OK;
}

// ---- edge prediction on a device image (csrc/ics_img_edges.hip) ------------------------------------------------------------------------
// route 0 of the shock filter: the blocked route from 511^2 pixels on.  Measured ("Edge prediction"; 4 steps, vector / channel):
// at 255^2 a launch per step takes 0.018 / 0.019 ms against 0.024 / 0.035 (64 tiles leave three quarters of the compute units idle), at
// 511^2 the blocked route 0.025 / 0.038 against 0.034 / 0.037, at 1023^2 0.062 / 0.095 against 0.097 / 0.104, at 4096^2 0.78 / 1.31
// against 1.38 / 1.53.  The threshold is the smallest size at which the blocked route was measured ahead or level.
static const long SHOCK_BLOCK_MIN_PIXELS = 511L * 511L;
extern "C" int ics_img_shock(const ics_img* src, int iterations, float dt, float flat, int coupling, int route, ics_img** out) {
  RC(check_new(src, out));
  if (iterations < 0) return ics_set_error(ICS_EINVAL, "iterations = %d", iterations);
  if (!std::isfinite(dt)) return ics_set_error(ICS_EINVAL, "dt = %g (must be finite)", (double)dt);
  if (!(flat > 0.f) || !std::isfinite(flat)) return ics_set_error(ICS_EINVAL, "flat = %g (must be positive and finite)", (double)flat);
  const float inv_flat = (float)(1.0 / (double)flat);
  if (!std::isfinite(inv_flat)) return ics_set_error(ICS_EINVAL, "flat = %g (1 / flat is not finite)", (double)flat);
  RC(check_coupling(coupling));
  RC(check_route(route, "per step", "blocked"));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int H = src->H, W = src->W;
  if (route == 0) route = (long)H * W >= SHOCK_BLOCK_MIN_PIXELS ? 2 : 1;
  ImgOp op(c, out, "img_shock");
  RC(img_new(c, H, W, out));
  float* tmp[2] = {nullptr, nullptr};
  hipError_t e = hipSuccess;
  const int frames = ics_img_shock_frames(iterations, route);
  for (int i = 0; i < frames && e == hipSuccess; ++i) e = op.alloc((void**)&tmp[i], (size_t)H * W * 12);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) {
    if (iterations == 0) e = hipMemcpyAsync((*out)->d, src->d, (size_t)H * W * 12, hipMemcpyDeviceToDevice, c->stream);
    else e = ics_launch_img_shock(src->d, H, W, iterations, dt, inv_flat, coupling, route, tmp, (*out)->d, c->stream);
  }
  return op.finish(e);
}

// ---- byte masks of a device image's size (ics_mask): what ics_img_edge_mask makes and ics_img_psf_estimate_masked reads
extern "C" void ics_mask_destroy(ics_mask* m) {
  if (!m) return;
  m->ctx->pool.release(m->d);
  delete m;
}
extern "C" int ics_mask_create(ics_ctx* c, int H, int W, int planes, const unsigned char* host, ics_mask** out) {
  if (out) *out = nullptr;
  if (!c || !host || !out) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (H < 1 || W < 1 || (planes != 1 && planes != 3)) return ics_set_error(ICS_EINVAL, "bad mask size %d x %d x %d (planes: 1 or 3)", planes, H, W);
  HIPCHK(hipSetDevice(c->device));
  ics_mask* m = new (std::nothrow) ics_mask{c, H, W, planes, nullptr};
  if (!m) return ics_set_error(ICS_ENOMEM, "host allocation failed");
  hipError_t e = c->pool.alloc((void**)&m->d, (size_t)planes * H * W);
  if (e != hipSuccess) { delete m; return ics_set_error(ICS_ENOMEM, "device allocation of a %d x %d mask: %s", H, W, hipGetErrorString(e)); }
  e = hipMemcpyAsync(m->d, host, (size_t)planes * H * W, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the host buffer may be released by the caller
  if (e != hipSuccess) { ics_mask_destroy(m); return ics_set_error(ICS_EHIP, "mask_create: %s", hipGetErrorString(e)); }
  *out = m;
  return ICS_OK;
}
extern "C" int ics_mask_shape(const ics_mask* m, int* H, int* W, int* planes) {
  if (!m) return ics_set_error(ICS_EINVAL, "mask is NULL");
  if (H) *H = m->H;
  if (W) *W = m->W;
  if (planes) *planes = m->planes;
  return ICS_OK;
}
extern "C" int ics_mask_download(const ics_mask* m, unsigned char* host) {
  if (!m || !host) return ics_set_error(ICS_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  HIPCHK(hipMemcpyAsync(host, m->d, (size_t)m->planes * m->H * m->W, hipMemcpyDeviceToHost, m->ctx->stream));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  return ICS_OK;
}
// route 0 of the mask: the keys route at every size.  Measured (vector / channel): 0.26 / 1.05 ms against 0.36 / 1.33 at 4096^2, 0.165 /
// 0.425 against 0.172 / 0.438 at 1023^2, 0.067 / 0.149 against 0.066 / 0.147 at 255^2, where the eight launches are all there is: no
// crossover worth a rule.  It borrows 4 bytes per pixel and plane from the pool; route 1 needs only the 98 KB block and stays callable.
extern "C" int ics_img_edge_mask(const ics_img* src, unsigned per_sector, int coupling, int route, ics_mask** out, float threshold[3], unsigned kept[3]) {
  if (out) *out = nullptr;
  if (!src || !out || !threshold || !kept) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (per_sector < 1) return ics_set_error(ICS_EINVAL, "per_sector = %u (at least 1)", per_sector);
  RC(check_coupling(coupling));
  RC(check_route(route, "recompute", "keys"));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int H = src->H, W = src->W, planes = coupling ? 1 : 3;
  if (route == 0) route = 2;
  ics_mask* m = new (std::nothrow) ics_mask{c, H, W, planes, nullptr};
  if (!m) return ics_set_error(ICS_ENOMEM, "host allocation failed");
  if (hipError_t e = c->pool.alloc((void**)&m->d, (size_t)planes * H * W); e != hipSuccess) {
    delete m;
    return ics_set_error(ICS_ENOMEM, "device allocation of a %d x %d mask: %s", H, W, hipGetErrorString(e));
  }
  ImgOp op(c, nullptr, "img_edge_mask");
  unsigned *blk = nullptr, *keys = nullptr, res[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  hipError_t e = op.alloc((void**)&blk, ics_img_edge_block_words() * sizeof(unsigned));
  if (const size_t words = ics_img_edge_key_words(H, W, coupling, route); e == hipSuccess && words) e = op.alloc((void**)&keys, words * sizeof(unsigned));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_edge_mask(src->d, H, W, per_sector, coupling, route, c->cus, blk, keys, m->d, c->stream);
  if (e == hipSuccess) e = op.end();
  if (e == hipSuccess) e = hipMemcpyAsync(res, blk + ics_img_edge_result_word(), sizeof(res), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (const int rc = op.finish(e); rc != ICS_OK) { ics_mask_destroy(m); return rc; }
  // (a plane without a pixel of g > 0 has nothing to select: its threshold comes back as the NaN 0xFFFFFFFF, its mask empty, its count 0)
  for (int i = 0; i < 3; ++i) {
    memcpy(&threshold[i], &res[coupling ? 0 : i], sizeof(float));
    kept[i] = res[3 + (coupling ? 0 : i)];
  }
  *out = m;
  return ICS_OK;
}

// ---- blur profile of a device image (csrc/ics_img_blurwidth.hip) --------------------------------------------------------------------
// One route (a second summation order would buy nothing).  The rule that turns the profiles into a width is twenty lines on
// 2 (max_lag + 1) numbers and lives on the host (lib/_native.py blur_extent).
extern "C" int ics_img_blur_profile(const ics_img* src, int y0, int y1, int x0, int x1, int max_lag, double* ax, double* ay, long long* nx, long long* ny) {
  if (!src) return ics_set_error(ICS_EINVAL, "src is NULL");
  if (!ax || !ay || !nx || !ny) return ics_set_error(ICS_EINVAL, "an output (ax, ay, nx, ny) is NULL");
  const int H = src->H, W = src->W;
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1)
    return ics_set_error(ICS_EINVAL, "window [%d, %d) x [%d, %d) (not empty, inside the %d x %d frame)", y0, y1, x0, x1, H, W);
  if (max_lag < 0 || max_lag > ICS_IMG_BLURWIDTH_MAX_LAG) return ics_set_error(ICS_EINVAL, "max_lag = %d (0 .. %d)", max_lag, ICS_IMG_BLURWIDTH_MAX_LAG);
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int hw = y1 - y0, ww = x1 - x0, n = max_lag + 1;
  ImgOp op(c, nullptr, "img_blur_profile");
  float* partial = nullptr;
  double *result = nullptr, got[2 * (ICS_IMG_BLURWIDTH_MAX_LAG + 1)];
  hipError_t e = op.alloc((void**)&partial, ics_img_blurwidth_partial_floats(hw, ww, max_lag) * sizeof(float));
  if (e == hipSuccess) e = op.alloc((void**)&result, 2 * n * sizeof(double));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_blurwidth(src->d, H, W, y0, y1, x0, x1, max_lag, c->cus, partial, result, c->stream);
  if (e == hipSuccess) e = op.end();
  if (e == hipSuccess) e = hipMemcpyAsync(got, result, 2 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  RC(op.finish(e));
  for (int l = 0; l < n; ++l) {
    ax[l] = got[l]; ay[l] = got[n + l];
    nx[l] = ww - 1 - l > 0 ? (long long)hw * (ww - 1 - l) : 0;
    ny[l] = hw - 1 - l > 0 ? (long long)ww * (hw - 1 - l) : 0;
  }
  return ICS_OK;
}

// ---- window scores of a device image (csrc/ics_img_mask.hip) ----------------------------------------------------------------------
// One route.  The cells and the candidate table stay on the device; the five result numbers, and the score map where asked for, come back.
extern "C" int ics_img_window_scores(const ics_img* src, int y0, int y1, int x0, int x1, int size, float clip, int* box_y, int* box_x, double* score, double* trace,
                                     long long* clipped, double* map, int map_rows, int map_cols) {
  if (!src) return ics_set_error(ICS_EINVAL, "src is NULL");
  if (!box_y || !box_x || !score || !trace || !clipped) return ics_set_error(ICS_EINVAL, "an output (box_y, box_x, score, trace, clipped) is NULL");
  const int H = src->H, W = src->W;
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1)
    return ics_set_error(ICS_EINVAL, "region [%d, %d) x [%d, %d) (not empty, inside the %d x %d frame)", y0, y1, x0, x1, H, W);
  if (size < ICS_IMG_MASK_CELL) return ics_set_error(ICS_EINVAL, "size = %d (at least %d)", size, ICS_IMG_MASK_CELL);
  const int hr = y1 - y0, wr = x1 - x0;
  if (hr < size || wr < size) return ics_set_error(ICS_EINVAL, "region of %d x %d pixels, smaller than the box (size = %d)", hr, wr, size);
  if (!(clip > 0.f)) return ics_set_error(ICS_EINVAL, "clip = %g (above 0; inf keeps every finite pixel)", (double)clip);
  const int nci = ics_img_mask_candidates(hr, size), ncj = ics_img_mask_candidates(wr, size);
  if (map && (map_rows != nci || map_cols != ncj)) return ics_set_error(ICS_EINVAL, "map of %d x %d scores (the candidate grid is %d x %d)", map_rows, map_cols, nci, ncj);
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const size_t cand = (size_t)nci * ncj;
  ImgOp op(c, nullptr, "img_window_scores");
  float* cells = nullptr;
  double *table = nullptr, *result = nullptr, got[5];
  hipError_t e = op.alloc((void**)&cells, (size_t)ics_img_mask_cells(hr, size) * ics_img_mask_cells(wr, size) * 4 * sizeof(float));
  if (e == hipSuccess) e = op.alloc((void**)&table, 3 * cand * sizeof(double));
  if (e == hipSuccess) e = op.alloc((void**)&result, sizeof got);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_mask(src->d, H, W, y0, y1, x0, x1, size, clip, c->cus, cells, table, result, c->stream);
  if (e == hipSuccess) e = op.end();
  if (e == hipSuccess) e = hipMemcpyAsync(got, result, sizeof got, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && map) e = hipMemcpyAsync(map, table, cand * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  RC(op.finish(e));
  *box_y = y0 + ICS_IMG_MASK_CELL * (int)got[0]; *box_x = x0 + ICS_IMG_MASK_CELL * (int)got[1];
  *score = got[2]; *trace = got[3]; *clipped = (long long)got[4];
  return ICS_OK;
}

// ---- blur map of a device image (csrc/ics_img_blurmap.hip) -----------------------------------------------------------------------
// One route, one launch.  The taps go up through put_table; the cell grid and the workgroups' counts of non-finite pixels come back in
// one copy, the sparse plane (where asked for) in a second.
extern "C" int ics_img_blur_map(const ics_img* src, int y0, int y1, int x0, int x1, float sigma_a, float sigma_b, float edge, float max_sigma, float* weight,
                                float* moment, int* count, long long* bad, float* sparse, int rows, int cols) {
  if (!src) return ics_set_error(ICS_EINVAL, "src is NULL");
  if (!weight || !moment || !count || !bad) return ics_set_error(ICS_EINVAL, "an output (weight, moment, count, bad) is NULL");
  const int H = src->H, W = src->W;
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1)
    return ics_set_error(ICS_EINVAL, "window [%d, %d) x [%d, %d) (not empty, inside the %d x %d frame)", y0, y1, x0, x1, H, W);
  if (!(sigma_a >= 0.5f) || !(sigma_a < sigma_b) || !std::isfinite(sigma_b) || ics_img_blurmap_radius(sigma_b) > ICS_IMG_BLURMAP_MAX_RADIUS)
    return ics_set_error(ICS_EINVAL, "sigmas = (%g, %g) (0.5 <= sigma_a < sigma_b, ceil(3 sigma_b) <= %d)", (double)sigma_a, (double)sigma_b, ICS_IMG_BLURMAP_MAX_RADIUS);
  if (!(edge > 0.f)) return ics_set_error(ICS_EINVAL, "edge = %g (above 0)", (double)edge);
  if (!(max_sigma > 0.f)) return ics_set_error(ICS_EINVAL, "max_sigma = %g (above 0)", (double)max_sigma);
  const int hw = y1 - y0, ww = x1 - x0, cell = ICS_IMG_BLURMAP_CELL, nr = (hw + cell - 1) / cell, nc = (ww + cell - 1) / cell;
  if (rows != nr || cols != nc) return ics_set_error(ICS_EINVAL, "grid of %d x %d cells (the window has %d x %d)", rows, cols, nr, nc);
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  const size_t cells = (size_t)nr * nc;
  const int grid = ics_img_blurmap_grid(hw, ww, c->cus);
  std::vector<float> taps(2 * (2 * ICS_IMG_BLURMAP_MAX_RADIUS + 1), 0.f);
  ics_img_blurmap_taps(sigma_a, taps.data());
  ics_img_blurmap_taps(sigma_b, taps.data() + 2 * ICS_IMG_BLURMAP_MAX_RADIUS + 1);
  std::vector<float> got(3 * cells + grid);
  ImgOp op(c, nullptr, "img_blur_map");
  float *dtaps = nullptr, *block = nullptr, *plane = nullptr;
  hipError_t e = op.alloc((void**)&dtaps, taps.size() * sizeof(float));
  if (e == hipSuccess) e = op.alloc((void**)&block, got.size() * sizeof(float));
  if (e == hipSuccess && sparse) e = op.alloc((void**)&plane, (size_t)hw * ww * sizeof(float));
  if (e == hipSuccess) e = put_table(c, dtaps, taps);
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess)
    e = ics_launch_img_blurmap(src->d, H, W, y0, y1, x0, x1, sigma_a, sigma_b, edge, max_sigma, grid, dtaps, block, block + cells, reinterpret_cast<int*>(block + 2 * cells),
                               reinterpret_cast<int*>(block + 3 * cells), plane, c->stream);
  if (e == hipSuccess) e = op.end();
  if (e == hipSuccess) e = hipMemcpyAsync(got.data(), block, got.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && sparse) e = hipMemcpyAsync(sparse, plane, (size_t)hw * ww * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  RC(op.finish(e));
  memcpy(weight, got.data(), cells * sizeof(float));
  memcpy(moment, got.data() + cells, cells * sizeof(float));
  memcpy(count, got.data() + 2 * cells, cells * sizeof(int));
  long long n = 0;
  for (int i = 0; i < grid; ++i) { int v; memcpy(&v, got.data() + 3 * cells + i, sizeof v); n += v; }
  *bad = n;
  return ICS_OK;
}

// ---- Wiener deconvolution of a device image (csrc/ics_img_wiener.hip) -------------------------------------------------------------
// One route.  Two spectrum frames and a block of tables from the pool; the PSF goes up planar through put_table.
static int wiener_shape(int H, int W, int K, int* Py, int* Px) {
  if (H < 1 || W < 1) return ics_set_error(ICS_EINVAL, "bad image size %d x %d", H, W);
  if (K < 3 || K > ICS_PSF_MAX || !(K & 1)) return ics_set_error(ICS_EINVAL, "K = %d (odd, 3 .. %d)", K, ICS_PSF_MAX);
  if (K > H || K > W) return ics_set_error(ICS_EINVAL, "K = %d above the smaller side of the %d x %d frame", K, H, W);
  if (!ics_img_wiener_sizes(H, W, K, Py, Px))
    return ics_set_error(ICS_ENOSUP, "a %d x %d frame with a %d x %d PSF needs a transform of %d x %d points (H + K - 1, W + K - 1); the limit is %d a side",
                         H, W, K, K, H + K - 1, W + K - 1, ICS_IMG_WIENER_MAX);
  return ICS_OK;
}
// the four *_plan entry points: the transform sizes, and bytes(Py, Px) of workspace
template <typename Bytes>
static int wiener_plan(int H, int W, int K, int* Py, int* Px, size_t* workspace_bytes, Bytes bytes) {
  int py = 0, px = 0;
  RC(wiener_shape(H, W, K, &py, &px));
  if (Py) *Py = py;
  if (Px) *Px = px;
  if (workspace_bytes) *workspace_bytes = bytes(py, px);
  return ICS_OK;
}
// the PSF, K x K x 3, as [3][K][K]
static std::vector<float> planar_psf(const float* psf, int K) {
  std::vector<float> planar((size_t)3 * K * K);
  for (int ch = 0; ch < 3; ++ch)
    for (int i = 0; i < K * K; ++i) planar[(size_t)ch * K * K + i] = psf[(size_t)3 * i + ch];
  return planar;
}
// the scalars of the TV solvers; data_penalty: the masked solver's, nullptr without
static int check_tv(float fidelity, float penalty, const float* data_penalty, int iterations, int coupling) {
  if (!std::isfinite(fidelity) || !(fidelity > 0.f)) return ics_set_error(ICS_EINVAL, "fidelity = %g (must be finite and > 0)", (double)fidelity);
  if (!std::isfinite(penalty) || !(penalty > 0.f)) return ics_set_error(ICS_EINVAL, "penalty = %g (must be finite and > 0)", (double)penalty);
  if (data_penalty && (!std::isfinite(*data_penalty) || !(*data_penalty > 0.f)))
    return ics_set_error(ICS_EINVAL, "data_penalty = %g (must be finite and > 0)", (double)*data_penalty);
  if (iterations < 1 || iterations > ICS_IMG_TVD_MAX_ITERATIONS) return ics_set_error(ICS_EINVAL, "iterations = %d (1 .. %d)", iterations, ICS_IMG_TVD_MAX_ITERATIONS);
  return check_coupling(coupling);
}
extern "C" int ics_img_wiener_plan(int H, int W, int K, int* Py, int* Px, size_t* workspace_bytes) {
  return wiener_plan(H, W, K, Py, Px, workspace_bytes, [&](int py, int px) { return 2 * ics_img_wiener_frame_bytes(py, px) + IcsWnTables(nullptr, K, py, px).bytes; });
}
extern "C" int ics_img_wiener(const ics_img* src, const float* psf, int K, float balance, ics_img** out) {
  RC(check_new(src, out));
  if (!psf) return ics_set_error(ICS_EINVAL, "psf is NULL");
  if (!std::isfinite(balance) || !(balance > 0.f)) return ics_set_error(ICS_EINVAL, "balance = %g (must be finite and > 0)", (double)balance);
  const int H = src->H, W = src->W;
  int Py = 0, Px = 0;
  RC(wiener_shape(H, W, K, &Py, &Px));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  ImgOp op(c, out, "img_wiener");
  RC(img_new(c, H, W, out));
  float2 *A = nullptr, *B = nullptr;
  void* tables = nullptr;
  hipError_t e = op.alloc((void**)&A, ics_img_wiener_frame_bytes(Py, Px));
  if (e == hipSuccess) e = op.alloc((void**)&B, ics_img_wiener_frame_bytes(Py, Px));
  if (e == hipSuccess) e = op.alloc(&tables, IcsWnTables(nullptr, K, Py, Px).bytes);
  if (e == hipSuccess) e = put_table(c, IcsWnTables(tables, K, Py, Px).psf, planar_psf(psf, K));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_wiener(src->d, H, W, K, balance, Py, Px, A, B, tables, (*out)->d, c->stream);
  return op.finish(e);
}

// ---- TV-regularised deconvolution of a device image (csrc/ics_img_tvdeconv.hip) ------------------------------------------------------
// One route.  The shapes and the limit are the Wiener filter's; one workspace from the pool, carved by the launcher.
extern "C" int ics_img_tv_deconvolve_plan(int H, int W, int K, int* Py, int* Px, size_t* workspace_bytes) {
  return wiener_plan(H, W, K, Py, Px, workspace_bytes, [&](int py, int px) { return ics_img_tvd_workspace_bytes(K, py, px); });
}
extern "C" int ics_img_tv_deconvolve(const ics_img* src, const float* psf, int K, float fidelity, float penalty, int iterations, int coupling, ics_img** out) {
  RC(check_new(src, out));
  if (!psf) return ics_set_error(ICS_EINVAL, "psf is NULL");
  RC(check_tv(fidelity, penalty, nullptr, iterations, coupling));
  const int H = src->H, W = src->W;
  int Py = 0, Px = 0;
  RC(wiener_shape(H, W, K, &Py, &Px));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  ImgOp op(c, out, "img_tv_deconvolve");
  RC(img_new(c, H, W, out));
  void* ws = nullptr;
  hipError_t e = op.alloc(&ws, ics_img_tvd_workspace_bytes(K, Py, Px));
  if (e == hipSuccess) e = put_table(c, IcsWnTables(ics_img_tvd_tables(ws, Py, Px), K, Py, Px).psf, planar_psf(psf, K));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_tv_deconvolve(src->d, H, W, K, fidelity, penalty, iterations, coupling, Py, Px, ws, (*out)->d, c->stream);
  return op.finish(e);
}

// ---- TV deconvolution of a device image with a masked data term (csrc/ics_img_tvmdeconv.hip) ---------------------------------------
// One route.  The shapes and the limits are those of ics_img_tv_deconvolve; one workspace from the pool, carved by the launcher, the
// caller's mask inside it.  Only the count comes back; the frame stays where it is.
extern "C" int ics_img_tv_deconvolve_masked_plan(int H, int W, int K, int* Py, int* Px, size_t* workspace_bytes) {
  return wiener_plan(H, W, K, Py, Px, workspace_bytes, [&](int py, int px) { return ics_img_tvm_workspace_bytes(K, py, px); });
}
extern "C" int ics_img_tv_deconvolve_masked(const ics_img* src, const float* psf, int K, const unsigned char* observed, float clip, float fidelity, float penalty,
                                            float data_penalty, int iterations, int coupling, long long* unobserved, ics_img** out) {
  RC(check_new(src, out));
  if (!psf) return ics_set_error(ICS_EINVAL, "psf is NULL");
  if (!(clip > 0.f)) return ics_set_error(ICS_EINVAL, "clip = %g (above 0; inf keeps every finite pixel)", (double)clip);
  RC(check_tv(fidelity, penalty, &data_penalty, iterations, coupling));
  const int H = src->H, W = src->W;
  int Py = 0, Px = 0;
  RC(wiener_shape(H, W, K, &Py, &Px));
  ics_ctx* c = src->ctx;
  HIPCHK(hipSetDevice(c->device));
  ImgOp op(c, out, "img_tv_deconvolve_masked");
  RC(img_new(c, H, W, out));
  void* ws = nullptr;
  long long got = 0;
  hipError_t e = op.alloc(&ws, ics_img_tvm_workspace_bytes(K, Py, Px));
  if (e == hipSuccess) e = put_table(c, IcsWnTables(ics_img_tvm_tables(ws, Py, Px), K, Py, Px).psf, planar_psf(psf, K));
  if (e == hipSuccess && observed) {
    e = hipMemcpyAsync(ics_img_tvm_mask_slot(ws, K, Py, Px), observed, (size_t)H * W, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the host buffer may be released by the caller
  }
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess)
    e = ics_launch_img_tv_deconvolve_masked(src->d, H, W, K, observed != nullptr, clip, fidelity, penalty, data_penalty, iterations, coupling, Py, Px, ws, (*out)->d, c->stream);
  if (e == hipSuccess && unobserved) {                 // the count and nothing else
    e = op.end();
    if (e == hipSuccess) e = hipMemcpyAsync(&got, ics_img_tvm_total(ws, Py, Px), sizeof got, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  RC(op.finish(e));
  if (unobserved) *unobserved = got;
  return ICS_OK;
}

// ---- PSF from a sharp / blurred pair of device images (csrc/ics_img_psfest.hip) ---------------------------------------------------------
// One route.  The shapes and the limit are the Wiener filter's for the box; one workspace from the pool, carved by the launcher.  Only
// the raw kernel and the energies come back; the projection to a PSF is a few lines on K K 3 numbers and lives on the host
// (lib/_native.py psf_project).
extern "C" int ics_img_psf_estimate_plan(int H, int W, int K, int* Py, int* Px, size_t* workspace_bytes) {
  return wiener_plan(H, W, K, Py, Px, workspace_bytes, [&](int py, int px) { return ics_img_pe_workspace_bytes(H, W, K, py, px); });
}
static int psf_estimate(const ics_img* blurred, const ics_img* sharp, const ics_mask* mask, int y0, int y1, int x0, int x1, int K, float regularisation,
                        int coupling, float* raw, double energy[3]) {
  if (!blurred || !sharp) return ics_set_error(ICS_EINVAL, "a frame (blurred, sharp) is NULL");
  if (!raw || !energy) return ics_set_error(ICS_EINVAL, "an output (raw, energy) is NULL");
  if (y0 < 0 || x0 < 0 || y0 >= y1 || x0 >= x1) return ics_set_error(ICS_EINVAL, "box [%d, %d) x [%d, %d) (not empty, no negative corner)", y0, y1, x0, x1);
  if (!std::isfinite(regularisation) || !(regularisation > 0.f)) return ics_set_error(ICS_EINVAL, "regularisation = %g (must be finite and > 0)", (double)regularisation);
  RC(check_coupling(coupling));
  const int H = y1 - y0, W = x1 - x0;
  int Py = 0, Px = 0;
  RC(wiener_shape(H, W, K, &Py, &Px));
  if (blurred->ctx != sharp->ctx) return ics_set_error(ICS_EINVAL, "the two frames belong to different contexts");
  if (blurred->H != sharp->H || blurred->W != sharp->W)
    return ics_set_error(ICS_EINVAL, "frames of different shapes: blurred %d x %d, sharp %d x %d", blurred->H, blurred->W, sharp->H, sharp->W);
  if (y1 > sharp->H || x1 > sharp->W) return ics_set_error(ICS_EINVAL, "box [%d, %d) x [%d, %d) outside the %d x %d frames", y0, y1, x0, x1, sharp->H, sharp->W);
  if (mask) {
    if (mask->ctx != sharp->ctx) return ics_set_error(ICS_EINVAL, "the mask belongs to a different context");
    if (mask->H != sharp->H || mask->W != sharp->W) return ics_set_error(ICS_EINVAL, "a %d x %d mask for %d x %d frames", mask->H, mask->W, sharp->H, sharp->W);
    if (mask->planes != (coupling ? 1 : 3)) return ics_set_error(ICS_EINVAL, "a mask of %d planes with coupling %d (one plane: vector, three: channel)", mask->planes, coupling);
  }
  ics_ctx* c = sharp->ctx;
  HIPCHK(hipSetDevice(c->device));
  const long pitch = 3L * sharp->W, first = (long)y0 * pitch + 3L * x0;
  ImgOp op(c, nullptr, "img_psf_estimate");
  void* ws = nullptr;
  std::vector<float> got((size_t)3 * K * K);
  double s[3] = {0.0, 0.0, 0.0};
  hipError_t e = op.alloc(&ws, ics_img_pe_workspace_bytes(H, W, K, Py, Px));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess && !mask) e = ics_launch_img_psf_estimate(sharp->d + first, blurred->d + first, pitch, H, W, K, regularisation, coupling, Py, Px, ws, c->stream);
  if (e == hipSuccess && mask)
    e = ics_launch_img_psf_estimate_masked(sharp->d + first, blurred->d + first, pitch, mask->d + (long)y0 * sharp->W + x0, sharp->W,
                                           mask->planes == 3 ? (long)sharp->H * sharp->W : 0, H, W, K, regularisation, coupling, Py, Px, ws, c->stream);
  if (e == hipSuccess) e = op.end();
  if (e == hipSuccess) e = hipMemcpyAsync(got.data(), ics_img_pe_raw(ws, H, W, K, Py, Px), got.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(s, ics_img_pe_energy(ws, H, W, K, Py, Px), sizeof s, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  RC(op.finish(e));
  std::copy(got.begin(), got.end(), raw);
  for (int ch = 0; ch < 3; ++ch) energy[ch] = s[ch];
  return ICS_OK;
}
extern "C" int ics_img_psf_estimate(const ics_img* blurred, const ics_img* sharp, int y0, int y1, int x0, int x1, int K, float regularisation, int coupling, float* raw,
                                    double energy[3]) {
  return psf_estimate(blurred, sharp, nullptr, y0, y1, x0, x1, K, regularisation, coupling, raw, energy);
}
extern "C" int ics_img_psf_estimate_masked(const ics_img* blurred, const ics_img* sharp, const ics_mask* mask, int y0, int y1, int x0, int x1, int K,
                                           float regularisation, int coupling, float* raw, double energy[3]) {
  if (!mask) return ics_set_error(ICS_EINVAL, "mask is NULL");
  return psf_estimate(blurred, sharp, mask, y0, y1, x0, x1, K, regularisation, coupling, raw, energy);
}

// ---- registration of two device images and the warp of one (csrc/ics_img_align.hip) -----------------------------------------------------
// One route.  The luma pyramids of both frames, the tiles' slots and the sums live in one workspace from the pool; a step is two launches
// and one read-back of at most 67 doubles through the context's pinned area; the damping and the solve, a Cholesky of at most 10 x 10 in
// double, run here.  The loop is restated in tests/align_ref.py (level_loop, align).
namespace {
const int AL_MIN_SIDE = 16, AL_AUTO_SIDE = 64, AL_MAX_LEVELS = ICS_IMG_ALIGN_MAX_LEVELS, AL_MAX_PARAMS = 10, AL_MAX_SUMS = 67;
const double AL_MIN_COVERAGE = 0.25, AL_LAMBDA0 = 1e-6;

struct Mat3 { double m[9]; };
Mat3 al_mul3(const Mat3& a, const Mat3& b) {
  Mat3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
  return r;
}
double al_det3(const Mat3& a) {
  return a.m[0] * (a.m[4] * a.m[8] - a.m[5] * a.m[7]) - a.m[1] * (a.m[3] * a.m[8] - a.m[5] * a.m[6]) + a.m[2] * (a.m[3] * a.m[7] - a.m[4] * a.m[6]);
}
Mat3 al_inv3(const Mat3& a) {   // (of a matrix whose determinant was checked, or of a frame / shift, which has one)
  const double d = 1.0 / al_det3(a);
  const double* m = a.m;
  return Mat3{{(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
               (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
               (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d}};
}
Mat3 al_unit(Mat3 a) { const double w = a.m[8]; for (double& v : a.m) v /= w; return a; }
Mat3 al_frame3(int H, int W) { const double s = (H > W ? H : W) / 2.0; return Mat3{{s, 0.0, (W - 1) / 2.0, 0.0, s, (H - 1) / 2.0, 0.0, 0.0, 1.0}}; }
Mat3 al_shift3(double tx, double ty) { return Mat3{{1.0, 0.0, tx, 0.0, 1.0, ty, 0.0, 0.0, 1.0}}; }
const Mat3 AL_UP = {{2.0, 0.0, 0.5, 0.0, 2.0, 0.5, 0.0, 0.0, 1.0}};   // level l + 1 -> level l: X = 2 (x + 0.5) - 0.5

int al_check_matrix(const double* M) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(M[k])) return ics_set_error(ICS_EINVAL, "the matrix is not finite");
  Mat3 a;
  memcpy(a.m, M, sizeof a.m);
  const double d = al_det3(a);
  if (!(M[8] != 0.0) || !std::isfinite(d) || !(fabs(d) > 0.0)) return ics_set_error(ICS_EINVAL, "the matrix is singular (determinant %g, M[2][2] = %g)", d, M[8]);
  return ICS_OK;
}
int al_check_model(int model) { return model >= 0 && model <= 2 ? ICS_OK : ics_set_error(ICS_EINVAL, "model %d (0 = translation, 1 = affine, 2 = homography)", model); }
int al_check_box(const ics_img* fixed, int y0, int y1, int x0, int x1) {
  if (y0 < 0 || x0 < 0 || y0 >= y1 || x0 >= x1) return ics_set_error(ICS_EINVAL, "box [%d, %d) x [%d, %d) (not empty, no negative corner)", y0, y1, x0, x1);
  if (fixed && (y1 > fixed->H || x1 > fixed->W)) return ics_set_error(ICS_EINVAL, "box [%d, %d) x [%d, %d) outside the %d x %d frame", y0, y1, x0, x1, fixed->H, fixed->W);
  return ICS_OK;
}
int al_levels(int side, int levels, int* used) {
  int n = levels;
  if (levels == 0) for (n = 1; n < AL_MAX_LEVELS && (side >> n) >= AL_AUTO_SIDE; ) ++n;
  if (n < 1 || n > AL_MAX_LEVELS) return ics_set_error(ICS_EINVAL, "levels = %d (0 = automatic, 1 .. %d)", levels, AL_MAX_LEVELS);
  if ((side >> (n - 1)) < AL_MIN_SIDE) return ics_set_error(ICS_EINVAL, "%d level(s) on planes of %d px: no level may be smaller than %d px a side", n, side, AL_MIN_SIDE);
  *used = n;
  return ICS_OK;
}
size_t al_workspace_floats(int Hf, int Wf, int Hm, int Wm, int levels) {
  size_t n = 2 * AL_MAX_SUMS + (size_t)ics_img_al_tiles(Hf, Wf) * AL_MAX_SUMS;   // the sums (as doubles), the slots
  for (int l = 0; l < levels; ++l) n += (size_t)(Hf >> l) * (Wf >> l) + (size_t)(Hm >> l) * (Wm >> l);
  return n;
}
hipError_t al_pin(ics_ctx* c) {
  if (c->pin) return hipSuccess;
  hipError_t e = hipHostMalloc((void**)&c->pin, ics_ctx::PIN_DOUBLES * 8, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming);
  return e;
}

struct AlSums { double S[AL_MAX_PARAMS][AL_MAX_PARAMS], g[AL_MAX_PARAMS], rr, count; };
struct AlLevel { const float *T, *I; int H, W, Hm, Wm; };
struct AlRun {
  ics_ctx* c; int model, photo, n; float* slots; double* out;
  // one evaluation: two launches, the raw sums read back into the context's pinned area, waited for
  hipError_t raw(const AlLevel& lv, const Mat3& A, double gain, double bias) {
    hipError_t e = ics_launch_img_al_sums(lv.T, lv.H, lv.W, lv.I, lv.Hm, lv.Wm, model, photo, A.m, gain, bias, slots, out, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pin, out, (size_t)ics_img_al_slot_floats(model, photo) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
  }
  // ... checked and unpacked: ICS_OK, a refusal (ICS_EINVAL) or ICS_EHIP with *he set
  int evaluate(const AlLevel& lv, const Mat3& A, double gain, double bias, AlSums* s, hipError_t* he) {
    *he = raw(lv, A, gain, bias);
    if (*he != hipSuccess) return ICS_EHIP;
    const double* v = c->pin;
    const int ns = ics_img_al_slot_floats(model, photo);
    for (int k = 0; k < ns; ++k)
      if (!std::isfinite(v[k])) return ics_set_error(ICS_EINVAL, "the frames are not finite: despeckle first");
    int k = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j, ++k) s->S[i][j] = s->S[j][i] = v[k];
    for (int i = 0; i < n; ++i) s->g[i] = v[k++];
    s->rr = v[k]; s->count = v[k + 1];
    if (s->count < AL_MIN_COVERAGE * ((double)lv.H * lv.W)) return ics_set_error(ICS_EINVAL, "frames do not overlap enough (coverage %.3f)", s->count / ((double)lv.H * lv.W));
    return ICS_OK;
  }
};
// (S + lambda diag S) d = -g by Cholesky; false: a pivot that is not > 0
bool al_solve(const AlSums& s, int n, double lambda, double* d) {
  double L[AL_MAX_PARAMS][AL_MAX_PARAMS] = {}, y[AL_MAX_PARAMS];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = s.S[i][j] + (i == j ? lambda * s.S[i][i] : 0.0);
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(v > 0.0) || !std::isfinite(v)) return false;
        L[i][i] = sqrt(v);
      } else L[i][j] = v / L[j][j];
    }
  for (int i = 0; i < n; ++i) { double v = -s.g[i]; for (int k = 0; k < i; ++k) v -= L[i][k] * y[k]; y[i] = v / L[i][i]; }
  for (int i = n - 1; i >= 0; --i) { double v = y[i]; for (int k = i + 1; k < n; ++k) v -= L[k][i] * d[k]; d[i] = v / L[i][i]; }
  return true;
}
// the largest motion, in pixels of the moving plane, of the fixed plane's four corners between A0 and A1
double al_corner_motion(const Mat3& A0, const Mat3& A1, const AlLevel& lv) {
  const Mat3 nf = al_frame3(lv.H, lv.W);
  const double sm = al_frame3(lv.Hm, lv.Wm).m[0];
  double worst = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double x = ((k & 1 ? lv.W - 1 : 0) - nf.m[2]) / nf.m[0], y = ((k & 2 ? lv.H - 1 : 0) - nf.m[5]) / nf.m[0];
    double p[2][2];
    const Mat3* both[2] = {&A0, &A1};
    for (int w = 0; w < 2; ++w) {
      const double* a = both[w]->m;
      const double D = a[6] * x + a[7] * y + a[8];
      p[w][0] = (a[0] * x + a[1] * y + a[2]) / D; p[w][1] = (a[3] * x + a[4] * y + a[5]) / D;
    }
    const double dx = (p[0][0] - p[1][0]) * sm, dy = (p[0][1] - p[1][1]) * sm, m = sqrt(dx * dx + dy * dy);
    if (!(m <= worst)) worst = m;
  }
  return worst;
}
const int AL_INDEX[3][8] = {{2, 5, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7}};   // the entries of A a step moves
}  // namespace

extern "C" int ics_img_align_plan(int H, int W, int levels, int* used, size_t* workspace_bytes) {
  if (H < 1 || W < 1) return ics_set_error(ICS_EINVAL, "bad frame size %d x %d", H, W);
  int n = 0;
  RC(al_levels(H < W ? H : W, levels, &n));
  if (used) *used = n;
  if (workspace_bytes) *workspace_bytes = al_workspace_floats(H, W, H, W, n) * sizeof(float);
  return ICS_OK;
}

namespace {
// what ics_img_align and ics_img_align_sums share: the checks on the pair, the workspace, the luma pyramids
struct AlSetup {
  AlLevel lv[AL_MAX_LEVELS];
  int levels = 0;
  AlRun run{};
};
int al_check_pair(const ics_img* moving, const ics_img* fixed, int y0, int y1, int x0, int x1, int model, const double* M, double gain, double bias) {
  if (!moving || !fixed) return ics_set_error(ICS_EINVAL, "a frame (moving, fixed) is NULL");
  if (!M) return ics_set_error(ICS_EINVAL, "the matrix is NULL");
  RC(al_check_model(model));
  RC(al_check_matrix(M));
  if (!std::isfinite(gain) || !std::isfinite(bias) || gain == 0.0) return ics_set_error(ICS_EINVAL, "gain %g, bias %g (finite, gain not 0)", gain, bias);
  return al_check_box(nullptr, y0, y1, x0, x1);
}
hipError_t al_setup(ImgOp& op, const ics_img* moving, const ics_img* fixed, int y0, int y1, int x0, int x1, int model, int photo, int levels, AlSetup* st) {
  ics_ctx* c = fixed->ctx;
  const int Hf = y1 - y0, Wf = x1 - x0;
  void* ws = nullptr;
  hipError_t e = op.alloc(&ws, al_workspace_floats(Hf, Wf, moving->H, moving->W, levels) * sizeof(float));
  if (e == hipSuccess) e = al_pin(c);
  if (e != hipSuccess) return e;
  st->levels = levels;
  st->run = AlRun{c, model, photo, ics_img_al_params(model, photo), nullptr, reinterpret_cast<double*>(ws)};
  float* at = reinterpret_cast<float*>(ws) + 2 * AL_MAX_SUMS;
  st->run.slots = at; at += (size_t)ics_img_al_tiles(Hf, Wf) * AL_MAX_SUMS;
  e = op.begin();
  for (int l = 0; l < levels && e == hipSuccess; ++l) {
    AlLevel& v = st->lv[l];
    v.H = Hf >> l; v.W = Wf >> l; v.Hm = moving->H >> l; v.Wm = moving->W >> l;
    float* T = at; at += (size_t)v.H * v.W;
    float* I = at; at += (size_t)v.Hm * v.Wm;
    v.T = T; v.I = I;
    if (l == 0) {
      e = ics_launch_img_al_luma(fixed->d + ((size_t)y0 * fixed->W + x0) * 3, 3L * fixed->W, v.H, v.W, T, c->stream);
      if (e == hipSuccess) e = ics_launch_img_al_luma(moving->d, 3L * moving->W, v.Hm, v.Wm, I, c->stream);
    } else {
      e = ics_launch_img_al_half(st->lv[l - 1].T, st->lv[l - 1].H, st->lv[l - 1].W, T, c->stream);
      if (e == hipSuccess) e = ics_launch_img_al_half(st->lv[l - 1].I, st->lv[l - 1].Hm, st->lv[l - 1].Wm, I, c->stream);
    }
  }
  return e;
}
}  // namespace

extern "C" int ics_img_align_sums(const ics_img* moving, const ics_img* fixed, int y0, int y1, int x0, int x1, int model, int photometric, const double M[9], double gain,
                                  double bias, double* sums, int count) {
  RC(al_check_pair(moving, fixed, y0, y1, x0, x1, model, M, gain, bias));
  const int ns = ics_img_al_slot_floats(model, photometric);
  if (!sums || count != ns) return ics_set_error(ICS_EINVAL, "sums of %d entries (this model has %d)", sums ? count : 0, ns);
  if (moving->ctx != fixed->ctx) return ics_set_error(ICS_EINVAL, "the two frames belong to different contexts");
  RC(al_check_box(fixed, y0, y1, x0, x1));
  ics_ctx* c = fixed->ctx;
  HIPCHK(hipSetDevice(c->device));
  ImgOp op(c, nullptr, "img_align_sums");
  AlSetup st;
  hipError_t e = al_setup(op, moving, fixed, y0, y1, x0, x1, model, photometric != 0, 1, &st);
  if (e == hipSuccess) {
    Mat3 m;
    memcpy(m.m, M, sizeof m.m);
    const Mat3 A = al_unit(al_mul3(al_mul3(al_inv3(al_frame3(moving->H, moving->W)), al_mul3(al_unit(m), al_shift3(x0, y0))), al_frame3(y1 - y0, x1 - x0)));
    e = st.run.raw(st.lv[0], A, gain, bias);
  }
  RC(op.finish(e));
  for (int k = 0; k < ns; ++k) sums[k] = c->pin[k];
  return ICS_OK;
}

extern "C" int ics_img_align(const ics_img* moving, const ics_img* fixed, int y0, int y1, int x0, int x1, int model, int photometric, int levels, int iterations,
                             double tolerance, double M[9], double gain_bias[2], double stats[5]) {
  if (!gain_bias || !stats) return ics_set_error(ICS_EINVAL, "an argument (gain_bias, stats) is NULL");
  RC(al_check_pair(moving, fixed, y0, y1, x0, x1, model, M, gain_bias[0], gain_bias[1]));
  if (iterations < 1) return ics_set_error(ICS_EINVAL, "iterations = %d (at least 1)", iterations);
  if (!std::isfinite(tolerance) || !(tolerance > 0.0)) return ics_set_error(ICS_EINVAL, "tolerance = %g (must be finite and > 0)", tolerance);
  if (levels < 0 || levels > AL_MAX_LEVELS) return ics_set_error(ICS_EINVAL, "levels = %d (0 = automatic, 1 .. %d)", levels, AL_MAX_LEVELS);
  if (moving->ctx != fixed->ctx) return ics_set_error(ICS_EINVAL, "the two frames belong to different contexts");
  RC(al_check_box(fixed, y0, y1, x0, x1));
  const int Hf = y1 - y0, Wf = x1 - x0;
  int side = Hf < Wf ? Hf : Wf, used = 0;
  if (moving->H < side) side = moving->H;
  if (moving->W < side) side = moving->W;
  RC(al_levels(side, levels, &used));
  ics_ctx* c = fixed->ctx;
  HIPCHK(hipSetDevice(c->device));
  ImgOp op(c, nullptr, "img_align");
  AlSetup st;
  hipError_t e = al_setup(op, moving, fixed, y0, y1, x0, x1, model, photometric != 0, used, &st);
  if (e != hipSuccess) return op.finish(e);
  const bool photo = photometric != 0;
  const int n = st.run.n, geo = n - (photo ? 2 : 0);
  Mat3 m;
  memcpy(m.m, M, sizeof m.m);
  m = al_mul3(al_unit(m), al_shift3(x0, y0));
  const Mat3 down = al_inv3(AL_UP);
  for (int l = 1; l < used; ++l) m = al_mul3(al_mul3(down, m), AL_UP);
  double gain = gain_bias[0], bias = gain_bias[1];
  int total = 0, rc = ICS_OK;
  double last = 0.0;                    // the corner motion of the last step taken at full resolution
  AlSums cur, nxt;
  for (int l = used - 1; l >= 0 && rc == ICS_OK; --l) {
    const AlLevel& lv = st.lv[l];
    const Mat3 nf = al_frame3(lv.H, lv.W), nm = al_frame3(lv.Hm, lv.Wm);
    Mat3 A = al_unit(al_mul3(al_mul3(al_inv3(nm), m), nf));
    rc = st.run.evaluate(lv, A, gain, bias, &cur, &e);
    double lambda = AL_LAMBDA0;
    for (int step = 0; step < iterations && rc == ICS_OK; ++step) {
      double d[AL_MAX_PARAMS];
      if (!al_solve(cur, n, lambda, d)) { rc = ics_set_error(ICS_EINVAL, "no texture to align on"); break; }
      Mat3 A1 = A;
      for (int k = 0; k < geo; ++k) A1.m[AL_INDEX[model][k]] += d[k];
      const double g1 = photo ? gain + d[n - 2] : gain, b1 = photo ? bias + d[n - 1] : bias;
      rc = st.run.evaluate(lv, A1, g1, b1, &nxt, &e);
      if (rc != ICS_OK) break;
      ++total;
      const double motion = al_corner_motion(A, A1, lv);
      if (l == 0) last = motion;
      if (nxt.rr / nxt.count <= cur.rr / cur.count) { A = A1; gain = g1; bias = b1; cur = nxt; lambda /= 10.0; }
      else lambda *= 10.0;
      if (motion < tolerance) break;
    }
    m = al_unit(al_mul3(al_mul3(nm, A), al_inv3(nf)));
    if (l) m = al_mul3(al_mul3(AL_UP, m), down);
  }
  if (rc == ICS_EHIP) return op.finish(e);
  const int done = op.finish(hipSuccess);
  if (rc != ICS_OK) return rc;          // (a refusal: its message stands)
  RC(done);
  m = al_unit(al_mul3(m, al_shift3(-x0, -y0)));
  memcpy(M, m.m, sizeof m.m);
  gain_bias[0] = gain; gain_bias[1] = bias;
  stats[0] = sqrt(cur.rr / cur.count); stats[1] = cur.count / ((double)Hf * Wf); stats[2] = total; stats[3] = used; stats[4] = last;
  return ICS_OK;
}

extern "C" int ics_img_warp(const ics_img* src, const double M[9], int oh, int ow, ics_img** out) {
  RC(check_new(src, out));
  if (!M) return ics_set_error(ICS_EINVAL, "the matrix is NULL");
  RC(al_check_matrix(M));
  if (oh < 1 || ow < 1) return ics_set_error(ICS_EINVAL, "bad output size %d x %d", oh, ow);
  ImgOp op(src->ctx, out, "img_warp");
  RC(img_new(src->ctx, oh, ow, out));
  hipError_t e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_al_warp(src->d, src->H, src->W, M, (*out)->d, oh, ow, src->ctx->stream);
  return op.finish(e);
}

// ---- guided filter of a device image (csrc/ics_img_guided.hip) ------------------------------------------------------------------
// route 0: the two-launch route at every radius and size ("Guided filter": the measured table).
extern "C" int ics_img_guided(const ics_img* src, int radius, float eps, float detail, int coupling, int route, ics_img** out) {
  RC(check_new(src, out));
  if (radius < 1 || radius > ICS_IMG_GUIDED_MAX_RADIUS) return ics_set_error(ICS_EINVAL, "radius = %d (1 .. %d)", radius, ICS_IMG_GUIDED_MAX_RADIUS);
  if (!std::isfinite(eps) || !(eps > 0.f)) return ics_set_error(ICS_EINVAL, "eps = %g (must be finite and > 0)", (double)eps);
  if (!std::isfinite(detail)) return ics_set_error(ICS_EINVAL, "detail = %g (must be finite)", (double)detail);
  RC(check_coupling(coupling));
  RC(check_route(route, "two launches", "one launch"));
  if (route == 2 && radius > ICS_IMG_GUIDED_FUSED_RADIUS)
    return ics_set_error(ICS_EINVAL, "route 2 takes a radius up to %d, got %d", ICS_IMG_GUIDED_FUSED_RADIUS, radius);
  ics_ctx* c = src->ctx;
  const int H = src->H, W = src->W;
  if (route == 0) route = 1;
  ImgOp op(c, out, "img_guided");
  RC(img_new(c, H, W, out));
  float* coef = nullptr;
  hipError_t e = hipSuccess;
  const size_t floats = ics_img_guided_coef_floats(H, W, coupling, route);
  if (floats) e = op.alloc((void**)&coef, floats * sizeof(float));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_guided(src->d, H, W, radius, eps, detail, coupling, route, coef, (*out)->d, c->stream);
  return op.finish(e);
}

// ---- local Laplacian filter of a device image (csrc/ics_img_llf.hip) ------------------------------------------------------------
// route 0: the batched route at every size.  Measured ("Local Laplacian on a resident frame"; K = 8, default levels, channel /
// vector): at 4096^2 it takes 2.23 / 0.75 ms against 4.01 / 1.36, at 256^2 0.20 / 0.07 against 0.78 / 0.27, and at 64^2, where one
// workgroup walks all nine pyramids of its tile, 0.13 / 0.045 against 0.35 / 0.12: no crossover.
extern "C" int ics_img_local_laplacian(const ics_img* src, float sigma, float detail, float edges, int levels, int samples, int coupling, int route,
                                       ics_img** out) {
  RC(check_new(src, out));
  if (!std::isfinite(sigma) || !(sigma > 0.f)) return ics_set_error(ICS_EINVAL, "sigma = %g (must be finite and > 0)", (double)sigma);
  if (!std::isfinite(detail) || !(detail >= 0.f)) return ics_set_error(ICS_EINVAL, "detail = %g (must be finite and >= 0)", (double)detail);
  if (!std::isfinite(edges) || !(edges > 0.f)) return ics_set_error(ICS_EINVAL, "edges = %g (must be finite and > 0)", (double)edges);
  if (detail > 3.f * edges) return ics_set_error(ICS_EINVAL, "detail = %g above 3 edges = %g (the remap must stay monotone)", (double)detail, (double)(3.f * edges));
  if (levels < 1 || levels > ICS_IMG_LLF_MAX_LEVELS) return ics_set_error(ICS_EINVAL, "levels = %d (1 .. %d)", levels, ICS_IMG_LLF_MAX_LEVELS);
  if (samples < 2 || samples > ICS_IMG_LLF_MAX_SAMPLES) return ics_set_error(ICS_EINVAL, "samples = %d (2 .. %d)", samples, ICS_IMG_LLF_MAX_SAMPLES);
  RC(check_coupling(coupling));
  RC(check_route(route, "per sample", "samples batched"));
  ics_ctx* c = src->ctx;
  const int H = src->H, W = src->W;
  if (route == 0) route = 2;
  ImgOp op(c, out, "img_local_laplacian");
  RC(img_new(c, H, W, out));
  float *pyr = nullptr, *r0 = nullptr, *r1 = nullptr;
  hipError_t e = op.alloc((void**)&pyr, ics_img_llf_pyramid_floats(H, W, levels, samples) * sizeof(float));
  if (e == hipSuccess) e = op.alloc((void**)&r0, ics_img_llf_collapse_floats(H, W) * sizeof(float));
  if (e == hipSuccess) e = op.alloc((void**)&r1, ics_img_llf_collapse_floats(H, W) * sizeof(float));
  if (e == hipSuccess) e = op.begin();
  if (e == hipSuccess) e = ics_launch_img_llf(src->d, H, W, sigma, detail, edges, levels, samples, coupling, route, pyr, r0, r1, (*out)->d, c->stream);
  return op.finish(e);
}
