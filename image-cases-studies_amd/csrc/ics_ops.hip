// ics_ops.hip -- the standalone operators of the C ABI (include/ics_hip.h) on host arrays: PSF normalisation, TV, and the float64
// filters of lib/utils.py (convolution, unsharp mask, bilateral) and the bicubic resize.  Host side only; kernels live in ics_kernels.hip /
// ics_filters.hip / ics_resize.hip.
#include "ics_host.h"

using namespace ics_host;

extern "C" int ics_normalize_kernel(ics_ctx* c, float* kern, int MK) {
  if (!c || !kern) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (MK < 1) return ics_set_error(ICS_EINVAL, "MK = %d", MK);
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)3 * MK * MK;
  float* d = nullptr;
  HIPCHK(c->pool.alloc((void**)&d, n * 4));
  hipError_t e = hipMemcpyAsync(d, kern, n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = ics_launch_normalize(d, MK, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(kern, d, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  c->pool.release(d);
  if (e != hipSuccess) return ics_set_error(ICS_EHIP, "normalize_kernel: %s", hipGetErrorString(e));
  return ICS_OK;
}

extern "C" int ics_tv(ics_ctx* c, const float* u, int M, int N, float eps, int order, int norm, float* out, float* div) {
  if (!c || !u || !out || !div) return ics_set_error(ICS_EINVAL, "NULL argument");
  if ((order != 1 && order != 2) || (norm != 1 && norm != 2)) return ics_set_error(ICS_EINVAL, "order/norm must be 1 or 2");
  if (M < 1 || N < 1) return ics_set_error(ICS_EINVAL, "size %dx%d", M, N);
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)M * N * 3;
  float *du = nullptr, *dout = nullptr, *ddiv = nullptr;
  hipError_t e = c->pool.alloc((void**)&du, n * 4);
  if (e == hipSuccess) e = c->pool.alloc((void**)&dout, n * 4);
  if (e == hipSuccess) e = c->pool.alloc((void**)&ddiv, n * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(du, u, n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(dout, 0, n * 4, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ddiv, 0, n * 4, c->stream);
  if (e == hipSuccess) e = ics_launch_tv(du, M, N, eps, order, norm, dout, ddiv, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(div, ddiv, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  c->pool.release(du); c->pool.release(dout); c->pool.release(ddiv);
  if (e != hipSuccess) return ics_set_error(e == hipErrorOutOfMemory ? ICS_ENOMEM : ICS_EHIP, "tv: %s", hipGetErrorString(e));
  return ICS_OK;
}

// Rank-1 test: kern == outer(col, row)?  Every window of lib/utils.py (uniform, gaussian, kaiser, poisson) is an outer product
// normalised by its sum; the two 1-D factors are taken through the largest element.
bool ics_host::rank1_factors(const double* k, int KH, int KW, std::vector<double>& col, std::vector<double>& row, double tol) {
  int r = 0, c = 0; double m = 0.0;
  for (int i = 0; i < KH; ++i) for (int j = 0; j < KW; ++j) if (fabs(k[i * KW + j]) > m) { m = fabs(k[i * KW + j]); r = i; c = j; }
  if (m == 0.0 || KH == 1 || KW == 1) return false;
  const double piv = k[r * KW + c];
  for (int i = 0; i < KH; ++i)
    for (int j = 0; j < KW; ++j)
      if (fabs(k[i * KW + j] * piv - k[i * KW + c] * k[r * KW + j]) > tol * m * m) return false;
  col.resize(KH); row.resize(KW);
  for (int i = 0; i < KH; ++i) col[i] = k[i * KW + c] / piv;
  for (int j = 0; j < KW; ++j) row[j] = k[r * KW + j];
  return true;
}

static int conv2d_common(ics_ctx* c, const double* src, int H, int W, const double* kern, int KH, int KW, int usm, double amount, double* out) {
  if (!c || !src || !kern || !out) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (H < 1 || W < 1 || KH < 1 || KW < 1) return ics_set_error(ICS_EINVAL, "bad sizes");
  if ((size_t)(32 + KH - 1) * (32 + KW - 1) * 8 > 160 * 1024) return ics_set_error(ICS_ENOSUP, "kernel %d x %d too large for the LDS tile (up to 112 x 112: (31 + KH) * (31 + KW) doubles within 160 KB)", KH, KW);
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)H * W, nk = (size_t)KH * KW;
  std::vector<double> col, row;
  const bool sep = rank1_factors(kern, KH, KW, col, row);
  void* base = nullptr;
  int rc = ctx_scratch(c, (3 * n + nk + KH + KW + 16) * 8, &base);
  if (rc != ICS_OK) return ics_set_error(rc, "device scratch of %zu bytes", (3 * n + nk) * 8);
  double *ds = (double*)base, *dout = ds + n, *dtmp = dout + n, *dk = dtmp + n;
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, s));
  if (sep) {
    HIPCHK(hipMemcpyAsync(dk, row.data(), KW * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dk + KW, col.data(), KH * 8, hipMemcpyHostToDevice, s));
  } else {
    HIPCHK(hipMemcpyAsync(dk, kern, nk * 8, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipEventRecord(c->ev0, s));
  if (sep) {   // rows (1 x KW), then columns (KH x 1) with the USM epilogue against the original channel
    HIPCHK(ics_launch_conv2d_symm(ds, H, W, dk, 1, KW, dtmp, ds, 0, 0.0, s));
    HIPCHK(ics_launch_conv2d_symm(dtmp, H, W, dk + KW, KH, 1, dout, ds, usm, amount, s));
  } else {
    HIPCHK(ics_launch_conv2d_symm(ds, H, W, dk, KH, KW, dout, ds, usm, amount, s));
  }
  HIPCHK(hipEventRecord(c->ev1, s));
  HIPCHK(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));   // (col / row are host vectors read by the async copies above)
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  return ICS_OK;
}

extern "C" int ics_conv2d_symm(ics_ctx* c, const double* src, int H, int W, const double* kern, int KH, int KW, double* out) {
  return conv2d_common(c, src, H, W, kern, KH, KW, 0, 0.0, out);
}
extern "C" int ics_usm(ics_ctx* c, const double* src, int H, int W, const double* kern, int KH, int KW, double amount, double* out) {
  return conv2d_common(c, src, H, W, kern, KH, KW, 1, amount, out);
}

extern "C" int ics_bilateral(ics_ctx* c, const double* src, int H, int W, int radius, double std_i, double std_s, double* out) {
  if (!c || !src || !out) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (H < 1 || W < 1 || radius < 0) return ics_set_error(ICS_EINVAL, "bad sizes");
  if ((size_t)(32 + 2 * radius) * (32 + 2 * radius) * 8 > 160 * 1024) return ics_set_error(ICS_ENOSUP, "radius %d too large for the LDS tile (up to 55)", radius);
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)H * W;
  const int D = 2 * radius + 1;
  std::vector<double> ws((size_t)D * D);
  for (int j = -radius; j <= radius; ++j)
    for (int i = -radius; i <= radius; ++i) ws[(size_t)(j + radius) * D + (i + radius)] = exp((double)(i * i + j * j) * (-1.0 / (2.0 * std_s * std_s)));
  void* base = nullptr;
  int rc = ctx_scratch(c, (2 * n + ws.size() + 16) * 8, &base);
  if (rc != ICS_OK) return ics_set_error(rc, "device scratch of %zu bytes", 2 * n * 8);
  double *ds = (double*)base, *dout = ds + n, *dws = dout + n;
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dws, ws.data(), ws.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(c->ev0, s));
  HIPCHK(ics_launch_bilateral(ds, H, W, radius, std_i, dws, dout, s));
  HIPCHK(hipEventRecord(c->ev1, s));
  HIPCHK(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  return ICS_OK;
}

// deconvolve.py:245-249 -- skimage.transform.resize(order=3, mode="edge") restated on scipy.ndimage semantics (oracle/resize_oracle.py)
extern "C" int ics_resize_bicubic(ics_ctx* c, const double* src, int H, int W, int C, double* out, int OH, int OW) {
  if (!c || !src || !out) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (H < 2 || W < 2 || C < 1 || OH < 1 || OW < 1) return ics_set_error(ICS_EINVAL, "bad sizes");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)H * W * C, no = (size_t)OH * OW * C;
  // Gaussian anti-aliasing weights (host, float64 like scipy.ndimage.gaussian_filter1d)
  auto weights = [](double sigma, std::vector<double>& w) {
    const int r = (int)(4.0 * sigma + 0.5);
    w.resize(2 * r + 1);
    double sum = 0.0;
    for (int k = -r; k <= r; ++k) { w[k + r] = exp(-0.5 / (sigma * sigma) * (double)k * (double)k); sum += w[k + r]; }
    for (double& v : w) v /= sum;
    return r;
  };
  const double sy = fmax(0.0, ((double)H / OH - 1.0) / 2.0), sx = fmax(0.0, ((double)W / OW - 1.0) / 2.0);
  const bool smooth = (sy > 0.0 || sx > 0.0) && !(H == OH && W == OW);
  std::vector<double> hwy, hwx;
  int ry = 0, rx = 0;
  if (smooth && sy > 1e-15) ry = weights(sy, hwy);
  if (smooth && sx > 1e-15) rx = weights(sx, hwx);
  double *ds = nullptr, *scr = nullptr, *dout = nullptr, *dw = nullptr;
  hipError_t e = c->pool.alloc((void**)&ds, n * 8);
  if (e == hipSuccess) e = c->pool.alloc((void**)&scr, ics_resize_scratch_doubles(H, W, C) * 8);
  if (e == hipSuccess) e = c->pool.alloc((void**)&dout, no * 8);
  if (e == hipSuccess) e = c->pool.alloc((void**)&dw, (hwy.size() + hwx.size() + 1) * 8);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && !hwy.empty()) e = hipMemcpyAsync(dw, hwy.data(), hwy.size() * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && !hwx.empty()) e = hipMemcpyAsync(dw + hwy.size(), hwx.data(), hwx.size() * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    if (H == OH && W == OW) e = hipMemcpyAsync(dout, ds, n * 8, hipMemcpyDeviceToDevice, c->stream);
    else e = ics_launch_resize(ds, H, W, C, hwy.empty() ? nullptr : dw, ry, hwx.empty() ? nullptr : dw + hwy.size(), rx, scr, dout, OH, OW, c->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, no * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (also keeps hwy / hwx alive until the copies are done)
  c->pool.release(ds); c->pool.release(scr); c->pool.release(dout); c->pool.release(dw);
  if (e != hipSuccess) return ics_set_error(e == hipErrorOutOfMemory ? ICS_ENOMEM : ICS_EHIP, "resize: %s", hipGetErrorString(e));
  return ICS_OK;
}
