// ics_context.hip -- the part of the C ABI of libics_hip.so (include/ics_hip.h) that belongs to no job: ABI and size queries, the
// debug switches, the error channel, device count, contexts (stream, block pool -- ics_host.h IcsPool -- and pinned staging area).
// Host side only.
#include "ics_host.h"

using namespace ics_host;

// -------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int ics_set_error(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}

extern "C" int ics_abi_version(void) { return ICS_ABI_VERSION; }
extern "C" size_t ics_rl_params_size(void) { return sizeof(ics_rl_params); }
extern "C" size_t ics_rl_stats_size(void) { return sizeof(ics_rl_stats); }

// test / measurement switches (ics_common.h IcsDebug): exported, deliberately absent from include/ics_hip.h
static std::atomic<int>* debug_switch(const char* name) {
  IcsDebug& d = ics_debug();
  const struct { const char* n; std::atomic<int>* v; } tab[] = {
      {"max_wgs", &d.max_wgs}, {"dynamic_tiles", &d.dynamic_tiles}, {"conv_rs", &d.conv_rs}, {"conv_path", &d.conv_path},
      {"fused_gradk", &d.fused_gradk}, {"update_kernel", &d.update_kernel}, {"fused_rs", &d.fused_rs},
      {"planar_image", &d.planar_image}, {"pam_exact", &d.pam_exact}, {"fail_window_alloc", &d.fail_window_alloc}, {"pool_limit_mb", &d.pool_limit_mb}, {"overlap", &d.overlap}, {"fft_gradk", &d.fft_gradk}, {"fft_fused", &d.fft_fused}, {"fft_conv2", &d.fft_conv2}, {"fft_rot", &d.fft_rot}, {"fft_psf1", &d.fft_psf1}, {"fft_maxg", &d.fft_maxg}, {"key_trace", &d.key_trace}, {"maxg_scanned", &d.maxg_scanned}, {"maxg_pairs", &d.maxg_pairs}, {"maxg_total", &d.maxg_total}, {"maxg_launches", &d.maxg_launches}, {"small_iter", &d.small_iter}, {"small_trace", &d.small_trace}, {"fail_small_launch", &d.fail_small_launch},
      {"pool_check", &d.pool_check}, {"pool_overruns", &d.pool_overruns}, {"pool_selftest", &d.pool_selftest}};
  for (auto& t : tab)
    if (strcmp(t.n, name) == 0) return t.v;
  return nullptr;
}
extern "C" int ics_debug_set(const char* name, int value) {
  std::atomic<int>* v = name ? debug_switch(name) : nullptr;
  if (!v) return -1;
  v->store(value, std::memory_order_relaxed);
  return 0;
}
extern "C" int ics_debug_get(const char* name, int* value) {
  std::atomic<int>* v = name && value ? debug_switch(name) : nullptr;
  if (!v) return -1;
  *value = v->load(std::memory_order_relaxed);
  return 0;
}
extern "C" const char* ics_last_error(void) { return g_err; }

extern "C" int ics_device_count(int* count) {
  if (!count) return ics_set_error(ICS_EINVAL, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return ics_set_error(ICS_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *count = n;
  return ICS_OK;
}

extern "C" int ics_ctx_create(int device, ics_ctx** out) {
  if (!out) return ics_set_error(ICS_EINVAL, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return ics_set_error(ICS_ENODEV, "no HIP device available (%s); libics_hip has no CPU fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  if (device < 0 || device >= n) return ics_set_error(ICS_EINVAL, "device %d out of range (0..%d)", device, n - 1);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return ics_set_error(ICS_ENODEV, "device %d is %s; this library only contains gfx950 (MI355X) code", device, prop.gcnArchName);
  ics_ctx* c = new ics_ctx();
  c->device = device;
  c->scratch = nullptr; c->scratch_bytes = 0; c->last_ms = 0.f;
  {
    const int lim = ics_debug().pool_limit_mb.load(std::memory_order_relaxed);   // ICS_POOL_LIMIT_MB, read once per process
    c->pool.limit = lim >= 0 ? (size_t)lim << 20 : (size_t)prop.totalGlobalMem / 4;
  }
  hipEventCreate(&c->ev0); hipEventCreate(&c->ev1);
  c->cus = prop.multiProcessorCount;
  c->hbm = prop.totalGlobalMem;
  snprintf(c->name, sizeof c->name, "%s (%s)", prop.name, prop.gcnArchName);
  hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (se != hipSuccess) { delete c; return ics_set_error(ICS_EHIP, "hipStreamCreate: %s", hipGetErrorString(se)); }
  c->pool.dev.stream = c->stream;
  *out = c;
  return ICS_OK;
}

extern "C" void ics_ctx_destroy(ics_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  if (c->scratch) c->pool.release(c->scratch);
  c->pool.clear();
  if (c->pin) hipHostFree(c->pin);
  if (c->pin_ev) hipEventDestroy(c->pin_ev);
  if (c->stream2) { hipStreamSynchronize(c->stream2); hipStreamDestroy(c->stream2); }
  hipEventDestroy(c->ev0); hipEventDestroy(c->ev1);
  hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int ics_ctx_synchronize(ics_ctx* c) {
  if (!c) return ics_set_error(ICS_EINVAL, "ctx is NULL");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  return ICS_OK;
}

extern "C" int ics_ctx_last_kernel_ms(ics_ctx* c, float* ms) {
  if (!c || !ms) return ics_set_error(ICS_EINVAL, "NULL argument");
  if (c->ev_pending) {   // a queued ics_img_convolve / _usm / _bilateral recorded ev0 / ev1 and did not wait for them
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev1));
    HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    c->ev_pending = false;
  }
  *ms = c->last_ms;
  return ICS_OK;
}

extern "C" int ics_ctx_info(ics_ctx* c, char* name, size_t name_len, int* cus, uint64_t* hbm) {
  if (!c) return ics_set_error(ICS_EINVAL, "ctx is NULL");
  if (name && name_len) { strncpy(name, c->name, name_len - 1); name[name_len - 1] = 0; }
  if (cus) *cus = c->cus;
  if (hbm) *hbm = c->hbm;
  return ICS_OK;
}

// ---- the pinned staging area (the image filters of ics_images.hip) --------------------------------------------------------------
// A small host table (kernel factors, spatial weights) -> device, queued.  It goes through the context's pinned staging area:
// the copy reads memory the context owns, `pin_ev` marks it and the next writer of the area waits for that event, so the
// caller's vector may die at once and the stream is not synchronised.  Only a table larger than the area (64 KB) is copied
// from pageable memory, and then that copy alone is waited for before the vector goes out of scope.
hipError_t ics_host::put_table(ics_ctx* c, float* dev, const std::vector<float>& t) {
  const size_t bytes = t.size() * sizeof(float);
  hipStream_t s = c->stream;
  hipError_t e = hipSuccess;
  if (bytes > ics_ctx::PIN_DOUBLES * 8) {
    e = hipMemcpyAsync(dev, t.data(), bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
  }
  if (!c->pin) { e = hipHostMalloc((void**)&c->pin, ics_ctx::PIN_DOUBLES * 8, hipHostMallocDefault); if (e == hipSuccess) e = hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming); }
  if (e == hipSuccess && c->pin_used) e = hipEventSynchronize(c->pin_ev);
  if (e != hipSuccess) return e;
  memcpy(c->pin, t.data(), bytes);
  e = hipMemcpyAsync(dev, c->pin, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(c->pin_ev, s);
  c->pin_used = true;
  return e;
}
