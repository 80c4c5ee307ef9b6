// ics_host.h -- what the host translation units of libics_hip.so share (ics_context.hip, ics_job.hip, ics_route.hip, ics_run.hip,
// ics_ops.hip, ics_images.hip, ics_group.hip): the error channel, the context with its block pool, the device-resident job, device
// images, the event-bracket profiler, the route of a run, and the helpers that cross a unit boundary (namespace ics_host).
// Host side only: kernel units include ics_kernels.h / ics_common.h (the device-image filter units through ics_img_px.h), not this.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>
#include <map>
#include <mutex>
#include <unordered_map>

#include "../../include/ics_hip.h"
#include "ics_kernels.h"
#include "ics_image_acc.h"
#include "ics_pool.h"

// -------------------------------------------------------------------------------------------------
// the error channel: formats the message ics_last_error returns (thread-local, ics_context.hip) and returns `code`
int ics_set_error(int code, const char* fmt, ...);
#define HIPCHK(x)                                                                                \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess)                                                                        \
      return ics_set_error(e_ == hipErrorOutOfMemory ? ICS_ENOMEM : ICS_EHIP, "%s failed: %s (%s:%d)", #x, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                                    \
  } while (0)

#define RC(x) do { int rc_ = (x); if (rc_ != ICS_OK) return rc_; } while (0)
#define RC0(x) do { int rc0_ = (x); if (rc0_ != ICS_OK) return rc0_; } while (0)   // (inside Prof: its callers wrap it in RC)

// The block pool of a context (ics_pool.h: recycling, rounding, and the check mode behind the debug switches pool_check /
// pool_overruns / pool_selftest) over the four HIP calls it needs.  The fills go to the context's stream, like everything the owner
// of a block queues; the read-back of a red zone waits for the whole device first (the overlapped statistics run on stream2).
struct IcsPoolHip {
  typedef hipError_t err_t;
  hipStream_t stream = nullptr;                  // the context's (ics_ctx_create)
  static hipError_t alloc(void** p, size_t bytes) { hipError_t e = hipMalloc(p, bytes); if (e != hipSuccess) (void)hipGetLastError(); return e; }
  static void free(void* p) { (void)hipFree(p); }
  hipError_t fill(void* p, int byte, size_t bytes) const { return hipMemsetAsync(p, byte, bytes, stream); }
  static hipError_t copy_back(void* host, const void* p, size_t bytes) {
    hipError_t e = hipDeviceSynchronize();
    return e != hipSuccess ? e : hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost);
  }
};
struct IcsPool : IcsPoolT<IcsPoolHip> {
  IcsPool() : IcsPoolT<IcsPoolHip>(&ics_debug().pool_check, &ics_debug().pool_overruns, &ics_debug().pool_selftest) {}
};

struct ics_ctx {
  IcsPool pool;
  int device;
  hipStream_t stream;
  int cus;
  char name[256];
  uint64_t hbm;
  void* scratch;            // device scratch of the standalone operators: grown on demand, kept between calls
  size_t scratch_bytes;
  bool scratch_checked = false;   // the scratch was handed out in the pool's check mode (ctx_scratch)
  hipEvent_t ev0, ev1;      // device time of the last standalone operator (kernels only, no transfers)
  float last_ms;
  // small pinned staging area for host -> device parameters of queued operations (the Gaussian weights of ics_img_resize): the copy
  // reads it asynchronously, `pin_ev` marks the last copy, the next writer waits for it (long done in practice) -- no stream
  // synchronisation per operation
  // second stream: the stop-test statistics of outer iteration i run here while the job's stream already works on iteration i + 1
  // (ics_rl_run, "overlap"; the events that order the two streams belong to the job)
  hipStream_t stream2 = nullptr;
  double* pin = nullptr;
  hipEvent_t pin_ev = nullptr;
  bool pin_used = false;
  static constexpr size_t PIN_DOUBLES = 8192;
  bool ev_pending = false;  // ev0 / ev1 were recorded by a queued image filter: ics_ctx_last_kernel_ms reads them on demand
};

struct ics_rl {
  ics_ctx* ctx;
  IcsGeom g;
  size_t frame_floats, origin;
  float *u, *u2, *ut, *gr, *f, *e;     // frame bases (origin = base + origin); u2 = ping-pong partner of u
  float* tvf;                           // TV term frame (tv_mode 1, allocated on first use)
  float* facc[2];                       // the image in accumulator order for 32-row / 64-row tiles (ics_image_acc.h), allocated on first use
  bool facc_valid[2];                   // ... and whether it still mirrors the image frame
  float *psf, *gradk, *wconv, *wcorr, *psf_caller, *partial;
  // k_psf_spectra (blind runs on the tiles, Route::psf1) reads `psf` and writes `psf_next`; do_psf exchanges the two pointers behind the
  // launch, so whatever is queued afterwards -- kernels, copies to and from psf_bak, downloads -- takes the stepped PSF through `psf` in
  // stream order.  No pointer to either buffer is kept across launches.
  float* psf_next;
  size_t partial_floats;                // size of `partial`
  float* psf_work;                      // PSF sizes above 63: working copy of k_psf (3*K*K floats), else NULL
  // overlap of the statistics with the next outer iteration: the reduction slots / DoF keys of outer iteration i are the set i & 1
  // (`par`; the stage API always uses set 0), the residual frame ping-pongs with e2, the PSF of the last finished iteration is kept
  int par;
  hipEvent_t ev_body[2], ev_stats[2];   // [i & 1]: iteration i's kernels are done / its scalars are on the host (created with e2)
  float* e2;                            // second residual frame (first overlapped run)
  float* psf_bak;                       // psf + psf_caller as they were when the running outer iteration started (blind, overlapped)
  double* gradk64;                      // row bands over several ranks: the gradient sums as float64 for the cross-rank all-reduce (first use)
  // PSF sizes 51 ... 255 on the matrix cores as nblk x nblk tap blocks of Kb x Kb (do_conv_blocks): weight tables of both
  // orientations, a scratch frame for the block results
  int blk_n, blk_kb;
  float *blk_conv, *blk_corr, *blk_scr, *blk_negf;   // blk_negf: -image (even block counts only: the chain of do_conv_blocks starts from it)
  bool negf_valid;
  uint32_t* blk_red;                    // reduction slots the block passes may scribble on (the maxima are taken over the sum)
  float *bt_conv, *bt_corr;  // Toeplitz fragment tables of the matrix-core convolution (MK <= 37), else NULL
  int gradk_blocks;
  int fused2_blocks;                    // persistent workgroups of the 32-row fused A11 + A13 kernel: three per CU (capped like gradk_blocks by the test switch)
  uint32_t* red;                        // INNER slots x ICS_RED_STRIDE keys
  uint32_t* dofkeys;                    // 4 words
  uint32_t* sched;                      // 16 words: tile-walk counters of the matrix-core convolutions (IcsConvArgs::sched)
  float* scal;                          // ICS_SC_COUNT
  double* dacc;                         // 8 accumulators of the window statistics
  uint32_t* ukey;                       // 2
  int* flags;                           // [0] frozen, [1] hasnan
  // stop-test scratch (allocated for the window of the last run)
  float2* z; float2* tw; float* weights;
  int P, logP, wt, wb, wl, wr;
  int Py, Px;                           // long-line path (a window side above 4096 px): per-axis transform sizes; 0 = the P x P path
  bool win_empty;
  float* h_scal;                        // pinned host mirror of scal (+ flags)
  bool uploaded;
  bool ut_is_u;                         // majoriser aliased to u (first inner iteration of an outer one, no copy made yet)
  // profiling
  std::vector<hipEvent_t> ev;
  struct EvPair { int b, e, cls; };     // a bracketed launch group: events ev[b] .. ev[e]
  std::vector<EvPair> ev_pairs;
  size_t ev_used;
  int ev_open = -1, ev_open_cls = 0;    // begin() without its end() yet
  int ev_chain = -1;                    // the event the last end() recorded, while nothing else has been queued behind it (Prof::begin)
  hipStream_t ev_chain_stream = nullptr;
  hipEvent_t ev_begin, ev_end;
  // FFT-tile pipeline (round 5; ics_conv_fft.hip, ics_planar.hip): channel-planar mirrors of the frames (ics_common.h), allocated by the
  // first run that uses it.  A mirror belongs to a BUFFER, not to a role: u / ut / u2 and e / e2 rotate as pointers, the table is looked
  // up by the HWC pointer's value.  fft_on = the mirrors hold the live frames of a run / stage on the pipeline (its route's `tiles`):
  // pack_weights also builds the two spectra.
  struct Twin { float* hwc; float* pl; };
  Twin twins[8];
  int ntwins;
  float *spec_conv, *spec_corr;
  float* fspec;         // mode 2 of the tile convolutions (A1 + A3 in one unit): the image windows' spectra, valid while fspec_valid
  bool fspec_valid;
  bool conv2_off;       // the spectra did not fit the device memory once: this job runs A1 and A3 as two kernels from then on
  // mode 2 without the epilogue's operands (Route::maxg; ics_maxg_select.h): the device words of a run and the tile maxima of a launch, allocated
  // by the first run that takes the route.  mgs_ready: an update pass of THIS run has recorded max u and Dmax into set mgs_set, so the next mode-2
  // launch may be the operand-free one; cleared when a run starts (its first launch reads its operands) -- and a run that ends through undo() ends.
  uint32_t *mgs, *mgs_wave;
  bool mgs_ready;
  int mgs_set;
  // debug switch key_trace: the reduction slot every update pass of the last run read, one copy of ICS_RED_STRIDE words per inner iteration
  // (the first ICS_KEY_TRACE_SLOTS of them), for ics_debug_key_trace
  uint32_t* ktrace;
  int ktrace_n;
  bool fft_on;
  bool plf_valid;                       // the mirror of the image frame still mirrors it (every writer of j->f calls image_changed)
  // small frames (ics_small.hip): the inner iterations of an outer one as a cooperative launch
  float* small_part;                    // the tiles' shares of the PSF gradient (3 x tiles x K^2)
  unsigned long long* small_bar;        // the grid barrier's counters, zeroed at the start of a run
  unsigned long long* small_keys;       // the tiles' step-size maxima (8 x workgroups)
  unsigned long long small_gen;         // barriers passed since then
  bool small_off;                       // the cooperative launch was refused once: this job stays on the multi-launch path
  bool small_bak;                       // the next cooperative launch first copies psf / psf_caller to psf_bak (overlapped statistics, blind)
};

struct ics_img {
  ics_ctx* ctx;
  int H, W;
  float* d;
};

struct ics_mask {              // byte planes of a device image's size (ics_img_edge_mask): planes x H x W, 0 or 1
  ics_ctx* ctx;
  int H, W, planes;
  unsigned char* d;
};

// ---- everything below is internal to the host units -----------------------------------------------------------------------------
namespace ics_host {

// at least `bytes` of device scratch that persists between calls (no hipMalloc / hipFree per filter call)
static inline int ctx_scratch(ics_ctx* c, size_t bytes, void** p) {
  // (pool check mode: a block per call, so that the scratch is filled and its red zone verified like everything else; the first call
  //  after the mode is switched off returns the last such block)
  const bool check = ics_debug().pool_check.load(std::memory_order_relaxed) >= 0;
  if (c->scratch_bytes < bytes || check || c->scratch_checked) {
    if (c->scratch) { c->pool.release(c->scratch); c->scratch = nullptr; c->scratch_bytes = 0; }
    const size_t want = bytes + bytes / 4;
    hipError_t e = c->pool.alloc(&c->scratch, want);
    if (e != hipSuccess) { (void)hipGetLastError(); c->scratch = nullptr; return ICS_ENOMEM; }
    c->scratch_bytes = want; c->scratch_checked = check;
  }
  *p = c->scratch;
  return ICS_OK;
}

static inline int rect_ok(const ics_img* m, int y0, int x0, int H, int W) { return y0 >= 0 && x0 >= 0 && H >= 1 && W >= 1 && y0 + H <= m->H && x0 + W <= m->W; }

static inline float* org(ics_rl* j, float* base) { return base + j->origin; }
static inline float* pl_of(ics_rl* j, const float* hwc) {
  for (int i = 0; i < j->ntwins; ++i) if (j->twins[i].hwc == hwc) return j->twins[i].pl;
  return nullptr;
}
// origin of the planar mirror of an HWC frame buffer
static inline float* porg(ics_rl* j, const float* hwc) { float* p = pl_of(j, hwc); return p ? p + ics_planar_origin(j->g) : nullptr; }
// majoriser frame: pyx:462 `ut = u.copy()` is realised without a copy -- until the first update of the outer
// iteration ut IS u; that update writes out of place and the old u frame becomes ut (buffer rotation)
static inline float* ut_of(ics_rl* j) { return j->ut_is_u ? j->u : j->ut; }
static inline uint32_t* red_of(ics_rl* j) { return j->red + (size_t)j->par * 8 * ICS_RED_STRIDE; }
static inline uint32_t* dof_of(ics_rl* j) { return j->dofkeys + 4 * j->par; }

// the accumulator-order copies of the image follow the image frame: every writer of j->f calls this
static inline void image_changed(ics_rl* j) { j->facc_valid[0] = j->facc_valid[1] = false; j->negf_valid = false; j->plf_valid = false; j->fspec_valid = false; }

#define ICS_KEY_TRACE_SLOTS 64
#define ICS_PSF_MAX 255   // PSF sizes: odd, 3 ... ICS_PSF_MAX (psf_supported, ics_route.hip)

// Device allocation, zero-filled ON THE GIVEN STREAM: the job's stream is non-blocking, so a
// null-stream hipMemset would not be ordered with the uploads/kernels that follow on it.
template <typename T>
static int dalloc(ics_ctx* c, T** p, size_t count, bool zero = true) {
  *p = nullptr;
  if (hipError_t e = c->pool.alloc((void**)p, count * sizeof(T)); e != hipSuccess)
    return ics_set_error(ICS_ENOMEM, "device allocation of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
  if (zero) HIPCHK(hipMemsetAsync(*p, 0, count * sizeof(T), c->stream));
  return ICS_OK;
}

// ... or collected in `zl` and zero-filled by ONE launch (flush_zero): a new job's ~24 buffers as 24 memsets cost the host ~35 us each
// (deblur_module creates a job per pyramid level and phase: 8 % of a resident 2048^2 run were the gaps in front of those fills)
struct ZeroList { std::vector<std::pair<void*, size_t>> items; };
template <typename T>
static int dalloc(ics_ctx* c, T** p, size_t count, ZeroList* zl) {
  const int rc = dalloc(c, p, count, false);
  if (rc == ICS_OK) zl->items.emplace_back((void*)*p, count * sizeof(T));
  return rc;
}

// ---- launch helpers with optional event bracketing -----------------------------------------------
struct Prof {
  ics_rl* j; bool on;
  hipStream_t s = nullptr;              // nullptr: the job's stream
  hipStream_t st() const { return s ? s : j->ctx->stream; }
  int grow() {
    if (j->ev_used + 1 > j->ev.size()) {
      for (int i = 0; i < 64; ++i) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); j->ev.push_back(e); }
    }
    return ICS_OK;
  }
  // Consecutive brackets on one stream share an event: the end of one is the begin of the next (an event record between two dependent
  // kernels is a bubble of a few microseconds on the device; 10 per bracketed blind iteration were 2 % of bench.py's timed region).
  // Anything queued outside a bracket breaks the chain: unbracketed launches come through a disabled Prof, other sites call unchain().
  int begin(int cls) {
    if (!on) { j->ev_chain = -1; return ICS_OK; }
    if (j->ev_chain >= 0 && j->ev_chain_stream == st()) j->ev_open = j->ev_chain;
    else {
      RC0(grow());
      HIPCHK(hipEventRecord(j->ev[j->ev_used], st()));
      j->ev_open = (int)j->ev_used++;
    }
    j->ev_open_cls = cls;
    j->ev_chain = -1;
    return ICS_OK;
  }
  int end() {
    if (!on) return ICS_OK;
    RC0(grow());
    HIPCHK(hipEventRecord(j->ev[j->ev_used], st()));
    j->ev_pairs.push_back({j->ev_open, (int)j->ev_used, j->ev_open_cls});
    j->ev_chain = (int)j->ev_used++; j->ev_chain_stream = st();
    j->ev_open = -1;
    return ICS_OK;
  }
  void unchain() { j->ev_chain = -1; }
  // call after a stream synchronisation
  int collect(double* ms, int* launches) {
    if (!on) return ICS_OK;
    size_t done = 0;
    RC0(collect_range(ms, launches, done, j->ev_pairs.size()));
    j->ev_used = 0; j->ev_pairs.clear(); j->ev_chain = -1;
    return ICS_OK;
  }
  // overlapped runs: the pairs [done, upto) are known to be complete; nothing is recycled until the run ends
  int collect_range(double* ms, int* launches, size_t& done, size_t upto) {
    if (!on) return ICS_OK;
    for (size_t i = done; i < upto; ++i) {
      const ics_rl::EvPair& q = j->ev_pairs[i];
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, j->ev[q.b], j->ev[q.e]));
      ms[q.cls] += t; launches[q.cls] += 1;
    }
    done = upto;
    return ICS_OK;
  }
};

// ---- the route of a run or a stage (ics_route.hip resolves it once, ics_run.hip dispatches on it).  Family numbers: those of ics_rl_route
// (include/ics_hip.h)
enum { CONV_MATRIX = 1, CONV_BLOCKS = 2, CONV_PACKED = 3, CONV_SIZED = 4, CONV_TILES = 5, CONV_SMALL = 6 };
enum { GK_FUSED_MATRIX = 1, GK_MATRIX = 2, GK_SPLIT = 3, GK_FP32 = 4, GK_SIZED = 5, GK_TILES = 6, GK_FUSED_TILES = 7, GK_SMALL = 8 };
struct Route {
  bool tiles;           // the FFT-tile pipeline on the planar mirrors (conv family 5)
  bool conv2;           // ... with A1 + A3 as one unit per tile pair (do_conv2)
  bool small;           // the cooperative small-frame iteration, one launch per outer iteration (conv family 6, gradient family 8), with its plan
  IcsSmallPlan plan;
  int conv;             // modes 0 / 1 on the HWC frames: CONV_MATRIX, CONV_BLOCKS, CONV_PACKED or CONV_SIZED
  int gradk;            // the PSF gradient, GK_FUSED_MATRIX ... GK_FUSED_TILES (resolved for non-blind parameters too: the stage API)
  bool image_acc;       // the residual's epilogues read the accumulator-order copy of the image where their tile height has one (ics_image_acc.h)
  bool acc_order;       // ... and a run of these parameters does (ics_rl_route.image_in_accumulator_order)
  bool psf1;            // internal (not in ics_rl_route): blind inner iterations of a tile run step the PSF and build both spectra in one launch (k_psf_spectra)
  bool maxg;            // internal (not in ics_rl_route): mode-2 launches behind an update pass of the run take no operands -- max u from that pass, max |g| from k_maxg_select
  bool overlap;         // the statistics of outer iteration i on the second stream beside iteration i + 1; else a drain at every outer boundary
};

// ---- host functions that cross a unit boundary ---------------------------------------------------------------------------------
// ics_context.hip
hipError_t put_table(ics_ctx* c, float* dev, const std::vector<float>& t);   // a small host table -> device through the pinned staging area, queued
// ics_route.hip (reads the routing switches, makes no HIP call)
bool psf_blocks_only(int K);
bool psf_supported(int K);
int check_params(ics_rl* j, const ics_rl_params* p);
Route resolve_route(const ics_rl* j, const ics_rl_params* p, bool in_run, bool tiles_allowed);
// ics_job.hip: what a job allocates on first use, and the conversions between its HWC frames and their planar mirrors
int pack_weights(ics_rl* j, int do_step, float step, int correlation, hipStream_t s);
int ensure_window(ics_rl* j, const ics_rl_params* p);
int ensure_planar(ics_rl* j);
int ensure_image_acc(ics_rl* j, int RS);
int ensure_tv(ics_rl* j);
int ensure_small(ics_rl* j, const IcsSmallPlan& pl);
int to_planar(ics_rl* j, float* hwc, hipStream_t s);
int from_planar(ics_rl* j, float* hwc, hipStream_t s);
// ics_ops.hip
bool rank1_factors(const double* k, int KH, int KW, std::vector<double>& col, std::vector<double>& row, double tol = 4e-16);

}  // namespace ics_host

// ---- device-side entries of ics_group.hip the job's rank exchange and all-reduces use (not part of include/ics_hip.h) -----------
int ics_group_sendrecv_device(ics_group* g, const float* send, size_t send_count, int send_peer, float* recv, size_t recv_count, int recv_peer);
int ics_group_allreduce_device(ics_group* g, void* buf, size_t count, int kind, hipStream_t stream);
int ics_group_info_local(const ics_group* g);
int ics_group_device(const ics_group* g);
