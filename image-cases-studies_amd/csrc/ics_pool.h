// ics_pool.h -- the block pool of a context (ics_host.h: IcsPool = IcsPoolT over the HIP calls), with its check mode.  Plain C++, no
// HIP header: the bookkeeping is instantiated over malloc / memset / memcpy by tests/host/pool_selfcheck.cpp and run under the
// address and undefined-behaviour sanitizers without a device.
//
// Device memory of a context is recycled, not returned (round 4).  deblur_module creates a job and a handful of images per pyramid
// level and phase (deconvolve.py:204-313); hipMalloc / hipFree cost 0.1 ... 0.7 ms each and hipFree synchronises the device: the
// rocprof timeline of a device-resident 2048^2 run showed 42 % of its 0.19 s idle, most of it in front of the first kernel that
// follows an allocation (profiles/r04_driver_trace_before.txt).  Blocks are rounded up to an eighth of their leading power of two
// (<= 12.5 % slack), a freed block goes to the free list of its rounded size and serves the next request of that size.  Everything a
// context allocates is used on its one stream, so a recycled block needs no synchronisation: the new owner's first operation is
// ordered behind the old owner's last.  The cache is trimmed above `limit` bytes (default: a quarter of the device memory; env
// ICS_POOL_LIMIT_MB / debug switch pool_limit_mb, read when a context is created) and emptied when an allocation fails.
//
// Check mode (debug switch pool_check = a fill byte 0 ... 255; -1, the default, = off: one relaxed load per alloc / release and
// nothing else).  A recycled block holds whatever its last owner left and a request is rounded up by as much as an eighth, so a
// read of memory nobody wrote and a store past the end of a buffer both go unnoticed.  In check mode
//   alloc    takes the caller's size as req = bytes rounded up to 16 (flush_zero writes whole 16-byte words by design), sizes the block
//            for req + RED more bytes, fills ALL of it with the byte (queued before any zero-fill of the caller's) and records req and
//            the byte for the block;
//   release  of a block that has such a record -- whatever the switch says by then -- waits for the device, compares [req, end of
//            block) with the byte, counts a mismatch in pool_overruns and reports it on stderr, zero-fills the block so that the
//            pattern does not outlive the test, and recycles it as usual.
// pool_selftest = 1 makes the next check-mode alloc write one other byte at offset req of its own block (inside the allocation: no
// fault), once: the proof that the red zone is watched.
//
// Dev, the four device calls (each returns 0 or an error code of type Dev::err_t):
//   err_t alloc(void** p, size_t bytes);  void free(void* p);
//   err_t fill(void* p, int byte, size_t bytes);                  queued like the owner's work
//   err_t copy_back(void* host, const void* p, size_t bytes);     after everything queued on the device has finished
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

template <typename Dev>
struct IcsPoolT {
  typedef typename Dev::err_t err_t;
  static constexpr size_t RED = 256;             // least red zone behind a checked block's req bytes
  Dev dev;
  std::mutex mu;
  std::multimap<size_t, void*> free_;            // rounded size -> block
  std::unordered_map<void*, size_t> size_of;     // every block handed out or cached -> rounded size
  struct Rec { size_t req; int byte; };
  std::unordered_map<void*, Rec> rec;            // blocks handed out in check mode
  size_t cached = 0, limit = 0;
  std::atomic<int>*check, *overruns, *selftest;  // the switches (IcsDebug::pool_check, pool_overruns, pool_selftest)
  IcsPoolT(std::atomic<int>* check_, std::atomic<int>* overruns_, std::atomic<int>* selftest_) : check(check_), overruns(overruns_), selftest(selftest_) {}
  static size_t round_up(size_t b) {
    if (b < 65536) b = 65536;
    size_t p2 = 65536;
    while (p2 * 2 <= b) p2 *= 2;                 // leading power of two
    const size_t q = p2 / 8;
    return (b + q - 1) / q * q;
  }
  void trim(size_t keep) {                       // (mu held) largest first
    while (cached > keep && !free_.empty()) {
      auto it = std::prev(free_.end());
      dev.free(it->second); size_of.erase(it->second); cached -= it->first; free_.erase(it);
    }
  }
  err_t alloc(void** p, size_t bytes) {
    const int byte = check->load(std::memory_order_relaxed);
    const bool chk = byte >= 0 && byte <= 255;
    const size_t req = chk ? (bytes + 15) / 16 * 16 : bytes;
    const size_t r = round_up(chk ? req + RED : req);
    std::lock_guard<std::mutex> g(mu);
    auto it = free_.find(r);
    if (it != free_.end()) { *p = it->second; cached -= r; free_.erase(it); }
    else {
      err_t e = dev.alloc(p, r);
      if (e != err_t(0)) { trim(0); e = dev.alloc(p, r); }
      if (e != err_t(0)) { *p = nullptr; return e; }
      size_of[*p] = r;
    }
    if (chk) {
      err_t e = dev.fill(*p, byte, r);
      if (e == err_t(0) && selftest->exchange(0, std::memory_order_relaxed) == 1) e = dev.fill((char*)*p + req, byte ^ 0xFF, 1);
      if (e != err_t(0)) { free_.emplace(r, *p); cached += r; *p = nullptr; return e; }
      rec[*p] = Rec{req, byte};
    }
    return err_t(0);
  }
  void release(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> g(mu);
    auto it = size_of.find(p);
    if (it == size_of.end()) { dev.free(p); return; }   // not ours
    if (!rec.empty()) verify(p, it->second);          // (blocks handed out in check mode, whatever the switch says by now)
    free_.emplace(it->second, p); cached += it->second;
    if (cached > limit) trim(limit / 2);
  }
  void clear() { std::lock_guard<std::mutex> g(mu); trim(0); }

 private:
  void verify(void* p, size_t r) {               // (mu held)
    auto ri = rec.find(p);
    if (ri == rec.end()) return;
    const Rec q = ri->second;
    rec.erase(ri);
    std::vector<unsigned char> red(r - q.req);
    if (dev.copy_back(red.data(), (const char*)p + q.req, red.size()) != err_t(0)) {
      overruns->fetch_add(1, std::memory_order_relaxed);
      fprintf(stderr, "ics pool check: block of %zu bytes (%zu requested): the red zone could not be read back\n", r, q.req);
    } else {
      for (size_t i = 0; i < red.size(); ++i)
        if (red[i] != (unsigned char)q.byte) {
          overruns->fetch_add(1, std::memory_order_relaxed);
          fprintf(stderr, "ics pool check: block of %zu bytes (%zu requested): written past its end, first at offset %zu (0x%02x over fill 0x%02x)\n",
                  r, q.req, q.req + i, (unsigned)red[i], (unsigned)q.byte);
          break;
        }
    }
    (void)dev.fill(p, 0, r);
  }
};
