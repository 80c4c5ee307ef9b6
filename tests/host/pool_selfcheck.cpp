// pool_selfcheck.cpp -- the bookkeeping of the context's block pool (csrc/ics_pool.h) over malloc / memset / memcpy, no device: size
// rounding, the 16-byte rounding of a checked request, the red zone of a request that lands exactly on a size class, the fill of fresh
// and of recycled blocks, a scribble planted by pool_selftest and found, no report for a clean block, the zero-fill on release, trim
// and clear while records are alive.  tests/test_pool_host.py builds it with -fsanitize=address,undefined and runs it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "ics_pool.h"

struct HostDev {
  typedef int err_t;
  std::set<void*> live;                          // what alloc handed out and free has not seen
  size_t fail_next = 0;                          // the next `fail_next` allocations fail
  int fills = 0, copies = 0;
  err_t alloc(void** p, size_t bytes) {
    if (fail_next) { --fail_next; *p = nullptr; return 2; }
    *p = malloc(bytes);
    if (!*p) return 2;
    memset(*p, 0xA5, bytes);                     // a fresh block is not zero
    live.insert(*p);
    return 0;
  }
  void free(void* p) { live.erase(p); ::free(p); }
  err_t fill(void* p, int byte, size_t bytes) { ++fills; memset(p, byte, bytes); return 0; }
  err_t copy_back(void* host, const void* p, size_t bytes) { ++copies; memcpy(host, p, bytes); return 0; }
};
typedef IcsPoolT<HostDev> Pool;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "pool_selfcheck: line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static bool all_bytes(const void* p, size_t from, size_t to, int byte) {
  const unsigned char* q = (const unsigned char*)p;
  for (size_t i = from; i < to; ++i) if (q[i] != (unsigned char)byte) return false;
  return true;
}

int main() {
  std::atomic<int> check(-1), overruns(0), selftest(0);
  {
    Pool pool(&check, &overruns, &selftest);
    pool.limit = (size_t)64 << 20;
    // ---- size rounding: 64 KiB at least, then eighths of the leading power of two (<= 12.5 % slack)
    CHECK(Pool::round_up(0) == 65536 && Pool::round_up(1) == 65536 && Pool::round_up(65536) == 65536);
    CHECK(Pool::round_up(65537) == 65536 + 8192 && Pool::round_up(73728) == 73728 && Pool::round_up(131071) == 131072);
    CHECK(Pool::round_up(131072) == 131072 && Pool::round_up(131073) == 131072 + 16384);
    for (size_t b = 1; b < ((size_t)1 << 33); b = b * 3 + 1) {
      const size_t r = Pool::round_up(b);
      CHECK(r >= b && r % 8192 == 0 && (b < 65536 || (r - b) * 8 <= b));
    }
    // ---- switch off: no fill, no record, no read-back; a freed block serves the next request of its size
    void *a = nullptr, *b = nullptr;
    CHECK(pool.alloc(&a, 1000) == 0 && a && pool.size_of.at(a) == 65536 && pool.rec.empty() && pool.dev.fills == 0);
    CHECK(all_bytes(a, 0, 65536, 0xA5));
    pool.release(a);
    CHECK(pool.cached == 65536 && pool.dev.copies == 0 && pool.dev.fills == 0);
    CHECK(pool.alloc(&b, 65536) == 0 && b == a && pool.cached == 0);
    pool.release(b);
    // ---- check mode: req = bytes rounded up to 16, the block sized for req + RED, all of it filled -- here a RECYCLED block (a's)
    check = 0xFF;
    void* c = nullptr;
    CHECK(pool.alloc(&c, 1001) == 0 && c == a);
    CHECK(pool.rec.at(c).req == 1008 && pool.rec.at(c).byte == 0xFF && pool.size_of.at(c) == 65536);
    CHECK(all_bytes(c, 0, 65536, 0xFF));
    memset(c, 0x11, 1008);                       // the owner writes all of req: legal, the 15 bytes of rounding included
    pool.release(c);
    CHECK(overruns == 0 && pool.rec.empty() && pool.dev.copies == 1);
    CHECK(all_bytes(c, 0, 65536, 0));            // the zero-fill on release: no pattern, no data left
    // ---- a request that lands exactly on a size class gets the next class: its red zone is never empty
    void* d = nullptr;
    check = 0x7F;
    CHECK(pool.alloc(&d, 65536) == 0 && d != c);                 // a FRESH block
    CHECK(pool.size_of.at(d) == 65536 + 8192 && pool.rec.at(d).req == 65536);
    CHECK(pool.size_of.at(d) - pool.rec.at(d).req >= Pool::RED);
    CHECK(all_bytes(d, 0, 65536 + 8192, 0x7F));
    CHECK(pool.alloc(&c, 65536 - Pool::RED) == 0 && pool.size_of.at(c) == 65536);     // the largest request of the 64 KiB class
    CHECK(pool.alloc(&b, 65536 - Pool::RED + 1) == 0 && pool.size_of.at(b) == 65536 + 8192 && pool.rec.at(b).req == 65536 - Pool::RED + 16);
    // ---- a store past the end is found at release, wherever in the slack it lands; the switch may be off by then
    ((unsigned char*)d)[65536 + 8192 - 1] = 0;                    // last byte of the block
    ((unsigned char*)b)[pool.rec.at(b).req] = 0x7E;               // first byte behind req
    check = -1;
    pool.release(d);
    CHECK(overruns == 1);
    pool.release(b);
    CHECK(overruns == 2);
    pool.release(c);
    CHECK(overruns == 2 && pool.rec.empty());
    CHECK(all_bytes(d, 0, 65536 + 8192, 0) && all_bytes(b, 0, 65536 + 8192, 0));
    overruns = 0;
    // ---- pool_selftest: the next check-mode allocation scribbles one byte at offset req of its own block, once
    selftest = 1;
    CHECK(pool.alloc(&a, 500) == 0 && pool.rec.empty() && selftest == 1);          // the switch off: nothing happens, the request stays armed
    pool.release(a);
    check = 0xFE;
    CHECK(pool.alloc(&a, 500) == 0 && selftest == 0 && pool.rec.at(a).req == 512);
    CHECK(all_bytes(a, 0, 512, 0xFE) && ((unsigned char*)a)[512] == (0xFE ^ 0xFF) && all_bytes(a, 513, 65536, 0xFE));
    CHECK(pool.alloc(&b, 500) == 0 && all_bytes(b, 0, 65536, 0xFE));               // ... and the one after it is clean
    pool.release(a);
    CHECK(overruns == 1);
    pool.release(b);
    CHECK(overruns == 1);
    overruns = 0;
    // ---- fill byte 0 is a fill byte, 256 is not
    check = 0;
    CHECK(pool.alloc(&a, 100) == 0 && pool.rec.count(a) == 1 && all_bytes(a, 0, 65536, 0));
    pool.release(a);
    check = 256;
    CHECK(pool.alloc(&a, 100) == 0 && pool.rec.empty());
    pool.release(a);
    // ---- trim and clear while records are alive: only cached blocks go, the records and their blocks stay
    check = 0xFF;
    void* live[3];
    for (int i = 0; i < 3; ++i) CHECK(pool.alloc(&live[i], (size_t)100000 * (i + 1)) == 0);
    CHECK(pool.rec.size() == 3 && pool.cached > 0);
    pool.clear();
    CHECK(pool.cached == 0 && pool.free_.empty() && pool.rec.size() == 3 && pool.size_of.size() == 3 && pool.dev.live.size() == 3);
    for (int i = 0; i < 3; ++i) CHECK(all_bytes(live[i], 0, pool.size_of.at(live[i]), 0xFF));
    pool.limit = 150000;                                           // a release that trims: the largest cached blocks are freed
    pool.release(live[2]);
    CHECK(pool.rec.size() == 2 && pool.cached <= pool.limit && pool.dev.live.size() == 2);
    pool.release(live[1]);
    pool.release(live[0]);
    CHECK(overruns == 0 && pool.rec.empty() && pool.cached <= pool.limit);
    // ---- a failed allocation empties the cache and tries again; a second failure is reported and leaves no record
    pool.limit = (size_t)64 << 20;
    CHECK(pool.alloc(&a, 70000) == 0);
    pool.release(a);
    CHECK(pool.cached > 0);
    pool.dev.fail_next = 1;
    CHECK(pool.alloc(&b, 3000000) == 0 && b && pool.cached == 0);
    pool.dev.fail_next = 2;
    CHECK(pool.alloc(&a, 5000000) != 0 && a == nullptr && pool.rec.size() == 1);
    pool.release(b);
    pool.release(nullptr);
    void* foreign = malloc(64);                                    // not ours: freed, never cached
    pool.dev.live.insert(foreign);
    pool.release(foreign);
    CHECK(pool.dev.live.size() == pool.size_of.size());
    pool.clear();
    CHECK(pool.dev.live.empty() && pool.size_of.empty() && overruns == 0);
  }
  if (failures) { fprintf(stderr, "pool_selfcheck: %d check(s) failed\n", failures); return 1; }
  printf("pool_selfcheck OK\n");
  return 0;
}
