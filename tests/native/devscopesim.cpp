// CPU simulation of the one-shot calls' device-memory owner: bgv_devscope.h's DevScope over a
// recording policy (no HIP here), driven through calls scripted like the library's.  Test
// infrastructure only; it reads a line protocol from stdin (tests/test_devscope_cpu.py writes it)
// and prints, per line, the call's code and the policy calls in order:
//   "rc <code> | a0 a1 ... s f0 f1 ..."   aK: allocation K succeeded, xK: it failed,
//                                          oJ: operation J enqueued, yJ: it failed,
//                                          s: a synchronize, fK: allocation K freed
// The policy's memory is real heap memory, so the sanitizer build also sees a double free, a
// free of a released buffer's neighbour, or a leak.
//
//   call <fail_alloc> <fail_op>   bgv_aggregate_signatures' shape: 7 allocations, 7 operations
//                                 (4 uploads, the launch, 2 downloads), the explicit synchronize.
//                                 Allocation fail_alloc fails (-1: none); operation fail_op fails
//                                 (-1: none; 7: the explicit synchronize itself)
//   release                       cache growth: 3 allocations, a copy, the synchronize, the
//                                 middle buffer handed out (the simulator frees it after the log)
//   commit                        a first allocation that is committed with nothing enqueued
//   idle                          a scope that allocates and enqueues nothing
//   rearm                         a chunk loop: 2 allocations, an operation, the synchronize,
//                                 enqueued(), an operation, one that fails
//   guard <fail>                  bgv_final_verify's shape: no allocation, enqueued(), 2
//                                 operations (the second fails if fail = 1), the synchronize
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <sstream>
#include <string>

#include "../../lodestar_amd/csrc/bgv_devscope.h"

namespace {

std::string g_log;
std::map<void*, int> g_ids;
int g_nalloc = 0, g_fail_alloc = -1, g_fail_sync = 0;

void note(char what, int k = -1) {
  g_log += ' ';
  g_log += what;
  if (k >= 0) g_log += std::to_string(k);
}

struct FakeApi {
  using stream_t = int;
  static bool alloc(void** p, size_t bytes) {
    const int k = g_nalloc++;
    if (k == g_fail_alloc) {
      note('x', k);
      return false;
    }
    *p = malloc(bytes);
    g_ids[*p] = k;
    note('a', k);
    return true;
  }
  static void free(void* p) {
    note('f', g_ids.count(p) ? g_ids[p] : 99);
    ::free(p);
  }
  static bool sync(stream_t) {
    note('s');
    return !g_fail_sync;
  }
};

// an enqueue on the stream, checked as the library checks a HIP call
#define OP(j)                       \
  do {                              \
    if ((j) == fail_op) {           \
      note('y', (j));               \
      return -BGV_E_DEVICE;         \
    }                               \
    note('o', (j));                 \
  } while (0)

int scripted_call(int fail_op) {
  DevScope<FakeApi> sc(1);
  uint8_t *ds, *dout;
  uint32_t *dl, *df, *dc;
  int32_t* dst;
  void* pts;
  const size_t n = 65, naggs = 3;
  if (sc.alloc(&ds, 96 * n + 1) || sc.alloc(&dl, n + 1) || sc.alloc(&dst, n + 1) || sc.alloc(&pts, 288 * n + 1) ||
      sc.alloc(&df, naggs) || sc.alloc(&dc, naggs) || sc.alloc(&dout, 96 * naggs))
    return -BGV_E_DEVICE;
  for (int j = 0; j < 7; ++j) OP(j);
  g_fail_sync = fail_op == 7;
  return sc.sync();
}

int scripted_release(void** kept) {
  const int fail_op = -1;
  DevScope<FakeApi> sc(1);
  uint32_t *a, *b, *c;
  if (sc.alloc(&a, 4) || sc.alloc(&b, 4) || sc.alloc(&c, 4)) return -BGV_E_DEVICE;
  OP(0);
  if (int rc = sc.sync()) return rc;
  *kept = sc.release(b);
  return BGV_OK;
}

int scripted_commit(void** kept) {
  DevScope<FakeApi> sc(1);
  void* p;
  if (int rc = sc.alloc(&p, 64)) return rc;
  *kept = sc.release(p);
  return BGV_OK;
}

int scripted_rearm() {
  const int fail_op = 2;
  DevScope<FakeApi> sc(1);
  uint8_t *a, *b;
  if (sc.alloc(&a, 8) || sc.alloc(&b, 8)) return -BGV_E_DEVICE;
  OP(0);
  if (int rc = sc.sync()) return rc;
  sc.enqueued();
  OP(1);
  OP(2);
  return sc.sync();
}

int scripted_guard(int fail) {
  const int fail_op = fail ? 1 : -1;
  DevScope<FakeApi> sc(1);
  sc.enqueued();
  OP(0);
  OP(1);
  return sc.sync();
}

}  // namespace

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    g_log.clear();
    g_ids.clear();
    g_nalloc = 0;
    g_fail_alloc = -1;
    g_fail_sync = 0;
    int rc = 0;
    void* kept = nullptr;
    if (cmd == "call") {
      int fail_op = -1;
      in >> g_fail_alloc >> fail_op;
      rc = scripted_call(fail_op);
    } else if (cmd == "release") {
      rc = scripted_release(&kept);
    } else if (cmd == "commit") {
      rc = scripted_commit(&kept);
    } else if (cmd == "rearm") {
      rc = scripted_rearm();
    } else if (cmd == "idle") {
      DevScope<FakeApi> sc(1);
    } else if (cmd == "guard") {
      int fail = 0;
      in >> fail;
      rc = scripted_guard(fail);
    } else {
      fprintf(stderr, "devscopesim: bad line: %s", line);
      return 2;
    }
    if (!in) {
      fprintf(stderr, "devscopesim: short line: %s", line);
      return 2;
    }
    printf("rc %d |%s\n", rc, g_log.c_str());
    free(kept);  // the released buffer is the caller's: still valid here, freed once
  }
  return 0;
}
