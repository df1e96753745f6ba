// libblsgpu: C-ABI host orchestration of the MI355X batch BLS verifier.
//
// Mirrors the reference's scheduling semantics:
//   * per-job verdicts and retry   packages/beacon-node/src/chain/bls/multithread/worker.ts:32-108
//   * batch vs single verify       packages/beacon-node/src/chain/bls/maybeBatch.ts:16-39
//   * pubkey aggregation errors    packages/beacon-node/src/chain/bls/utils.ts:5-16
//   * packing jobs into packages   packages/beacon-node/src/chain/bls/multithread/index.ts:290-401
// but lays the sets out for the GPU: one lane per set, device groups of <= 64
// sets (one wavefront) each closed by its own final exponentiation.
//
// Dynamic batching: every bgv_verify / bgv_verify_async call is laid out on the
// calling thread and queued; dispatcher threads (a few per device, one HIP
// stream each) merge all queued calls into one device super-batch, run the
// kernels once over it and hand each call its own verdicts.  This is the GPU
// form of the reference's prepareWork(), which packs queued jobs into one worker
// package: concurrent calls share wavefronts instead of competing for queues.
//
// A job's verdict is the AND of the groups holding its sets.  A failing group
// that mixes batchable jobs sends exactly those jobs to retry rounds run over the
// per-set results already on the device (no set is recomputed).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <unordered_map>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <unordered_set>
#include <thread>
#include <vector>

#include "../../include/blsgpu.h"
#include "bgv_launch.h"
#include "bgv_retry_plan.h"  // with bgv_host_layout.h: the host-only layout and retry planning
#include "bls_field.h"  // fp12_t (sizes of the per-group u copies)
#include "bgv_shuffle.h"  // the committee bounds of an epoch shuffling (bgv_shuffling_put)

// slots merged into one device super-batch (BGV_MAX_BATCH_SLOTS env)
#define BGV_MAX_BATCH_SLOTS 131072
// dispatcher threads (= HIP streams) per device (BGV_DISPATCHERS env)
#define BGV_DISPATCHERS 2

static size_t max_batch_slots() {
  static const size_t v = env_size("BGV_MAX_BATCH_SLOTS", BGV_MAX_BATCH_SLOTS, BGV_WAVE);
  return v;
}
// how long an idle dispatcher waits for more calls to merge (BGV_COALESCE_US env)
#define BGV_COALESCE_US 500
static size_t coalesce_us() {
  static const size_t v = env_size("BGV_COALESCE_US", BGV_COALESCE_US, 0);
  return v;
}
// the window while no super-batch is running: a lone call (block import, a quiet gossip
// moment) then launches almost at once instead of waiting the full window for company
// that is not coming (BGV_IDLE_COALESCE_US env)
#define BGV_IDLE_COALESCE_US 50
static size_t idle_coalesce_us() {
  static const size_t v = env_size("BGV_IDLE_COALESCE_US", BGV_IDLE_COALESCE_US, 0);
  return v;
}
// calls of at least this many sets on a context with several devices are spread over them
// (verify_split; BGV_SPLIT_MIN env, bgv_set_split; 0 disables): a range-sync call ("64 blocks
// ~ 8000 signatures", chain/bls/multithread/index.ts:34) takes every device
#define BGV_SPLIT_MIN_SETS 4096
static size_t split_min_env() {
  static const size_t v = env_size("BGV_SPLIT_MIN", BGV_SPLIT_MIN_SETS, 0);
  return v == 1 ? 2 : v;  // a one-set job is never cut (bgv_set_split)
}
static int dispatchers_per_device() {
  static const int v = (int)env_size("BGV_DISPATCHERS", BGV_DISPATCHERS, 1);
  return v;
}
// Exec buffer sets per device (BGV_EXECS): one per dispatcher plus the ones whose super-batch
// is in its retry rounds
static int execs_per_device() {
  static const int v = (int)env_size("BGV_EXECS", 2 * BGV_DISPATCHERS, 1);
  return std::max(v, dispatchers_per_device());
}

// Retry threads per device (BGV_RETRY_THREADS), each with its own high-priority stream: the
// retry rounds of several super-batches then run side by side instead of queueing behind one
// another (their rounds are latency-bound chains of small launches)
// batches a retry thread holds at once (BGV_RETRY_HOLD): 1, one batch's rounds at a time.
// Holding up to 8 (their rounds side by side, one wait per pass) measured 2.11-2.51 against
// 2.44-2.46 M sets/s, interleaved (profiles/r05/retry_hold/): the steadier one is the default.
static size_t retry_hold_max() {
  static const size_t v = env_size("BGV_RETRY_HOLD", 1, 1);
  return v;
}
static int retry_threads_per_device() {
  static const int v = (int)env_size("BGV_RETRY_THREADS", 1, 1);
  return v;
}

extern "C" int bgv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

namespace {

// Page-locked host staging: copies from it run on the DMA engines, whereas pageable
// copies are staged by blit kernels that queue behind the verify kernels on the CUs.
template <class T>
struct Pinned {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    n = std::max(n, 2 * cap);
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T), 0);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = n;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// One dispatcher's device resources: its stream, events and buffers.
struct Exec {
  // streams lent by the user of the buffers: the dispatcher's stream for a super-batch's first
  // pass, the device's retry stream for its retry rounds (Device::sched)
  hipStream_t main = nullptr;   // per-set kernels and the first pass's closing
  hipStream_t close = nullptr;  // retry rounds (latency-bound): high priority
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_prep = nullptr, ev_sets = nullptr;
  hipEvent_t kev[2 * BGV_NKERNELS] = {};
  void* slot_mem = nullptr;
  uint32_t slot_cap = 0;
  void* group_mem = nullptr;
  uint32_t group_cap = 0;
  bgv_dslot* d_slots = nullptr;
  bgv_dgroup* d_groups = nullptr;
  uint32_t* d_idx = nullptr;
  size_t idx_cap = 0;
  uint8_t* d_pkb = nullptr;
  size_t pkb_cap = 0;
  // host staging of one super-batch
  Pinned<bgv_dslot> h_slots;
  Pinned<bgv_dgroup> h_groups;
  Pinned<uint32_t> h_idx;
  Pinned<uint8_t> h_pkb;
  Pinned<int32_t> h_ss, h_ps, h_verdict;
  fp12_t* d_gu1 = nullptr;  // the first pass's per-group u values, kept for the retry rounds' pattern tests
  size_t gu1_cap = 0;
  void* d_pscratch = nullptr;  // Fp12 products of bgv_verify_partial calls
  size_t pscratch_cap = 0;
  uint8_t* d_pout = nullptr;
  size_t pout_cap = 0;
  uint32_t* d_lines = nullptr;  // the bulk Miller loop's line records (bgv_lines_pairs)
  uint32_t lines_cap = 0;       // pairs
};

// bgv_final_verify's device buffers (under util_mu)
struct FinalScratch {
  uint8_t* din = nullptr;
  void* vals = nullptr;
  void* one = nullptr;
  bgv_dgroup* dg = nullptr;
  int32_t* dst = nullptr;
  int32_t* dv = nullptr;
  size_t cap = 0;
};

// Device-resident committees (bgv_committee_put).  Every device keeps a directory of
// kComHandles entries (bgv_dcommittee: where the members are, how many, their pubkey sum) and one
// pool of member indices; a committee has the same handle and pool range on every device.  The
// host maps the caller's ids to handles: a set is laid out with the HANDLE, and every call holds
// a reference to the committees it names, so a drop (and a put that reuses the id) never changes
// what a call laid out before it reads -- the handle and the pool range return to the free lists
// when the last reference goes, i.e. after those calls have finished.
static const uint32_t kComHandles = 2 * BGV_MAX_COMMITTEES;  // live ones plus dropped ones still referenced
static const size_t kComPoolInit = size_t(1) << 20;          // member indices (4 MB), doubled on demand
struct ComPool {
  std::mutex mu;
  std::vector<uint32_t> free_handles;
  std::map<uint32_t, uint32_t> free_ranges;  // offset -> length, coalesced
  size_t cap = 0;
  bool alloc(uint32_t n, uint32_t* handle, uint32_t* off) {  // under mu
    if (free_handles.empty()) return false;
    for (auto it = free_ranges.begin(); it != free_ranges.end(); ++it)
      if (it->second >= n) {
        *off = it->first;
        const uint32_t rest = it->second - n;
        free_ranges.erase(it);
        if (rest) free_ranges.emplace(*off + n, rest);
        *handle = free_handles.back();
        free_handles.pop_back();
        return true;
      }
    return false;
  }
  // one range of n words and nh handles (an epoch's committees, bgv_shuffling_put: each of its
  // records returns its own part of the range, which add_range joins again)
  bool alloc_bulk(uint32_t n, uint32_t nh, std::vector<uint32_t>* handles, uint32_t* off) {  // under mu
    if (free_handles.size() < nh) return false;
    for (auto it = free_ranges.begin(); it != free_ranges.end(); ++it)
      if (it->second >= n) {
        *off = it->first;
        const uint32_t rest = it->second - n;
        free_ranges.erase(it);
        if (rest) free_ranges.emplace(*off + n, rest);
        handles->assign(free_handles.end() - nh, free_handles.end());
        free_handles.resize(free_handles.size() - nh);
        return true;
      }
    return false;
  }
  void add_range(uint32_t off, uint32_t n) {  // under mu
    auto nx = free_ranges.lower_bound(off);
    if (nx != free_ranges.begin()) {
      auto pv = std::prev(nx);
      if (pv->first + pv->second == off) {
        off = pv->first;
        n += pv->second;
        free_ranges.erase(pv);
      }
    }
    if (nx != free_ranges.end() && off + n == nx->first) {
      n += nx->second;
      free_ranges.erase(nx);
    }
    free_ranges.emplace(off, n);
  }
};
struct CommitteeRec {
  uint32_t handle = 0, off = 0;
  std::vector<uint32_t> idx;  // the members (host mirror: set checks, recomputing after a pubkey overwrite)
  bool bad = false;           // holds a marked key (written under the exclusive cache_mu)
  std::shared_ptr<ComPool> pool;
  ~CommitteeRec() {
    if (!pool) return;
    std::lock_guard<std::mutex> lk(pool->mu);
    pool->free_handles.push_back(handle);
    pool->add_range(off, (uint32_t)idx.size());
  }
};

struct Call;
// What a super-batch's retry rounds need from its first pass.
struct BatchState {
  std::chrono::steady_clock::time_point tb;
  double t_merge = 0, t_tok = 0, t_sets = 0, t_pass1 = 0, t_post = 0;
  uint32_t nslots = 0, ngroups = 0;
  std::vector<uint32_t> call_gb;  // each call's first group in the merged batch
  bool want_gu = false;           // the first pass's u values are in x.d_gu1 (pattern tests)
  bool uniform = false;           // the first pass ran uniform groups (their slots have no own pair f_i)
  bool prof = false;
};
// A super-batch whose first pass is done and whose retry rounds wait for the retry thread.
struct RetryJob {
  std::vector<Call*> calls;
  Exec* x = nullptr;
  std::shared_ptr<BatchState> st;
};
// Exec buffer sets and retry rounds of one device.  A dispatcher takes a free Exec for each
// super-batch and, when its first pass leaves failing groups, hands the batch to the device's
// retry thread and goes on with the next super-batch; the Exec returns to the pool when the
// retry rounds are done.  So the latency-bound retry rounds of one batch overlap the per-set
// kernels of the next ones instead of holding a dispatcher.  Streams: one per dispatcher, one
// (high priority) for the retry rounds, the utility stream: within HIP's default of 4 hardware
// queues per process (GPU_MAX_HW_QUEUES).
struct DevSched {
  std::mutex mu;
  std::condition_variable cv;  // an Exec was released / a retry job was queued / stop
  std::deque<Exec*> free;
  std::deque<RetryJob> rq;
  bool stop = false;
  std::vector<std::thread> retry_threads;
  std::vector<hipStream_t> retries;  // one stream per retry thread
  std::vector<hipStream_t> dstreams;
};

struct Device {
  int id = 0;
  std::unique_ptr<DevSched> sched = std::make_unique<DevSched>();
  FinalScratch final_scratch;
  hipStream_t stream = nullptr;      // utility work (cache upload, hooks, keygen)
  bgv_cache_entry* cache = nullptr;  // pubkey cache (replicated on every device)
  size_t cache_cap = 0;
  bgv_dcommittee* com_dir = nullptr;  // kComHandles entries
  uint32_t* com_pool = nullptr;       // member indices of every committee (ComPool::cap words)
  uint32_t* com_list = nullptr;       // kComHandles words: the handles of one k_committee_total launch
  uint32_t* shuf_buf = nullptr;       // bgv_shuffling_put's scratch (active indices, digest table, pivots)
  size_t shuf_cap = 0;                // in words; grown on demand, under util_mu
  std::vector<Exec*> execs;
  // held while one super-batch runs its per-set kernels (pointer: Device stays movable)
  std::unique_ptr<std::mutex> compute_mu = std::make_unique<std::mutex>();
};

// One bgv_verify call travelling through a dispatcher: its host state (layout, codes, retry
// units: CallPlan, bgv_retry_plan.h) and how its caller hears of the end.
struct Call : CallPlan {
  const bgv_set* sets = nullptr;
  const bgv_pkbits* pkbits = nullptr;                   // per set, or null (bgv_verify_bits)
  std::vector<SetCommittee> setcom;                     // per set once checked (empty without pkbits)
  std::vector<std::shared_ptr<CommitteeRec>> com_refs;  // the committees the layout names
  int32_t* out = nullptr;
  bgv_stats* stats_out = nullptr;
  bgv_done_fn done = nullptr;
  void* user = nullptr;
  bool owned = false;
  std::chrono::steady_clock::time_point t0;
  int dev = -1;  // index in bgv_ctx::devs of the only device whose dispatchers may take it (-1: any)
  bgv_job pjob{};
  int32_t pcode = 0;
  int rc = BGV_OK;
  // completion
  std::mutex mu;
  std::condition_variable cv;
  bool finished = false;
};

}  // namespace

struct bgv_ctx {
  std::vector<Device> devs;
  // cached pubkeys: entries [0, n_pubkeys) are valid on every device.  A pure append writes
  // entries at and past n_pubkeys (which no submitted call reads) and then publishes the new
  // count, so it needs only the shared cache_mu; growth and overwrites take it exclusively.
  std::atomic<size_t> n_pubkeys{0};
  std::mutex put_mu;  // one cache writer at a time (bgv_pubkeys_put, bgv_keygen)
  // indices whose record failed to decode in bgv_pubkeys_put: kept in the count (later runs
  // stay contiguous) but any set naming one rejects with BGV_E_BAD_INDEX.  Written under the
  // exclusive cache_mu, read under the shared one.
  std::unordered_set<uint32_t> bad_pk;
  std::atomic<bool> closed{false};
  std::mutex rng_mu;
  uint64_t rng_seed = 0, rng_state = 0;
  std::shared_mutex cache_mu;  // verify: shared; cache writes: exclusive
  std::mutex util_mu;          // utility streams
  // live committees by id (com_mu: a call's checks read it shared, once per call; puts and drops,
  // serialised by put_mu, write it exclusively).  Lock order: cache_mu, then com_mu.
  std::shared_mutex com_mu;
  std::unordered_map<uint32_t, std::shared_ptr<CommitteeRec>> committees;
  // dropped committees that queued calls may still name (expired entries are pruned at the next
  // drop): a pubkey overwrite recomputes their sums too
  std::vector<std::weak_ptr<CommitteeRec>> retired;
  std::shared_ptr<ComPool> com_pool = std::make_shared<ComPool>();
  std::mutex prof_mu;
  bool profile = false;
  // BGV_FAULT_INJECT=1 at bgv_init: every super-batch fails as a HIP error would (tests of
  // the device-error path: every job in flight rejects with BGV_E_DEVICE, none resolves false)
  bool fault_inject = false;
  // super-batch geometry (bgv_set_batching; env defaults at bgv_init)
  std::atomic<uint32_t> max_slots{BGV_MAX_BATCH_SLOTS};
  std::atomic<uint32_t> coalesce{BGV_COALESCE_US};
  std::atomic<uint32_t> idle_coalesce{BGV_IDLE_COALESCE_US};
  std::atomic<int> running{0};  // super-batches being run by dispatchers
  // calls of at least this many sets are spread over the devices (verify_split; 0: never)
  std::atomic<uint32_t> split_min{BGV_SPLIT_MIN_SETS};
  // split calls not yet done (bgv_close waits for them); split_closing, set by bgv_close under
  // split_mu before it waits, turns later split calls away.  Both under split_mu.
  int split_inflight = 0;
  bool split_closing = false;
  std::mutex split_mu;
  std::condition_variable split_cv;
  double kernel_ms[BGV_NKERNELS] = {};
  uint64_t kernel_launches = 0;
  // dispatch
  std::vector<std::thread> dispatchers;
  std::mutex qmu;
  std::condition_variable qcv;
  std::deque<Call*> queue;
  bool stop = false;
};

#define HIPCHK(x)                               \
  do {                                          \
    hipError_t e_ = (x);                        \
    if (e_ != hipSuccess) return -BGV_E_DEVICE; \
  } while (0)

static uint64_t splitmix64(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// nonzero 64-bit randomizers (blst mul_n_aggregate with 64 random bits)
static void fill_scalars(bgv_ctx* c, uint64_t* out, size_t n) {
  {
    std::lock_guard<std::mutex> lk(c->rng_mu);
    if (c->rng_seed) {
      for (size_t i = 0; i < n; ++i) {
        uint64_t v;
        do v = splitmix64(&c->rng_state);
        while (v == 0);
        out[i] = v;
      }
      return;
    }
  }
  par_ranges(n, [out](size_t lo, size_t hi) {
    size_t got = 0;
    uint8_t* p = reinterpret_cast<uint8_t*>(out + lo);
    while (got < (hi - lo) * 8) {
      const ssize_t r = getrandom(p + got, (hi - lo) * 8 - got, 0);
      if (r > 0) got += (size_t)r;
    }
    for (size_t i = lo; i < hi; ++i)
      if (out[i] == 0) out[i] = 1;
  });
}

template <class T>
static int grow(T** p, size_t* cap, size_t want) {
  if (want <= *cap) return BGV_OK;
  size_t n = std::max(want, *cap * 2);
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)));
  *cap = n;
  return BGV_OK;
}

static int exec_reserve_slots(Exec& x, uint32_t slots) {
  if (slots <= x.slot_cap) return BGV_OK;
  uint32_t n = std::max<uint32_t>(slots, x.slot_cap * 2);
  if (x.slot_mem) (void)hipFree(x.slot_mem);
  if (x.d_slots) (void)hipFree(x.d_slots);
  x.slot_mem = nullptr;
  x.d_slots = nullptr;
  HIPCHK(hipMalloc(&x.slot_mem, bgv_slot_mem_bytes(n)));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&x.d_slots), sizeof(bgv_dslot) * n));
  x.slot_cap = n;
  return BGV_OK;
}

static int exec_reserve_groups(Exec& x, uint32_t groups) {
  if (groups <= x.group_cap) return BGV_OK;
  uint32_t n = std::max<uint32_t>(groups, x.group_cap * 2);
  if (x.group_mem) (void)hipFree(x.group_mem);
  if (x.d_groups) (void)hipFree(x.d_groups);
  x.group_mem = nullptr;
  x.d_groups = nullptr;
  HIPCHK(hipMalloc(&x.group_mem, bgv_group_bytes() * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&x.d_groups), sizeof(bgv_dgroup) * n));
  x.group_cap = n;
  return BGV_OK;
}

// line records for the batch's bulk Miller launch (none on the latency path): allocated on
// first use, in steps of 16,384 pairs (374 MB); kept for the next batch up to the context's
// current super-batch geometry (c->max_slots, which bgv_set_batching may raise above the
// environment's default: trimming against the default would free and reallocate the records --
// each hipFree a device synchronization -- after every first pass), freed after a larger call
// (a 2^20-set job alone needs ~24 GB: exec_trim_lines)
static uint32_t lines_keep_pairs(size_t slots) {
  return (uint32_t)((slots + slots / BGV_WAVE + 16383u) & ~(size_t)16383u);
}
static void exec_trim_lines(Exec& x, size_t max_slots) {
  if (x.lines_cap <= lines_keep_pairs(max_slots)) return;
  (void)hipFree(x.d_lines);
  x.d_lines = nullptr;
  x.lines_cap = 0;
}
static int exec_reserve_lines(Exec& x, bgv_dev_batch& b) {
  const uint32_t need = bgv_lines_pairs(b);
  if (need > x.lines_cap) {
    const uint32_t cap = (need + 16383u) & ~16383u;
    if (x.d_lines) (void)hipFree(x.d_lines);
    x.d_lines = nullptr;
    x.lines_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&x.d_lines), bgv_line_record_bytes() * cap));
    x.lines_cap = cap;
  }
  b.lines = x.d_lines;
  b.lines_cap = x.lines_cap;
  return BGV_OK;
}

static int exec_create(Exec* x) {
  HIPCHK(hipEventCreate(&x->ev0));
  HIPCHK(hipEventCreate(&x->ev1));
  HIPCHK(hipEventCreateWithFlags(&x->ev_sets, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&x->ev_prep, hipEventDisableTiming));
  for (auto& e : x->kev) HIPCHK(hipEventCreate(&e));
  return BGV_OK;
}

static void exec_destroy(Exec* x) {
  if (x->main) (void)hipStreamSynchronize(x->main);
  void* ptrs[] = {x->slot_mem, x->group_mem, x->d_slots,    x->d_groups, x->d_idx,
                  x->d_pkb,      x->d_pscratch, x->d_pout, x->d_lines};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  x->h_slots.release();
  x->h_groups.release();
  x->h_idx.release();
  x->h_pkb.release();
  x->h_ss.release();
  x->h_ps.release();
  x->h_verdict.release();
  if (x->d_gu1) (void)hipFree(x->d_gu1);
  if (x->ev0) (void)hipEventDestroy(x->ev0);
  if (x->ev1) (void)hipEventDestroy(x->ev1);
  if (x->ev_sets) (void)hipEventDestroy(x->ev_sets);
  if (x->ev_prep) (void)hipEventDestroy(x->ev_prep);
  for (auto& e : x->kev)
    if (e) (void)hipEventDestroy(e);
  if (x->close) (void)hipStreamSynchronize(x->close);
  delete x;
}

static void prof_add(bgv_ctx* c, Exec& x, bool sets, bool groups) {
  std::lock_guard<std::mutex> lk(c->prof_mu);
  if (!c->profile) return;
  for (int k = 0; k < BGV_NKERNELS; ++k) {
    const bool is_set_kernel = k < BGV_NSETKERNELS;
    if ((is_set_kernel && !sets) || (!is_set_kernel && !groups)) continue;
    float km = 0;
    if (hipEventElapsedTime(&km, x.kev[2 * k], x.kev[2 * k + 1]) == hipSuccess) c->kernel_ms[k] += km;
  }
  if (sets) c->kernel_launches++;
}

static bgv_dev_batch make_batch(Device& d, Exec& x, uint32_t nslots, uint32_t ngroups) {
  bgv_dev_batch b;
  memset(&b, 0, sizeof(b));
  b.nslots = nslots;
  b.ngroups = ngroups;
  b.slots = x.d_slots;
  b.groups = x.d_groups;
  b.pk_idx = x.d_idx;
  b.cache_opaque = d.cache;
  b.pk_bytes = x.d_pkb;
  b.com_dir = d.com_dir;
  b.com_pool = d.com_pool;
  bgv_carve(&b, x.slot_mem, x.slot_cap, x.group_mem, x.group_cap);
  return b;
}

// ---------------------------------------------------------------------------
// Call lifecycle
// ---------------------------------------------------------------------------
static void call_finish(Call* call) {
  for (size_t j = 0; j < call->njobs; ++j) call->out[j] = call->code[j] == 2 ? -BGV_E_DEVICE : call->code[j];
  call->st.wall_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call->t0).count();
  if (call->stats_out) *call->stats_out = call->st;
  if (call->done) call->done(call->user, call->rc);
  if (call->owned) {
    delete call;
    return;
  }
  {
    std::lock_guard<std::mutex> lk(call->mu);
    call->finished = true;
  }
  call->cv.notify_all();
}

static void call_fail(Call* call, int rc) {
  call->rc = rc;
  for (auto& x : call->code)
    if (x == 2) x = -BGV_E_DEVICE;
  call_finish(call);
}

// The argument checks the reference raises before any crypto, for one job: *code = 2 when the
// job goes to the device, else its verdict (empty job, empty aggregate, an index that is not
// in the cache -- the first such set in set order).  -BGV_E_ARG for a malformed set record.
// The caller holds cache_mu (shared).
// A committee set (pkbits[i].committee != BGV_NO_COMMITTEE) is checked against the live
// committee of its id (committee_set_check); with a call, what the layout needs of it goes to
// call->setcom and the call takes a reference to the committee.  The caller holds com_mu (shared)
// when pkbits is given.
static int host_job_code(bgv_ctx* c, const bgv_job& jb, const bgv_set* sets, int32_t* code,
                         const bgv_pkbits* pkbits = nullptr, Call* call = nullptr) {
  *code = 2;
  if (jb.n_sets == 0) {
    *code = -BGV_E_EMPTY_SET;
    return BGV_OK;
  }
  for (uint32_t k = 0; k < jb.n_sets && *code == 2; ++k) {
    const bgv_set& s = sets[jb.first_set + k];
    if (pkbits && pkbits[jb.first_set + k].committee != BGV_NO_COMMITTEE) {
      const bgv_pkbits& pb = pkbits[jb.first_set + k];
      if (!s.msg || (!s.sig && s.sig_len) || (!pb.bits && pb.n_bits)) return -BGV_E_ARG;
      const auto it = c->committees.find(pb.committee);
      const CommitteeRec* rec = it != c->committees.end() ? it->second.get() : nullptr;
      CommitteeInfo ci{};
      if (rec) ci = CommitteeInfo{rec->handle, (uint32_t)rec->idx.size(), rec->bad};
      SetCommittee sc;
      *code = committee_set_check(rec ? &ci : nullptr, pb, &sc);
      if (*code == 2 && call) {
        call->setcom[jb.first_set + k] = sc;
        if (call->com_refs.empty() || call->com_refs.back().get() != rec) call->com_refs.push_back(it->second);
      }
      continue;
    }
    if (s.n_pk == 0)
      *code = -BGV_E_EMPTY_AGGREGATE;
    else if (!s.msg || (!s.sig && s.sig_len) || (!s.pk_indices && !s.pk_bytes))
      return -BGV_E_ARG;
    else if (s.pk_indices)
      for (uint32_t q = 0; q < s.n_pk; ++q)
        if (s.pk_indices[q] >= c->n_pubkeys || (!c->bad_pk.empty() && c->bad_pk.count(s.pk_indices[q]))) {
          *code = -BGV_E_BAD_INDEX;
          break;
        }
  }
  return BGV_OK;
}

// A freshly allocated layout of a huge call is first touched page by page: 168 MB of slot
// records for a 2^20-set call are ~43,000 page faults.  Transparent huge pages (where the host
// allows them) cut that to ~100.
static void advise_huge(void* p, size_t bytes) {
  const uintptr_t a = ((uintptr_t)p + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
  const uintptr_t e = ((uintptr_t)p + bytes) & ~(uintptr_t)((2u << 20) - 1);
  if (e > a) (void)madvise(reinterpret_cast<void*>(a), e - a, MADV_HUGEPAGE);
}

// host-side checks and layout, on the caller's thread
static int call_submit(bgv_ctx* c, Call* call, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                       int mode, int32_t* out, bgv_stats* stats, bgv_done_fn done, void* user, int dev = -1,
                       const bgv_pkbits* pkbits = nullptr) {
  call->t0 = std::chrono::steady_clock::now();
  call->dev = dev;
  if (c->closed) return -BGV_E_CLOSED;
  if ((njobs && (!jobs || !out)) || (nsets && !sets)) return -BGV_E_ARG;
  if (mode != BGV_MODE_WORKER && mode != BGV_MODE_PER_JOB) return -BGV_E_ARG;
  call->jobs = jobs;
  call->njobs = njobs;
  call->sets = sets;
  call->nsets = nsets;
  call->mode = mode;
  call->out = out;
  call->stats_out = stats;
  call->done = done;
  call->user = user;
  call->code.assign(njobs, 2);
  call->pkbits = pkbits;
  if (pkbits) call->setcom.assign(nsets, SetCommittee{});
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    std::shared_lock<std::shared_mutex> mlk(c->com_mu, std::defer_lock);
    if (pkbits) mlk.lock();
    for (size_t j = 0; j < njobs; ++j) {
      if ((size_t)jobs[j].first_set + jobs[j].n_sets > nsets) return -BGV_E_ARG;
      if (host_job_code(c, jobs[j], sets, &call->code[j], pkbits, call) != BGV_OK) return -BGV_E_ARG;
    }
  }
  const auto is_com = [pkbits](size_t i) { return pkbits && pkbits[i].committee != BGV_NO_COMMITTEE; };
  // pass-1 layout (bgv_host_layout.h)
  Layout& L = call->L;
  {
    size_t npk = 0;
    for (size_t i = 0; i < nsets; ++i)
      if (is_com(i))
        npk += 1 + pkb_nwords(call->setcom[i].n);  // the handle and the bit words (a refused set: n = 0)
      else if (sets[i].pk_indices)
        npk += sets[i].n_pk;
    const size_t cap = nsets + nsets / 8 + BGV_WAVE;  // with room for the groups' padding
    L.slots.reserve(cap);
    L.slot_set.reserve(cap);
    L.idx.reserve(npk);
    if (nsets >= (1u << 17)) {
      advise_huge(L.slots.data(), sizeof(bgv_dslot) * cap);
      advise_huge(L.slot_set.data(), 4 * cap);
      advise_huge(L.idx.data(), 4 * npk);
    }
  }
  layout_call(L, call->todo, jobs, njobs, sets, mode, call->code, pkbits ? call->setcom.data() : nullptr);
  call->set_sig.assign(nsets, 0);
  call->set_pk.assign(nsets, 0);
  if (L.slots.empty()) {  // nothing for the device
    call_finish(call);
    return BGV_OK;
  }
  {
    std::lock_guard<std::mutex> lk(c->qmu);
    if (c->stop) return -BGV_E_CLOSED;
    c->queue.push_back(call);
  }
  if (dev < 0)
    c->qcv.notify_one();
  else
    c->qcv.notify_all();  // only the pinned device's dispatchers may take it
  return BGV_OK;
}

// Run one merged super-batch of calls on one dispatcher's stream.
static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

static bool needs_retry(const std::vector<Call*>& calls) {
  for (const Call* call : calls)
    if (!call->units.empty()) return true;
  return false;
}

// The first pass of one merged super-batch on the dispatcher's stream x.main: layout merge,
// per-set kernels, the groups' closing, verdicts; leaves the retry units in the calls.
static int run_pass1(bgv_ctx* c, Device& d, Exec& x, std::vector<Call*>& calls, BatchState& bs) {
  const auto tb = std::chrono::steady_clock::now();
  bs.tb = tb;
  double t_merge = 0, t_tok = 0, t_sets = 0, t_pass1 = 0, t_post = 0;
  // merge the calls' layouts
  uint32_t nslots = 0, ngroups = 0;
  size_t nidx = 0, npkb = 0, nuniq = 0, ncom_team = 0, ncom_wave = 0;
  bool any_uniform = false;
  for (Call* call : calls) {
    call->slot_base = nslots;
    nslots += (uint32_t)call->L.slots.size();
    ngroups += (uint32_t)call->L.groups.size();
    nidx += call->L.idx.size();
    npkb += call->L.pkb.size();
    nuniq += call->L.uniq.size();
    ncom_team += call->L.com_team.size();
    ncom_wave += call->L.com_wave.size();
    for (char u : call->L.group_uniform) any_uniform = any_uniform || u;
  }
  const size_t ncom = ncom_team + ncom_wave, nlist = nuniq + ncom;  // the lists after the indices
  const bool bulk = nslots + ngroups > bgv_fold_pairs_max();
  // uniform groups (BGV_GROUP_UNIFORM): bulk batches on the two-phase Miller stage
  const bool uniform = uniform_enabled() && any_uniform && bulk && !bgv_single_pass_miller();
  HIPCHK(hipSetDevice(d.id));
  int rc;
  if ((rc = exec_reserve_slots(x, nslots)) || (rc = exec_reserve_groups(x, ngroups)) ||
      (rc = grow(&x.d_idx, &x.idx_cap, std::max<size_t>(nidx + nlist, 1))) ||
      (rc = grow(&x.d_pkb, &x.pkb_cap, std::max<size_t>(npkb, 1))))
    return rc;
  HIPCHK(x.h_slots.reserve(nslots));
  HIPCHK(x.h_groups.reserve(std::max<size_t>(ngroups, 1)));
  HIPCHK(x.h_idx.reserve(nidx + nlist));  // pubkey indices, the hashed slots (b.uniq), the committee slots (b.com)
  HIPCHK(x.h_pkb.reserve(npkb));
  HIPCHK(x.h_ss.reserve(nslots));
  HIPCHK(x.h_ps.reserve(nslots));
  HIPCHK(x.h_verdict.reserve(std::max<size_t>(ngroups, 1)));
  bgv_dslot* slots = x.h_slots.p;
  bgv_dgroup* groups = x.h_groups.p;
  uint32_t max_npk = 0;
  {
    size_t ns = 0, ng = 0, ni = 0, npb = 0;
    for (Call* call : calls) {
      const uint32_t ib = (uint32_t)ni, pb = (uint32_t)(npb / 96), gb = (uint32_t)ng;
      if (ns == 0 && ib == 0 && pb == 0 && gb == 0) {  // the first call: its layout as it is
        const bgv_dslot* src = call->L.slots.data();
        std::atomic<uint32_t> mx{0};
        par_ranges(call->L.slots.size(), [&](size_t lo, size_t hi) {
          memcpy(slots + lo, src + lo, sizeof(bgv_dslot) * (hi - lo));
          uint32_t m = 0;
          for (size_t i = lo; i < hi; ++i)  // a committee slot's n_pk is no run of indices (k_pk_agg_bits sums it)
            if (!(src[i].flags & BGV_SLOT_PK_COMMITTEE)) m = std::max(m, src[i].n_pk);
          uint32_t cur = mx.load();
          while (m > cur && !mx.compare_exchange_weak(cur, m)) {
          }
        });
        max_npk = std::max(max_npk, mx.load());
        ns = call->L.slots.size();
      } else {
        for (const bgv_dslot& s0 : call->L.slots) {
          const bgv_dslot s = rebase_slot(s0, call->slot_base, ib, pb, gb);
          if (!(s.flags & BGV_SLOT_PK_COMMITTEE)) max_npk = std::max(max_npk, s.n_pk);
          slots[ns++] = s;
        }
      }
      for (size_t gi = 0; gi < call->L.groups.size(); ++gi) {
        const bgv_dgroup& g = call->L.groups[gi];
        groups[ng++] = bgv_dgroup{g.first_slot + call->slot_base, g.n_slots, g.mask, 0,
                                  uniform && call->L.group_uniform[gi] ? BGV_GROUP_UNIFORM : 0u};
      }
      if (!call->L.idx.empty()) memcpy(x.h_idx.p + ni, call->L.idx.data(), 4 * call->L.idx.size());
      ni += call->L.idx.size();
      if (!call->L.pkb.empty()) memcpy(x.h_pkb.p + npb, call->L.pkb.data(), call->L.pkb.size());
      npb += call->L.pkb.size();
    }
    uint32_t* u = x.h_idx.p + nidx;
    for (Call* call : calls)
      for (uint32_t v : call->L.uniq) *u++ = v + call->slot_base;
    for (Call* call : calls)
      for (uint32_t v : call->L.com_team) *u++ = v + call->slot_base;
    for (Call* call : calls)
      for (uint32_t v : call->L.com_wave) *u++ = v + call->slot_base;
  }
  std::vector<uint64_t> sc(nslots);
  fill_scalars(c, sc.data(), nslots);
  par_ranges(nslots, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) slots[i].scalar = sc[i];
  });

  bool prof;
  {
    std::lock_guard<std::mutex> lk(c->prof_mu);
    prof = c->profile;
  }
  t_merge = ms_since(tb);
  if (c->fault_inject) HIPCHK(hipErrorLaunchFailure);
  HIPCHK(hipMemcpyAsync(x.d_slots, slots, sizeof(bgv_dslot) * nslots, hipMemcpyHostToDevice, x.main));
  HIPCHK(hipMemcpyAsync(x.d_groups, groups, sizeof(bgv_dgroup) * ngroups, hipMemcpyHostToDevice, x.main));
  if (nidx + nlist) HIPCHK(hipMemcpyAsync(x.d_idx, x.h_idx.p, 4 * (nidx + nlist), hipMemcpyHostToDevice, x.main));
  if (npkb) HIPCHK(hipMemcpyAsync(x.d_pkb, x.h_pkb.p, npkb, hipMemcpyHostToDevice, x.main));
  bgv_dev_batch b = make_batch(d, x, nslots, ngroups);
  b.max_npk = max_npk;
  b.uniform = uniform;
  bs.uniform = uniform;
  b.uniq = x.d_idx + nidx;
  b.nuniq = (uint32_t)nuniq;
  b.com = x.d_idx + nidx + nuniq;
  b.ncom_team = (uint32_t)ncom_team;
  b.ncom_wave = (uint32_t)ncom_wave;
  if (int lrc = exec_reserve_lines(x, b)) return lrc;
  bgv_streams S{x.main, prof ? x.kev : nullptr};
  int32_t *ss = x.h_ss.p, *ps = x.h_ps.p, *verdict = x.h_verdict.p;
  {
    // One super-batch at a time runs k_prep (the token); the token passes on as
    // soon as k_prep is done, so the next batch's k_prep waves queue behind this
    // batch's k_miller and take each SIMD as a Miller wave retires (no drain
    // bubble between batches).  The group closing follows on the same stream.
    const auto tt = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> tok(*d.compute_mu);
    t_tok = ms_since(tt);
    HIPCHK(hipEventRecord(x.ev0, x.main));
    HIPCHK(bgv_launch_prep(b, S));
    HIPCHK(hipEventRecord(x.ev_prep, x.main));
    HIPCHK(bgv_launch_miller(b, S));
    HIPCHK(hipEventRecord(x.ev_sets, x.main));
    HIPCHK(hipEventSynchronize(x.ev_prep));
    t_sets = ms_since(tt) - t_tok;
  }
  const auto tg = std::chrono::steady_clock::now();
  HIPCHK(bgv_launch_groups(b, S, false));
  HIPCHK(hipEventRecord(x.ev1, x.main));
  HIPCHK(hipMemcpyAsync(ss, b.sig_status, 4ull * nslots, hipMemcpyDeviceToHost, x.main));
  HIPCHK(hipMemcpyAsync(ps, b.pk_status, 4ull * nslots, hipMemcpyDeviceToHost, x.main));
  HIPCHK(hipMemcpyAsync(verdict, b.verdict, 4ull * ngroups, hipMemcpyDeviceToHost, x.main));
  HIPCHK(hipStreamSynchronize(x.main));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, x.ev0, x.ev1));
  exec_trim_lines(x, c->max_slots.load());  // the records are dead once the first pass is done
  if (prof) prof_add(c, x, true, true);
  t_pass1 = ms_since(tg);
  const auto tp = std::chrono::steady_clock::now();
  std::vector<uint32_t>& call_gb = bs.call_gb;
  bool& want_gu = bs.want_gu;
  {
    uint32_t gb = 0;
    for (Call* call : calls) {
      call->st.device_ms += ms;
      call->after_pass1(ss + call->slot_base, ps + call->slot_base, verdict + gb);
      call_gb.push_back(gb);
      gb += (uint32_t)call->L.groups.size();
      want_gu = want_gu || call->any_pattern_eligible();
    }
  }
  if (want_gu) {  // the first pass's u values of the groups, before a retry round reuses the array
    if ((rc = grow(&x.d_gu1, &x.gu1_cap, ngroups))) return rc;
    HIPCHK(hipMemcpyAsync(x.d_gu1, b.gu, sizeof(fp12_t) * ngroups, hipMemcpyDeviceToDevice, x.main));
  }
  {
    // bgv_verify_partial calls: the product of the call's groups (before any retry round
    // reuses the per-group arrays), serialized on the device
    uint32_t gb = 0, np = 0, maxg = 0;
    for (Call* call : calls) {
      if (call->partial_out) {
        ++np;
        maxg = std::max<uint32_t>(maxg, (uint32_t)call->L.groups.size());
      }
    }
    if (np) {
      if ((rc = grow(reinterpret_cast<uint8_t**>(&x.d_pscratch), &x.pscratch_cap,
                     bgv_fp12_bytes() * (maxg / 32 + 4))) ||
          (rc = grow(&x.d_pout, &x.pout_cap, 576)))
        return rc;
      for (Call* call : calls) {
        const uint32_t ng = (uint32_t)call->L.groups.size();
        if (call->partial_out) {
          HIPCHK(bgv_launch_partial(b, gb, ng, x.d_pscratch, x.d_pout, x.main));
          HIPCHK(hipMemcpyAsync(call->partial_out, x.d_pout, 576, hipMemcpyDeviceToHost, x.main));
          HIPCHK(hipStreamSynchronize(x.main));
        }
        gb += ng;
      }
    }
  }
  HIPCHK(hipStreamSynchronize(x.main));  // the u copy, before the Exec changes hands
  t_post = ms_since(tp);
  bs.t_merge = t_merge;
  bs.t_tok = t_tok;
  bs.t_sets = t_sets;
  bs.t_pass1 = t_pass1;
  bs.t_post = t_post;
  bs.nslots = nslots;
  bs.ngroups = ngroups;
  bs.prof = prof;
  if (trace_on() && !needs_retry(calls))
    fprintf(stderr,
            "[bgv] dev %d calls %zu slots %u groups %u | submit..dispatch %.1f | merge %.1f tokwait %.1f sets %.1f "
            "groups %.1f post %.1f total %.1f ms\n",
            d.id, calls.size(), nslots, ngroups,
            std::chrono::duration<double, std::milli>(tb - calls.front()->t0).count(), t_merge, t_tok, t_sets,
            t_pass1, t_post, ms_since(tb));
  return BGV_OK;
}

// The retry rounds of a super-batch after run_pass1, on x.close (the device's retry stream),
// over the per-slot results the first pass left in x's buffers.
// One super-batch in its retry rounds on a retry thread (retry_loop): the rounds of every batch
// the thread holds are launched back to back on its stream and waited for together, so a
// round's launch-to-verdict latency is paid once for all of them.
struct RetryRun {
  RetryJob job;
  int rounds = 0;
  uint32_t nrg = 0;  // groups of the round in flight (0: none)
  double t_build = 0;
  std::chrono::steady_clock::time_point tr;
};

// Builds r's next round and enqueues it on its Exec's retry stream (groups up, kernels,
// verdicts down).  *more = false: the batch has no parts left (its rounds are done).
static int retry_launch(Device& d, RetryRun& r, bool* more) {
  Exec& x = *r.job.x;
  std::vector<Call*>& calls = r.job.calls;
  BatchState& bs = *r.job.st;
  const auto th = std::chrono::steady_clock::now();
  std::vector<bgv_dgroup> rg;
  for (size_t k = 0; k < calls.size(); ++k)
    calls[k]->build_parts(rg, bs.want_gu ? (int64_t)bs.call_gb[k] : -1, bs.uniform);
  *more = !rg.empty();
  r.nrg = 0;
  if (rg.empty()) return BGV_OK;
  ++r.rounds;
  const uint32_t nrg = (uint32_t)rg.size();
  // the tests inside uniform first-pass groups (they pair their pubkey sums, bgv_launch_gpairs),
  // listed after the groups in the same upload
  std::vector<uint32_t> upk;
  if (bs.uniform)
    for (uint32_t t = 0; t < nrg; ++t)
      if (rg[t].flags & BGV_GROUP_UNIFORM) upk.push_back(t);
  const uint32_t per = (uint32_t)(sizeof(bgv_dgroup) / sizeof(uint32_t));
  const uint32_t nlist = ((uint32_t)upk.size() + per - 1) / per;  // in bgv_dgroup units
  int rc;
  if ((rc = exec_reserve_groups(x, nrg + nlist))) return rc;
  HIPCHK(x.h_groups.reserve(nrg + nlist));
  HIPCHK(x.h_verdict.reserve(nrg));
  memcpy(x.h_groups.p, rg.data(), sizeof(bgv_dgroup) * nrg);
  if (!upk.empty()) memcpy(x.h_groups.p + nrg, upk.data(), 4 * upk.size());
  HIPCHK(hipMemcpyAsync(x.d_groups, x.h_groups.p, sizeof(bgv_dgroup) * (nrg + nlist), hipMemcpyHostToDevice,
                        x.close));
  bgv_dev_batch b = make_batch(d, x, bs.nslots, nrg);
  b.uniform = !upk.empty();
  b.upk = reinterpret_cast<const uint32_t*>(b.groups + nrg);
  b.npk = (uint32_t)upk.size();
  for (const bgv_dgroup& t : rg) b.weighted = b.weighted || (t.flags & BGV_GROUP_WEIGHTED);
  bool pattern = false;
  for (Call* call : calls) pattern = pattern || !call->punits.empty();
  if (pattern) b.gu1 = x.d_gu1;
  r.t_build = ms_since(th);
  bgv_streams SC{x.close, bs.prof ? x.kev : nullptr};
  HIPCHK(hipEventRecord(x.ev0, x.close));
  HIPCHK(bgv_launch_groups(b, SC, true));
  HIPCHK(hipEventRecord(x.ev1, x.close));
  HIPCHK(hipMemcpyAsync(x.h_verdict.p, b.verdict, 4ull * nrg, hipMemcpyDeviceToHost, x.close));
  r.nrg = nrg;
  return BGV_OK;
}

// After the stream has drained: the round's verdicts into r's calls
static int retry_complete(bgv_ctx* c, RetryRun& r, double t_wait) {
  Exec& x = *r.job.x;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, x.ev0, x.ev1));
  if (r.job.st->prof) prof_add(c, x, false, true);
  if (trace_on()) {
    size_t npt = 0;
    for (Call* call : r.job.calls)
      for (const PatternUnit& pu : call->punits) npt += pu.tests.size();
    fprintf(stderr,
            "[bgv]  round %d: %u groups (%zu tests with a reference), host %.2f, launch..verdicts %.2f, device %.2f ms, "
            "since round start %.1f ms\n",
            r.rounds, r.nrg, npt, r.t_build, t_wait, ms, ms_since(r.tr));
  }
  for (Call* call : r.job.calls) {
    call->st.device_ms += ms;
    call->after_round(x.h_verdict.p);  // part group indices are global to this round
  }
  r.nrg = 0;
  return BGV_OK;
}

static void retry_trace_done(const Device& d, const RetryRun& r) {
  if (!trace_on()) return;
  const BatchState& bs = *r.job.st;
  fprintf(stderr,
          "[bgv] dev %d calls %zu slots %u groups %u | merge %.1f tokwait %.1f sets %.1f groups %.1f post %.1f "
          "retry(%d) %.1f total %.1f ms\n",
          d.id, r.job.calls.size(), bs.nslots, bs.ngroups, bs.t_merge, bs.t_tok, bs.t_sets, bs.t_pass1, bs.t_post,
          r.rounds, ms_since(r.tr), ms_since(bs.tb));
}

static Exec* exec_acquire(Device& d) {
  DevSched& s = *d.sched;
  std::unique_lock<std::mutex> lk(s.mu);
  s.cv.wait(lk, [&s] { return !s.free.empty(); });
  // the most recently released buffer set first: on a quiet device the same warm Exec serves
  // call after call (a huge call's first use of an Exec pins ~170 MB of staging)
  Exec* x = s.free.back();
  s.free.pop_back();
  return x;
}

static void exec_release(Device& d, Exec* x) {
  DevSched& s = *d.sched;
  {
    std::lock_guard<std::mutex> lk(s.mu);
    s.free.push_back(x);
  }
  s.cv.notify_all();
}

static void finish_calls(std::vector<Call*>& calls, int rc) {
  for (Call* call : calls) {
    if (rc != BGV_OK)
      call_fail(call, rc);
    else
      call_finish(call);
  }
}

// The device's retry thread: the retry rounds of handed-over super-batches, in order; drains
// the queue before it stops.
// The retry thread holds up to retry_hold_max() handed-over batches and runs their rounds side by side: each
// pass launches one round of every held batch on the thread's stream, waits once, and applies
// the verdicts; a batch joins at the next pass after its hand-over and leaves (its calls
// finished, its Exec released) when it has no parts left.  Under load, when hand-overs queue up,
// several batches share each launch-to-verdict wait instead of taking turns.
static void retry_loop(bgv_ctx* c, Device* d, int k) {
  DevSched& s = *d->sched;
  (void)hipSetDevice(d->id);
  hipStream_t st = s.retries[k];
  std::vector<RetryRun> held;
  auto leave = [&](size_t i, int rc) {
    finish_calls(held[i].job.calls, rc);
    exec_release(*d, held[i].job.x);
    c->running.fetch_sub(1);
    held.erase(held.begin() + (std::ptrdiff_t)i);
  };
  for (;;) {
    {
      std::unique_lock<std::mutex> lk(s.mu);
      if (held.empty()) s.cv.wait(lk, [&s] { return s.stop || !s.rq.empty(); });
      if (held.empty() && s.rq.empty()) return;  // stopping, and the queue is drained
      while (!s.rq.empty() && held.size() < retry_hold_max()) {
        RetryRun r;
        r.job = std::move(s.rq.front());
        s.rq.pop_front();
        r.job.x->close = st;
        r.tr = std::chrono::steady_clock::now();
        // No cache_mu here: the retry kernels (k_gsum, the group pairs, the closing) read only
        // the per-slot results of pass 1 (r_i sig_i, r_i pk_i, f_i, H, u values), never the
        // pubkey cache, and bgv_close joins this thread before it frees the devices.  A batch in
        // its retry rounds keeps the device busy, so it counts as running for the coalescing
        // window.
        c->running.fetch_add(1);
        held.push_back(std::move(r));
      }
    }
    (void)hipSetDevice(d->id);
    for (size_t i = 0; i < held.size();) {
      bool more = false;
      const int rc = retry_launch(*d, held[i], &more);
      if (rc != BGV_OK) {  // a device error fails this batch's calls; the others go on
        (void)hipStreamSynchronize(st);
        leave(i, rc);
      } else if (!more) {
        retry_trace_done(*d, held[i]);
        leave(i, BGV_OK);
      } else {
        ++i;
      }
    }
    if (held.empty()) continue;
    const auto tl = std::chrono::steady_clock::now();
    const hipError_t e = hipStreamSynchronize(st);
    const double t_wait = ms_since(tl);
    for (size_t i = 0; i < held.size();) {
      const int rc = e == hipSuccess ? retry_complete(c, held[i], t_wait) : -BGV_E_DEVICE;
      if (rc != BGV_OK)
        leave(i, rc);
      else
        ++i;
    }
  }
}

static void dispatcher_loop(bgv_ctx* c, Device* d, hipStream_t stream) {
  (void)hipSetDevice(d->id);
  const int di = (int)(d - c->devs.data());
  // a call pinned to another device (a shard of a split call, verify_split) is not ours
  auto mine = [di](const Call* q) { return q->dev < 0 || q->dev == di; };
  auto any_mine = [c, &mine] {
    for (Call* q : c->queue)
      if (mine(q)) return true;
    return false;
  };
  for (;;) {
    std::vector<Call*> calls;
    {
      std::unique_lock<std::mutex> lk(c->qmu);
      c->qcv.wait(lk, [c, &any_mine] { return c->stop || any_mine(); });
      if (!any_mine()) return;  // stopping, and nothing of ours left to drain
      // Coalescing window: a super-batch costs about the same device time from a
      // few thousand to ~10^5 sets (its closing phases are latency-bound), so give
      // concurrent callers a moment to join before launching.
      auto queued_slots = [c, &mine] {
        size_t n = 0;
        for (Call* q : c->queue)
          if (mine(q)) n += q->L.slots.size();
        return n;
      };
      const size_t cap = c->max_slots.load();
      // a full window only while another super-batch keeps the device busy anyway
      const size_t win = c->running.load() > 0 ? c->coalesce.load()
                                               : std::min<size_t>(c->coalesce.load(), c->idle_coalesce.load());
      const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(win);
      while (!c->stop && queued_slots() < cap &&
             c->qcv.wait_until(lk, until) != std::cv_status::timeout) {
      }
      if (!any_mine()) continue;
      size_t slots = 0;
      for (auto it = c->queue.begin(); it != c->queue.end();) {
        Call* call = *it;
        if (!mine(call)) {
          ++it;
          continue;
        }
        const size_t n = call->L.slots.size();
        if (!calls.empty() && slots + n > cap) break;
        calls.push_back(call);
        slots += n;
        it = c->queue.erase(it);
      }
      if (!c->queue.empty()) c->qcv.notify_all();
    }
    Exec* x = exec_acquire(*d);
    x->main = stream;
    auto bs = std::make_shared<BatchState>();
    int rc;
    {
      std::shared_lock<std::shared_mutex> clk(c->cache_mu);
      c->running.fetch_add(1);
      rc = run_pass1(c, *d, *x, calls, *bs);
      c->running.fetch_sub(1);
    }
    if (rc == BGV_OK && needs_retry(calls)) {
      DevSched& s = *d->sched;
      {
        std::lock_guard<std::mutex> lk(s.mu);
        s.rq.push_back(RetryJob{std::move(calls), x, bs});
      }
      s.cv.notify_all();
      continue;
    }
    finish_calls(calls, rc);
    exec_release(*d, x);
  }
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" {

static void ctx_free_devices(bgv_ctx* c) {
  for (Device& d : c->devs) {
    if (!d.stream) continue;  // never set up (e.g. an index past the device count)
    (void)hipSetDevice(d.id);
    for (Exec* x : d.execs) exec_destroy(x);
    d.execs.clear();
    d.sched->free.clear();
    for (hipStream_t st : d.sched->dstreams) (void)hipStreamDestroy(st);
    d.sched->dstreams.clear();
    for (hipStream_t st : d.sched->retries) (void)hipStreamDestroy(st);
    d.sched->retries.clear();
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    if (d.cache) (void)hipFree(d.cache);
    d.cache = nullptr;
    {
      void* cbufs[] = {d.com_dir, d.com_pool, d.com_list, d.shuf_buf};
      for (void* q : cbufs)
        if (q) (void)hipFree(q);
      d.shuf_buf = nullptr;
      d.shuf_cap = 0;
      d.com_dir = nullptr;
      d.com_pool = nullptr;
      d.com_list = nullptr;
    }
    {
      FinalScratch& fs = d.final_scratch;
      void* bufs[] = {fs.din, fs.vals, fs.one, fs.dg, fs.dst, fs.dv};
      for (void* q : bufs)
        if (q) (void)hipFree(q);
      fs = FinalScratch{};
    }
    if (d.stream) (void)hipStreamDestroy(d.stream);
    d.stream = nullptr;
  }
}

int bgv_init(const int* devices, int ndev, bgv_ctx** out) {
  if (!out) return -BGV_E_ARG;
  *out = nullptr;
  int avail = bgv_device_count();
  if (avail <= 0) return -BGV_E_DEVICE;
  bgv_ctx* c = new bgv_ctx();
  {
    const char* fi = getenv("BGV_FAULT_INJECT");
    c->fault_inject = fi && atoi(fi) > 0;
  }
  c->max_slots = (uint32_t)max_batch_slots();
  c->coalesce = (uint32_t)coalesce_us();
  c->idle_coalesce = (uint32_t)idle_coalesce_us();
  c->split_min = (uint32_t)split_min_env();
  const int n = (devices && ndev > 0) ? ndev : 1;
  c->devs.resize(n);
  for (int i = 0; i < n; ++i) {
    Device& d = c->devs[i];
    d.id = (devices && ndev > 0) ? devices[i] : 0;
    bool ok = d.id >= 0 && d.id < avail && hipSetDevice(d.id) == hipSuccess &&
              hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) == hipSuccess;
    int least = 0, greatest = 0;
    ok = ok && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    // high priority: at normal priority the mainnet-shaped leg measured 2.30-2.73 against
    // 3.21-3.27 M sets/s (profiles/r05/uniform/mainnet_probe_r05g.jsonl)
    for (int k = 0; ok && k < retry_threads_per_device(); ++k) {
      hipStream_t st = nullptr;
      ok = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest) == hipSuccess;
      if (ok) d.sched->retries.push_back(st);
    }
    for (int k = 0; ok && k < dispatchers_per_device(); ++k) {
      hipStream_t st = nullptr;
      ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
      if (ok) d.sched->dstreams.push_back(st);
    }
    // the committee directory and index pool (bgv_committee_put)
    ok = ok && hipMalloc(reinterpret_cast<void**>(&d.com_dir), sizeof(bgv_dcommittee) * kComHandles) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&d.com_pool), 4 * kComPoolInit) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&d.com_list), 4 * (size_t)kComHandles) == hipSuccess;
    for (int k = 0; ok && k < execs_per_device(); ++k) {
      Exec* x = new Exec();
      d.execs.push_back(x);
      ok = exec_create(x) == BGV_OK;
      if (ok) d.sched->free.push_back(x);
    }
    if (!ok) {
      ctx_free_devices(c);
      delete c;
      (void)hipGetLastError();  // no stale error for the launch checks of later calls
      return d.id < 0 || d.id >= avail ? -BGV_E_ARG : -BGV_E_DEVICE;
    }
  }
  c->com_pool->cap = kComPoolInit;
  c->com_pool->free_ranges.emplace(0u, (uint32_t)kComPoolInit);
  for (uint32_t h = kComHandles; h-- > 0;) c->com_pool->free_handles.push_back(h);
  for (Device& d : c->devs) {
    for (hipStream_t st : d.sched->dstreams) c->dispatchers.emplace_back(dispatcher_loop, c, &d, st);
    for (int k = 0; k < (int)d.sched->retries.size(); ++k) d.sched->retry_threads.emplace_back(retry_loop, c, &d, k);
  }
  *out = c;
  return BGV_OK;
}

int bgv_close(bgv_ctx* c) {
  if (!c) return -BGV_E_ARG;
  {
    // asynchronous split calls finish first: their pieces need the dispatchers
    std::unique_lock<std::mutex> lk(c->split_mu);
    c->split_closing = true;
    c->split_cv.wait(lk, [c] { return c->split_inflight == 0; });
  }
  {
    std::lock_guard<std::mutex> lk(c->qmu);
    c->stop = true;
  }
  c->qcv.notify_all();
  for (auto& w : c->dispatchers)
    if (w.joinable()) w.join();
  c->dispatchers.clear();
  // the retry threads finish the super-batches handed to them, then stop
  for (Device& d : c->devs) {
    {
      std::lock_guard<std::mutex> lk(d.sched->mu);
      d.sched->stop = true;
    }
    d.sched->cv.notify_all();
    for (auto& t : d.sched->retry_threads)
      if (t.joinable()) t.join();
    d.sched->retry_threads.clear();
  }
  std::unique_lock<std::shared_mutex> lk(c->cache_mu);
  if (c->closed.exchange(true)) return BGV_OK;
  ctx_free_devices(c);
  return BGV_OK;
}

int bgv_destroy(bgv_ctx* c) {
  if (!c) return -BGV_E_ARG;
  bgv_close(c);
  delete c;
  return BGV_OK;
}

int bgv_set_batching(bgv_ctx* c, uint32_t max_batch_slots, uint32_t coalesce_us, uint32_t idle_coalesce_us) {
  if (!c) return -BGV_E_ARG;
  if (max_batch_slots) c->max_slots = std::max<uint32_t>(max_batch_slots, BGV_WAVE);
  if (coalesce_us != UINT32_MAX) c->coalesce = coalesce_us;
  if (idle_coalesce_us != UINT32_MAX) c->idle_coalesce = idle_coalesce_us;
  return BGV_OK;
}

int bgv_set_rng_seed(bgv_ctx* c, uint64_t seed) {
  if (!c) return -BGV_E_ARG;
  std::lock_guard<std::mutex> lk(c->rng_mu);
  c->rng_seed = seed;
  c->rng_state = seed;
  return BGV_OK;
}

size_t bgv_pubkeys_count(const bgv_ctx* c) { return c ? c->n_pubkeys.load() : 0; }

// grow every device's cache to hold `need` entries (contents preserved); caller holds cache_mu exclusively
static int cache_reserve(bgv_ctx* c, size_t need) {
  const size_t esz = bgv_cache_entry_bytes();
  for (Device& d : c->devs) {
    HIPCHK(hipSetDevice(d.id));
    if (need <= d.cache_cap) continue;
    size_t cap = std::max(need, d.cache_cap * 2);
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, esz * cap));
    if (d.cache) {
      HIPCHK(hipMemcpyAsync(p, d.cache, esz * c->n_pubkeys, hipMemcpyDeviceToDevice, d.stream));
      HIPCHK(hipStreamSynchronize(d.stream));
      HIPCHK(hipFree(d.cache));
    }
    d.cache = static_cast<bgv_cache_entry*>(p);
    d.cache_cap = cap;
  }
  return BGV_OK;
}

// The pubkey sums of the committees in handles, on every device (k_committee_total on the
// utility streams).  The caller holds what keeps the utility streams its own (util_mu, or the
// exclusive cache_mu) and, for committees that are live, the exclusive cache_mu.
static int committee_totals(bgv_ctx* c, const std::vector<uint32_t>& handles) {
  if (handles.empty()) return BGV_OK;
  for (Device& d : c->devs) {
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(hipMemcpyAsync(d.com_list, handles.data(), 4 * handles.size(), hipMemcpyHostToDevice, d.stream));
    HIPCHK(bgv_launch_committee_totals(d.com_dir, d.com_list, (uint32_t)handles.size(), d.com_pool, d.cache, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
  }
  return BGV_OK;
}

// After cache entries [first, first + n) were overwritten: the committees that hold one of them
// -- the live ones, and the dropped ones a queued call still names -- get their sums recomputed
// and their marked-key flag refreshed.  Under the exclusive
// cache_mu (no verify reads a directory entry meanwhile).
static int committees_refresh(bgv_ctx* c, uint32_t first, size_t n) {
  std::vector<uint32_t> handles;
  {
    std::unique_lock<std::shared_mutex> lk(c->com_mu);
    std::vector<std::shared_ptr<CommitteeRec>> recs;
    for (auto& kv : c->committees) recs.push_back(kv.second);
    for (auto& w : c->retired)
      if (auto sp = w.lock()) recs.push_back(std::move(sp));
    for (auto& sp : recs) {
      CommitteeRec& r = *sp;
      bool touched = false, bad = false;
      for (uint32_t i : r.idx) {
        touched = touched || (i >= first && (size_t)i < (size_t)first + n);
        bad = bad || (!c->bad_pk.empty() && c->bad_pk.count(i));
      }
      if (!touched) continue;
      r.bad = bad;
      handles.push_back(r.handle);
    }
  }
  return committee_totals(c, handles);
}

// the devices' index pools grown to hold `need` more words; under the exclusive cache_mu
static int com_pool_grow(bgv_ctx* c, size_t need) {
  ComPool& P = *c->com_pool;
  const size_t old = P.cap, cap = std::max(2 * old, old + need);
  if (cap > (size_t)UINT32_MAX) return -BGV_E_NOMEM;
  for (Device& d : c->devs) {
    HIPCHK(hipSetDevice(d.id));
    uint32_t* p = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), 4 * cap));
    HIPCHK(hipMemcpyAsync(p, d.com_pool, 4 * old, hipMemcpyDeviceToDevice, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    HIPCHK(hipFree(d.com_pool));
    d.com_pool = p;
  }
  std::lock_guard<std::mutex> lk(P.mu);
  P.add_range((uint32_t)old, (uint32_t)(cap - old));
  P.cap = cap;
  return BGV_OK;
}

int bgv_committee_put(bgv_ctx* c, uint32_t id, const uint32_t* indices, size_t n) {
  if (!c || id >= BGV_MAX_COMMITTEES || !indices || n < 1 || n > 65536) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  auto rec = std::make_shared<CommitteeRec>();
  // the checks, then the upload into a handle and a pool range no laid-out call names, and the
  // sum; under the shared cache lock (verifies go on) unless the pool has to grow
  auto checks = [&]() -> int {
    if (c->closed) return -BGV_E_CLOSED;
    {
      std::shared_lock<std::shared_mutex> lk(c->com_mu);
      if (c->committees.count(id)) return -BGV_E_ARG;
    }
    for (size_t i = 0; i < n; ++i)
      if (indices[i] >= c->n_pubkeys || (!c->bad_pk.empty() && c->bad_pk.count(indices[i]))) return -BGV_E_BAD_INDEX;
    return BGV_OK;
  };
  auto take = [&]() -> bool {
    std::lock_guard<std::mutex> lk(c->com_pool->mu);
    if (!c->com_pool->alloc((uint32_t)n, &rec->handle, &rec->off)) return false;
    rec->pool = c->com_pool;  // from here on the record gives both back
    return true;
  };
  auto upload = [&]() -> int {
    rec->idx.assign(indices, indices + n);
    const bgv_dcommittee head{rec->off, (uint32_t)n, {}};
    std::lock_guard<std::mutex> ulk(c->util_mu);
    for (Device& d : c->devs) {
      HIPCHK(hipSetDevice(d.id));
      HIPCHK(hipMemcpyAsync(d.com_pool + rec->off, indices, 4 * n, hipMemcpyHostToDevice, d.stream));
      HIPCHK(hipMemcpyAsync(d.com_dir + rec->handle, &head, sizeof(head), hipMemcpyHostToDevice, d.stream));
      HIPCHK(hipStreamSynchronize(d.stream));  // head is on this stack
    }
    const int rc = committee_totals(c, {rec->handle});
    if (rc) return rc;
    std::unique_lock<std::shared_mutex> lk(c->com_mu);
    c->committees.emplace(id, rec);
    return BGV_OK;
  };
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    if (int rc = checks()) return rc;
    if (take()) return upload();
    std::lock_guard<std::mutex> lk(c->com_pool->mu);
    if (c->com_pool->free_handles.empty()) return -BGV_E_NOMEM;  // every handle is live or still referenced
  }
  std::unique_lock<std::shared_mutex> clk(c->cache_mu);
  if (int rc = checks()) return rc;
  {
    std::lock_guard<std::mutex> ulk(c->util_mu);
    if (int rc = com_pool_grow(c, n)) return rc;
  }
  if (!take()) return -BGV_E_NOMEM;
  return upload();
}

int bgv_committee_drop(bgv_ctx* c, uint32_t id) {
  if (!c) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  if (c->closed) return -BGV_E_CLOSED;
  std::shared_ptr<CommitteeRec> rec;  // released after com_mu: the last reference frees the handle
  std::unique_lock<std::shared_mutex> lk(c->com_mu);
  auto it = c->committees.find(id);
  if (it == c->committees.end()) return -BGV_E_BAD_INDEX;
  rec = std::move(it->second);
  c->committees.erase(it);
  c->retired.erase(std::remove_if(c->retired.begin(), c->retired.end(),
                                  [](const std::weak_ptr<CommitteeRec>& w) { return w.expired(); }),
                   c->retired.end());
  c->retired.push_back(rec);
  return BGV_OK;
}

// An epoch's committees in one call: the device shuffles the active indices straight into one
// range of the index pool (k_shuffle_table, k_shuffle_walk), writes the directory entries of the
// non-empty committees (k_shuffle_dir) and sums them (k_committee_total) -- one launch chain and
// one synchronize per device.  The host mirror of every committee is cut from the shuffling read
// back from the first device.  Locks as bgv_committee_put's.  Nothing is published before
// everything succeeded, and the records give their handles and ranges back otherwise.
int bgv_shuffling_put(bgv_ctx* c, uint32_t first_id, const uint8_t seed[32], const uint32_t* active, size_t n_active,
                      uint32_t slots, uint32_t committees_per_slot, uint32_t rounds, uint32_t* out_shuffling) {
  if (!c || !seed || !active || n_active < 1 || n_active > BGV_SHUFFLE_MAX_N || !slots || !committees_per_slot ||
      rounds > BGV_SHUFFLE_MAX_ROUNDS)
    return -BGV_E_ARG;
  const uint64_t count64 = (uint64_t)slots * committees_per_slot;
  if (first_id > BGV_MAX_COMMITTEES || count64 > BGV_MAX_COMMITTEES - first_id) return -BGV_E_ARG;
  const uint32_t n = (uint32_t)n_active, count = (uint32_t)count64, m = shuf_nonempty(n, count);
  if (shuf_longest(n, count) > 65536) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  std::vector<std::shared_ptr<CommitteeRec>> recs;  // the non-empty committees, in order
  std::vector<uint32_t> ks, handles;                // their numbers in the epoch, their handles
  uint32_t base = 0;
  auto checks = [&]() -> int {
    if (c->closed) return -BGV_E_CLOSED;
    {
      std::shared_lock<std::shared_mutex> lk(c->com_mu);
      for (uint32_t k = 0; k < count; ++k)
        if (c->committees.count(first_id + k)) return -BGV_E_ARG;
    }
    const size_t npk = c->n_pubkeys;
    const bool marks = !c->bad_pk.empty();
    for (size_t i = 0; i < n; ++i)
      if (active[i] >= npk || (marks && c->bad_pk.count(active[i]))) return -BGV_E_BAD_INDEX;
    return BGV_OK;
  };
  auto take = [&]() -> bool {
    std::lock_guard<std::mutex> lk(c->com_pool->mu);
    if (!c->com_pool->alloc_bulk(n, m, &handles, &base)) return false;
    for (uint32_t j = 0; j < m; ++j) {  // from here on the records give everything back
      uint32_t lo, hi;
      ks.push_back(shuf_nonempty_k(n, count, j, &lo, &hi));
      auto rec = std::make_shared<CommitteeRec>();
      rec->handle = handles[j];
      rec->off = base + lo;
      rec->idx.resize(hi - lo);
      rec->pool = c->com_pool;
      recs.push_back(std::move(rec));
    }
    return true;
  };
  auto run = [&]() -> int {
    std::vector<uint32_t> shuf(n);
    {
      std::lock_guard<std::mutex> ulk(c->util_mu);
      const size_t words = bgv_shuffle_scratch_words(n, rounds);
      bool first = true;
      for (Device& d : c->devs) {
        HIPCHK(hipSetDevice(d.id));
        if (d.shuf_cap < words) {
          uint32_t* p = nullptr;
          HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), 4 * words));
          if (d.shuf_buf) (void)hipFree(d.shuf_buf);
          d.shuf_buf = p;
          d.shuf_cap = words;
        }
        HIPCHK(hipMemcpyAsync(d.shuf_buf, active, 4 * (size_t)n, hipMemcpyHostToDevice, d.stream));
        HIPCHK(hipMemcpyAsync(d.com_list, handles.data(), 4 * (size_t)m, hipMemcpyHostToDevice, d.stream));
        HIPCHK(bgv_launch_shuffle(seed, n, rounds, d.shuf_buf, d.com_pool + base, d.stream));
        HIPCHK(bgv_launch_shuffle_dir(d.com_dir, d.com_list, m, base, n, count, d.stream));
        HIPCHK(bgv_launch_committee_totals(d.com_dir, d.com_list, m, d.com_pool, d.cache, d.stream));
        if (first)
          HIPCHK(hipMemcpyAsync(shuf.data(), d.com_pool + base, 4 * (size_t)n, hipMemcpyDeviceToHost, d.stream));
        first = false;
        HIPCHK(hipStreamSynchronize(d.stream));
      }
    }
    for (uint32_t j = 0; j < m; ++j) {
      CommitteeRec& r = *recs[j];
      std::copy_n(shuf.begin() + (r.off - base), r.idx.size(), r.idx.begin());
    }
    if (out_shuffling) memcpy(out_shuffling, shuf.data(), 4 * (size_t)n);
    std::unique_lock<std::shared_mutex> lk(c->com_mu);
    for (uint32_t j = 0; j < m; ++j) c->committees.emplace(first_id + ks[j], recs[j]);
    return BGV_OK;
  };
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    if (int rc = checks()) return rc;
    if (take()) return run();
    std::lock_guard<std::mutex> lk(c->com_pool->mu);
    if (c->com_pool->free_handles.size() < m) return -BGV_E_NOMEM;  // the rest are live or still referenced
  }
  std::unique_lock<std::shared_mutex> clk(c->cache_mu);
  if (int rc = checks()) return rc;
  {
    std::lock_guard<std::mutex> ulk(c->util_mu);
    if (int rc = com_pool_grow(c, n)) return rc;
  }
  if (!take()) return -BGV_E_NOMEM;
  return run();
}

int bgv_committee_drop_range(bgv_ctx* c, uint32_t first_id, uint32_t count) {
  if (!c || first_id > BGV_MAX_COMMITTEES || count > BGV_MAX_COMMITTEES - first_id) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  if (c->closed) return -BGV_E_CLOSED;
  std::vector<std::shared_ptr<CommitteeRec>> recs;  // released after com_mu, as in bgv_committee_drop
  std::unique_lock<std::shared_mutex> lk(c->com_mu);
  c->retired.erase(std::remove_if(c->retired.begin(), c->retired.end(),
                                  [](const std::weak_ptr<CommitteeRec>& w) { return w.expired(); }),
                   c->retired.end());
  for (uint32_t id = first_id; id < first_id + count; ++id) {
    auto it = c->committees.find(id);
    if (it == c->committees.end()) continue;
    c->retired.push_back(it->second);
    recs.push_back(std::move(it->second));
    c->committees.erase(it);
  }
  return (int)recs.size();
}

// Decode n records into per-device staging buffers (the slow part: host-to-device copy and
// one square root per compressed key) under the SHARED cache lock, so running and newly
// submitted verifies are never held up by it; then commit.  A pure append within capacity
// copies the staged entries past n_pubkeys and publishes the new count, still under the shared
// lock; growth, overwrites and undecodable records commit under the exclusive lock (rare: the
// capacity doubles, validator indices only grow).  Records that fail to decode are committed
// as marked indices (sets naming them reject with BGV_E_BAD_INDEX) and the first one's code is
// returned, so one bad key neither leaves a hole that blocks later appends nor reaches a
// verify as a usable key.
int bgv_pubkeys_put(bgv_ctx* c, uint32_t first, const uint8_t* keys, size_t n, int fmt) {
  if (!c || (n && !keys) || (fmt != BGV_PK_COMPRESSED && fmt != BGV_PK_UNCOMPRESSED)) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  const size_t esz = bgv_cache_entry_bytes();
  std::vector<void*> staged(c->devs.size(), nullptr);
  std::vector<int32_t> status(n, 0);
  auto free_staged = [&] {
    for (size_t di = 0; di < staged.size(); ++di)
      if (staged[di]) {
        (void)hipSetDevice(c->devs[di].id);
        (void)hipFree(staged[di]);
      }
  };
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    if (c->closed) return -BGV_E_CLOSED;
    if ((size_t)first > c->n_pubkeys) return -BGV_E_ARG;  // append or overwrite, no holes
    if (n == 0) return BGV_OK;
    std::lock_guard<std::mutex> ulk(c->util_mu);
    for (size_t di = 0; di < c->devs.size(); ++di) {
      Device& d = c->devs[di];
      // zeroed: k_cache_put writes no entry for an undecodable record
      if (hipSetDevice(d.id) != hipSuccess || hipMalloc(&staged[di], esz * n) != hipSuccess ||
          hipMemsetAsync(staged[di], 0, esz * n, d.stream) != hipSuccess) {
        free_staged();
        return -BGV_E_DEVICE;
      }
      const size_t chunk = 1 << 20;
      uint8_t* dk = nullptr;
      int32_t* dst = nullptr;
      int rc = BGV_OK;
      if (hipMalloc(reinterpret_cast<void**>(&dk), (size_t)fmt * std::min(n, chunk) + 1) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&dst), 4 * std::min(n, chunk) + 4) != hipSuccess)
        rc = -BGV_E_DEVICE;
      for (size_t off = 0; rc == BGV_OK && off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        bgv_cache_entry* out =
            reinterpret_cast<bgv_cache_entry*>(static_cast<uint8_t*>(staged[di]) + esz * off);
        if (hipMemcpyAsync(dk, keys + (size_t)fmt * off, (size_t)fmt * m, hipMemcpyHostToDevice, d.stream) !=
                hipSuccess ||
            bgv_launch_cache_put(dk, (uint32_t)m, fmt, out, dst, d.stream) != hipSuccess ||
            (di == 0 && hipMemcpyAsync(status.data() + off, dst, 4 * m, hipMemcpyDeviceToHost, d.stream) !=
                            hipSuccess) ||
            hipStreamSynchronize(d.stream) != hipSuccess)
          rc = -BGV_E_DEVICE;
      }
      if (dk) (void)hipFree(dk);
      if (dst) (void)hipFree(dst);
      if (rc) {
        free_staged();
        return rc;
      }
    }
  }
  int first_err = BGV_OK;
  std::vector<uint32_t> bad;
  for (size_t i = 0; i < n; ++i)
    if (status[i]) {
      if (first_err == BGV_OK) first_err = status[i];
      bad.push_back(first + (uint32_t)i);
    }
  const size_t need = (size_t)first + n;
  auto copy_in = [&]() -> int {
    for (size_t di = 0; di < c->devs.size(); ++di) {
      Device& d = c->devs[di];
      HIPCHK(hipSetDevice(d.id));
      HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(d.cache) + esz * first, staged[di], esz * n,
                            hipMemcpyDeviceToDevice, d.stream));
      HIPCHK(hipStreamSynchronize(d.stream));
    }
    return BGV_OK;
  };
  int rc = BGV_OK;
  bool done = false;
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    if (c->closed) {
      rc = -BGV_E_CLOSED;
      done = true;
    } else if (first == c->n_pubkeys && bad.empty()) {
      bool fits = true;
      for (const Device& d : c->devs) fits = fits && need <= d.cache_cap;
      if (fits) {
        std::lock_guard<std::mutex> ulk(c->util_mu);
        rc = copy_in();
        if (rc == BGV_OK) c->n_pubkeys.store(need);
        done = true;
      }
    }
  }
  if (!done) {
    std::unique_lock<std::shared_mutex> clk(c->cache_mu);
    if (c->closed) {
      rc = -BGV_E_CLOSED;
    } else {
      std::lock_guard<std::mutex> ulk(c->util_mu);
      rc = cache_reserve(c, need);
      // an undecodable record that overwrites an existing entry keeps the old entry: a call
      // that passed its index check before this put may still read it (later calls reject
      // the index with BGV_E_BAD_INDEX)
      const uint32_t old_n = (uint32_t)c->n_pubkeys.load();
      for (size_t di = 0; rc == BGV_OK && di < c->devs.size(); ++di) {
        Device& d = c->devs[di];
        if (hipSetDevice(d.id) != hipSuccess) rc = -BGV_E_DEVICE;
        for (uint32_t i : bad)
          if (rc == BGV_OK && i < old_n &&
              hipMemcpyAsync(static_cast<uint8_t*>(staged[di]) + esz * (i - first),
                             reinterpret_cast<const uint8_t*>(d.cache) + esz * i, esz, hipMemcpyDeviceToDevice,
                             d.stream) != hipSuccess)
            rc = -BGV_E_DEVICE;
      }
      if (rc == BGV_OK) rc = copy_in();
      if (rc == BGV_OK) {
        for (uint32_t i = first; i < need; ++i) c->bad_pk.erase(i);  // overwritten entries
        for (uint32_t i : bad) c->bad_pk.insert(i);
        c->n_pubkeys.store(std::max(c->n_pubkeys.load(), need));
        if (first < old_n) rc = committees_refresh(c, first, n);  // live committees over these keys
      }
    }
  }
  free_staged();
  if (rc) return rc;
  return first_err ? -first_err : BGV_OK;
}

// ---------------------------------------------------------------------------
// One call over several devices (a context on a device list; SURVEY 8(e) inside the library).
// The reference splits a big call into >= 128-set jobs for its workers
// (chain/bls/multithread/index.ts:153-166; range sync hands ~8000 sets at once, :34); here a
// call of at least split_min sets is spread over the context's devices:
//   * a job of at least split_min sets is cut into one contiguous run of sets per device; each
//     run's Miller-loop product (576 B, bgv_verify_partial's) is computed on its device, the
//     partials are combined with ONE final exponentiation (bgv_final_verify on the first
//     device), and the job's code follows the reference's precedence: the first undecodable
//     signature in set order, then the pubkey condition, then the verdict;
//   * the other jobs go to the devices in contiguous runs balanced by set count, each run one
//     call pinned to its device (retry rounds stay on the device that ran the first pass).
// Codes are those of the same call on one device (tests/test_gpu_r04.py).
// ---------------------------------------------------------------------------
static void fp12_one_bytes(uint8_t out[576]) {
  memset(out, 0, 576);
  out[47] = 1;  // c0.c0.c0 = 1, big-endian
}

// One job's sets -> its Fp12 Miller-loop product and status codes on device dev (-1: any).
static int partial_submit(bgv_ctx* c, Call* call, const bgv_set* sets, size_t nsets, uint8_t* out576,
                          int32_t* out_codes, int dev, const bgv_pkbits* pkbits = nullptr) {
  out_codes[0] = out_codes[1] = 0;
  fp12_one_bytes(out576);
  call->partial_out = out576;
  call->partial_codes = out_codes;
  call->pjob = bgv_job{0, (uint32_t)nsets, 0};
  return call_submit(c, call, &call->pjob, 1, sets, nsets, BGV_MODE_PER_JOB, &call->pcode, nullptr, nullptr, nullptr,
                     dev, pkbits);
}

static int call_wait(Call* call) {
  std::unique_lock<std::mutex> lk(call->mu);
  call->cv.wait(lk, [call] { return call->finished; });
  return call->rc;
}

static int partial_finish(Call* call, int rc, int32_t* out_codes) {
  if (rc == BGV_OK) rc = call_wait(call);
  if (rc == BGV_OK && call->pcode < 0 && call->pcode != -BGV_E_DEVICE) out_codes[0] = call->pcode;  // host-side
  return rc;
}

static size_t split_min_sets(const bgv_ctx* c) {
  return c->split_min.load();
}

static void stats_add(bgv_stats* a, const bgv_stats& b) {
  a->batch_retries += b.batch_retries;
  a->batch_sigs_success += b.batch_sigs_success;
  a->device_groups += b.device_groups;
  a->sets_verified += b.sets_verified;
  a->device_ms = std::max(a->device_ms, b.device_ms);
}

static bool split_wanted(const bgv_ctx* c, size_t nsets) {
  return c->devs.size() > 1 && split_min_sets(c) > 0 && nsets >= split_min_sets(c);
}

// A split call registers itself before it submits anything (false: the context is closing)
// and deregisters when it no longer touches the context; bgv_close waits for the count to
// drop to zero.  The notify happens under split_mu, so a woken bgv_close (and the
// bgv_destroy after it) cannot free the context before split_leave has returned.
static bool split_enter(bgv_ctx* c) {
  std::lock_guard<std::mutex> lk(c->split_mu);
  if (c->split_closing) return false;
  ++c->split_inflight;
  return true;
}

static void split_leave(bgv_ctx* c) {
  std::lock_guard<std::mutex> lk(c->split_mu);
  --c->split_inflight;
  c->split_cv.notify_all();
}

static int verify_split(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                        const bgv_pkbits* pkbits, int mode, int32_t* out, bgv_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t K = c->devs.size(), big = split_min_sets(c);
  struct Shard {  // one run of a big job on one device
    Call call;
    size_t job;
    uint8_t part[576];
    int32_t codes[2] = {0, 0};
    int rc = BGV_OK;
  };
  struct Child {  // small jobs [j0, j1) pinned to one device
    Call call;
    std::vector<bgv_job> jobs;
    std::vector<int32_t> out;
    bgv_stats st{};
    size_t j0 = 0;
    int rc = BGV_OK;
  };
  std::vector<std::unique_ptr<Shard>> shards;
  std::vector<std::unique_ptr<Child>> kids;
  std::vector<size_t> small;
  size_t small_sets = 0;
  // a big job's host-side checks run on the whole job before it is cut, so they take
  // precedence over every shard's device statuses, as in the unsplit call (job_precheck)
  std::vector<int32_t> pre(njobs, 2);
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    std::shared_lock<std::shared_mutex> mlk(c->com_mu, std::defer_lock);
    if (pkbits) mlk.lock();
    for (size_t j = 0; j < njobs; ++j) {
      if ((size_t)jobs[j].first_set + jobs[j].n_sets > nsets) return -BGV_E_ARG;
      if (jobs[j].n_sets >= big && host_job_code(c, jobs[j], sets, &pre[j], pkbits) != BGV_OK) return -BGV_E_ARG;
    }
  }
  for (size_t j = 0; j < njobs; ++j) {
    if (jobs[j].n_sets >= big) continue;
    small.push_back(j);
    small_sets += jobs[j].n_sets;
  }
  int rc = BGV_OK;
  // small jobs: contiguous runs of the call's job order, about small_sets / K sets each
  {
    size_t i = 0, acc = 0;
    for (size_t d = 0; d < K && i < small.size(); ++d) {
      const size_t target = (small_sets * (d + 1) + K - 1) / K;
      auto kid = std::make_unique<Child>();
      kid->j0 = i;
      while (i < small.size() && (acc < target || kid->jobs.empty())) {
        kid->jobs.push_back(jobs[small[i]]);
        acc += jobs[small[i]].n_sets;
        ++i;
      }
      if (d == K - 1)
        while (i < small.size()) {
          kid->jobs.push_back(jobs[small[i]]);
          ++i;
        }
      kid->out.assign(kid->jobs.size(), 0);
      kid->rc = call_submit(c, &kid->call, kid->jobs.data(), kid->jobs.size(), sets, nsets, mode, kid->out.data(),
                            &kid->st, nullptr, nullptr, (int)d, pkbits);
      if (kid->rc != BGV_OK && rc == BGV_OK) rc = kid->rc;
      kids.push_back(std::move(kid));
    }
  }
  // big jobs: one run of sets per device
  for (size_t j = 0; j < njobs; ++j) {
    const uint32_t n = jobs[j].n_sets;
    if (n < big || pre[j] != 2) continue;
    for (size_t d = 0; d < K; ++d) {
      const size_t lo = n * d / K, hi = n * (d + 1) / K;
      if (hi <= lo) continue;
      auto sh = std::make_unique<Shard>();
      sh->job = j;
      sh->rc = partial_submit(c, &sh->call, sets + jobs[j].first_set + lo, hi - lo, sh->part, sh->codes, (int)d,
                              pkbits ? pkbits + jobs[j].first_set + lo : nullptr);
      if (sh->rc != BGV_OK && rc == BGV_OK) rc = sh->rc;
      shards.push_back(std::move(sh));
    }
  }
  // every submitted piece completes before its memory goes away
  for (auto& k : kids)
    if (k->rc == BGV_OK) {
      k->rc = call_wait(&k->call);
      if (k->rc != BGV_OK && rc == BGV_OK) rc = k->rc;
    }
  for (auto& sh : shards)
    if (sh->rc == BGV_OK) {
      sh->rc = partial_finish(&sh->call, BGV_OK, sh->codes);
      if (sh->rc != BGV_OK && rc == BGV_OK) rc = sh->rc;
    }
  if (rc != BGV_OK) return rc;
  bgv_stats st{};
  for (auto& k : kids) {
    for (size_t q = 0; q < k->jobs.size(); ++q) out[small[k->j0 + q]] = k->out[q];
    stats_add(&st, k->st);
  }
  for (size_t j = 0; j < njobs; ++j) {
    if (jobs[j].n_sets < big) continue;
    if (pre[j] != 2) {
      out[j] = pre[j];
      continue;
    }
    int32_t code = 0;
    bool decided = false;
    std::vector<uint8_t> parts;
    for (auto& sh : shards)
      if (sh->job == j && sh->codes[0] && !decided) {  // first undecodable signature in set order
        code = sh->codes[0];
        decided = true;
      }
    for (auto& sh : shards)
      if (sh->job == j && sh->codes[1] && !decided) {  // then the first pubkey condition
        code = sh->codes[1] == 1 ? -BGV_BLST_PK_IS_INFINITY : sh->codes[1];
        decided = true;
      }
    if (!decided) {
      for (auto& sh : shards)
        if (sh->job == j) parts.insert(parts.end(), sh->part, sh->part + 576);
      int32_t v = 0;
      const int frc = bgv_final_verify(c, parts.data(), parts.size() / 576, &v);
      if (frc != BGV_OK) return frc;
      code = v ? 1 : 0;
    }
    out[j] = code;
    st.sets_verified += jobs[j].n_sets;
    st.device_groups += 1;
  }
  st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (stats) *stats = st;
  return BGV_OK;
}

int bgv_set_split(bgv_ctx* c, uint32_t min_sets) {
  if (!c) return -BGV_E_ARG;
  // at least 2: a one-set job is never cut (its infinity-key verdict is false, not
  // BLST_PK_IS_INFINITY, which a shard's codes cannot tell apart)
  c->split_min = min_sets == 1 ? 2 : min_sets;
  return BGV_OK;
}

int bgv_verify(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, int mode,
               int32_t* out, bgv_stats* stats) {
  return bgv_verify_bits(c, jobs, njobs, sets, nsets, nullptr, mode, out, stats);
}

int bgv_verify_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, int mode,
                     int32_t* out, bgv_stats* stats, bgv_done_fn done, void* user) {
  return bgv_verify_bits_async(c, jobs, njobs, sets, nsets, nullptr, mode, out, stats, done, user);
}

int bgv_verify_bits(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                    const bgv_pkbits* pkbits, int mode, int32_t* out, bgv_stats* stats) {
  if (!c) return -BGV_E_ARG;
  if (split_wanted(c, nsets)) {
    if (c->closed) return -BGV_E_CLOSED;
    if ((njobs && (!jobs || !out)) || (nsets && !sets)) return -BGV_E_ARG;
    if (mode != BGV_MODE_WORKER && mode != BGV_MODE_PER_JOB) return -BGV_E_ARG;
    if (!split_enter(c)) return -BGV_E_CLOSED;
    const int rc = verify_split(c, jobs, njobs, sets, nsets, pkbits, mode, out, stats);
    split_leave(c);
    return rc;
  }
  Call* call = new Call();
  int rc = call_submit(c, call, jobs, njobs, sets, nsets, mode, out, stats, nullptr, nullptr, -1, pkbits);
  if (rc == BGV_OK) {
    std::unique_lock<std::mutex> lk(call->mu);
    call->cv.wait(lk, [call] { return call->finished; });
    rc = call->rc;
  }
  delete call;
  return rc;
}

int bgv_verify_bits_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                          const bgv_pkbits* pkbits, int mode, int32_t* out, bgv_stats* stats, bgv_done_fn done,
                          void* user) {
  if (!c) return -BGV_E_ARG;
  if (split_wanted(c, nsets)) {
    // a split call waits for its pieces and combines them: on a thread of its own (big calls
    // only), then done() as for any call
    if (c->closed) return -BGV_E_CLOSED;
    if ((njobs && (!jobs || !out)) || (nsets && !sets)) return -BGV_E_ARG;
    if (mode != BGV_MODE_WORKER && mode != BGV_MODE_PER_JOB) return -BGV_E_ARG;
    if (!split_enter(c)) return -BGV_E_CLOSED;
    std::thread([=] {
      const int rc = verify_split(c, jobs, njobs, sets, nsets, pkbits, mode, out, stats);
      if (done) done(user, rc);
      split_leave(c);
    }).detach();
    return BGV_OK;
  }
  Call* call = new Call();
  call->owned = true;  // deleted by the dispatcher after done()
  int rc = call_submit(c, call, jobs, njobs, sets, nsets, mode, out, stats, done, user, -1, pkbits);
  if (rc != BGV_OK) delete call;
  return rc;
}

int bgv_verify_partial(bgv_ctx* c, const bgv_set* sets, size_t nsets, uint8_t out576[576], int32_t out_codes[2]) {
  if (!c || !out576 || !out_codes || (nsets && !sets)) return -BGV_E_ARG;
  out_codes[0] = out_codes[1] = 0;
  fp12_one_bytes(out576);
  if (nsets == 0) return c->closed ? -BGV_E_CLOSED : BGV_OK;  // an empty shard: the identity
  Call* call = new Call();
  const int rc = partial_finish(call, partial_submit(c, call, sets, nsets, out576, out_codes, -1), out_codes);
  delete call;
  return rc;
}

int bgv_final_verify(bgv_ctx* c, const uint8_t* partials, size_t n, int32_t* out_verdict) {
  if (!c || !out_verdict || (n && !partials) || n > (1u << 20)) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  const size_t m = std::max<size_t>(n, 1);
  std::vector<uint8_t> in(576 * m);
  if (n) memcpy(in.data(), partials, 576 * n);
  else fp12_one_bytes(in.data());
  // persistent buffers, grown to the largest n seen (a hipFree would synchronize the device
  // against the super-batches running on it)
  FinalScratch& fs = d.final_scratch;
  if (m > fs.cap) {
    void* bufs[] = {fs.din, fs.vals, fs.one, fs.dg, fs.dst, fs.dv};
    for (void* q : bufs)
      if (q) (void)hipFree(q);
    fs = FinalScratch{};
    const size_t cap = std::max<size_t>(m, 8);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&fs.din), 576 * cap));
    HIPCHK(hipMalloc(&fs.vals, bgv_fp12_bytes() * cap));
    HIPCHK(hipMalloc(&fs.one, bgv_fp12_bytes()));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&fs.dg), sizeof(bgv_dgroup)));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&fs.dst), 4 * cap));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&fs.dv), 4));
    fs.cap = cap;
  }
  const bgv_dgroup g{0, (uint32_t)m, BGV_ALL_SLOTS};
  HIPCHK(hipMemcpyAsync(fs.din, in.data(), 576 * m, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(fs.dg, &g, sizeof(g), hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_final_verify(fs.din, (uint32_t)m, fs.vals, fs.one, fs.dg, fs.dst, fs.dv, d.stream));
  std::vector<int32_t> st(m);
  int32_t v = 0;
  HIPCHK(hipMemcpyAsync(st.data(), fs.dst, 4 * m, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(&v, fs.dv, 4, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  for (int32_t x : st)
    if (x) return -BGV_E_ARG;  // a coefficient >= p: not a serialized partial
  *out_verdict = v;
  return BGV_OK;
}

int bgv_debug_prepare(bgv_ctx* c, const bgv_set* sets, size_t nsets, int path, uint64_t seed, uint8_t* out_h192,
                      uint8_t* out_f576, int32_t* out_status) {
  if (!c || (nsets && (!sets || !out_h192 || !out_f576 || !out_status)) ||
      (path != BGV_PATH_BULK && path != BGV_PATH_LATENCY))
    return -BGV_E_ARG;
  if (nsets == 0) return BGV_OK;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  // one job's layout: groups of 64 consecutive slots, every slot hashes its own root
  std::vector<bgv_dslot> slots;
  std::vector<bgv_dgroup> groups;
  std::vector<uint32_t> idx;
  uint64_t state = seed;
  uint32_t max_npk = 0;
  for (size_t i = 0; i < nsets; ++i) {
    const bgv_set& st = sets[i];
    if (!st.pk_indices || st.n_pk == 0 || !st.msg || (st.sig_len && !st.sig)) return -BGV_E_ARG;
    for (uint32_t q = 0; q < st.n_pk; ++q)
      if (st.pk_indices[q] >= c->n_pubkeys || c->bad_pk.count(st.pk_indices[q])) return -BGV_E_BAD_INDEX;
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.flags = BGV_SLOT_PK_CACHED;
    s.n_pk = st.n_pk;
    s.sig_len = st.sig_len;
    s.pk_off = (uint32_t)idx.size();
    idx.insert(idx.end(), st.pk_indices, st.pk_indices + st.n_pk);
    memcpy(s.msg, st.msg, 32);
    if (st.sig_len == 96) memcpy(s.sig, st.sig, 96);
    s.group = (uint32_t)(i / BGV_WAVE);
    s.hsrc = (uint32_t)i;
    do s.scalar = splitmix64(&state);
    while (s.scalar == 0);
    max_npk = std::max(max_npk, st.n_pk);
    slots.push_back(s);
  }
  while (slots.size() % BGV_WAVE) {
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.flags = BGV_SLOT_PAD;
    s.hsrc = (uint32_t)slots.size();
    slots.push_back(s);
  }
  for (size_t g = 0; g * BGV_WAVE < nsets; ++g)
    groups.push_back(bgv_dgroup{(uint32_t)(g * BGV_WAVE), (uint32_t)std::min<size_t>(BGV_WAVE, nsets - g * BGV_WAVE),
                                BGV_ALL_SLOTS});
  const uint32_t nslots = (uint32_t)slots.size(), ngroups = (uint32_t)groups.size();
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  Exec* x = new Exec();
  uint8_t *dh = nullptr, *df = nullptr;
  int rc = exec_create(x);
  // a non-blocking stream of its own, like the dispatchers' (not the legacy null stream)
  hipStream_t dstream = nullptr;
  if (!rc && hipStreamCreateWithFlags(&dstream, hipStreamNonBlocking) != hipSuccess) rc = -BGV_E_DEVICE;
  x->main = dstream;
  if (!rc) rc = exec_reserve_slots(*x, nslots);
  if (!rc) rc = exec_reserve_groups(*x, ngroups);
  if (!rc) rc = grow(&x->d_idx, &x->idx_cap, idx.size());
  if (!rc && (hipMalloc(reinterpret_cast<void**>(&dh), 192ull * nslots) != hipSuccess ||
              hipMalloc(reinterpret_cast<void**>(&df), 576ull * nslots) != hipSuccess))
    rc = -BGV_E_DEVICE;
  std::vector<int32_t> ss(nslots), ps(nslots);
  if (!rc) {
    bgv_dev_batch b = make_batch(d, *x, nslots, ngroups);
    b.max_npk = max_npk;
    b.path = path;
    rc = exec_reserve_lines(*x, b);
    bgv_streams S{x->main, nullptr};
    const bool ok = rc == BGV_OK &&
        hipMemcpyAsync(x->d_slots, slots.data(), sizeof(bgv_dslot) * nslots, hipMemcpyHostToDevice, x->main) ==
            hipSuccess &&
        hipMemcpyAsync(x->d_groups, groups.data(), sizeof(bgv_dgroup) * ngroups, hipMemcpyHostToDevice, x->main) ==
            hipSuccess &&
        hipMemcpyAsync(x->d_idx, idx.data(), 4 * idx.size(), hipMemcpyHostToDevice, x->main) == hipSuccess &&
        bgv_launch_sets(b, S) == hipSuccess && bgv_launch_debug_out(b, dh, df, x->main) == hipSuccess &&
        hipMemcpyAsync(out_h192, dh, 192 * nsets, hipMemcpyDeviceToHost, x->main) == hipSuccess &&
        hipMemcpyAsync(out_f576, df, 576 * nsets, hipMemcpyDeviceToHost, x->main) == hipSuccess &&
        hipMemcpyAsync(ss.data(), b.sig_status, 4ull * nslots, hipMemcpyDeviceToHost, x->main) == hipSuccess &&
        hipMemcpyAsync(ps.data(), b.pk_status, 4ull * nslots, hipMemcpyDeviceToHost, x->main) == hipSuccess &&
        hipStreamSynchronize(x->main) == hipSuccess;
    if (!ok) rc = -BGV_E_DEVICE;
  }
  if (dh) (void)hipFree(dh);
  if (df) (void)hipFree(df);
  exec_destroy(x);  // synchronizes x->main first
  if (dstream) (void)hipStreamDestroy(dstream);
  if (rc) return rc;
  for (size_t i = 0; i < nsets; ++i) {
    out_status[2 * i] = ss[i];
    out_status[2 * i + 1] = ps[i];
  }
  return BGV_OK;
}

int bgv_debug_uniform(bgv_ctx* c, const bgv_set* sets, size_t nsets, uint64_t seed, const uint64_t* test_masks,
                      const uint32_t* test_weighted, size_t ntests, uint8_t* out_first576, uint8_t* out_pk576,
                      uint8_t* out_sig576) {
  if (!c || nsets < 2 || nsets > BGV_WAVE || !sets || !out_first576 || ntests > BGV_WAVE ||
      (ntests && (!test_masks || !test_weighted || !out_pk576 || !out_sig576)))
    return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  // one uniform first-pass group: every set signs the first set's root (hsrc 0)
  std::vector<bgv_dslot> slots;
  std::vector<uint32_t> idx;
  uint64_t state = seed;
  uint32_t max_npk = 0;
  for (size_t i = 0; i < nsets; ++i) {
    const bgv_set& st = sets[i];
    if (!st.pk_indices || st.n_pk == 0 || !st.msg || st.sig_len != 96 || !st.sig ||
        memcmp(st.msg, sets[0].msg, 32) != 0)
      return -BGV_E_ARG;
    for (uint32_t q = 0; q < st.n_pk; ++q)
      if (st.pk_indices[q] >= c->n_pubkeys || c->bad_pk.count(st.pk_indices[q])) return -BGV_E_BAD_INDEX;
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.flags = BGV_SLOT_PK_CACHED;
    s.n_pk = st.n_pk;
    s.sig_len = st.sig_len;
    s.pk_off = (uint32_t)idx.size();
    idx.insert(idx.end(), st.pk_indices, st.pk_indices + st.n_pk);
    memcpy(s.msg, st.msg, 32);
    memcpy(s.sig, st.sig, 96);
    s.group = 0;
    s.hsrc = 0;
    do s.scalar = splitmix64(&state);
    while (s.scalar == 0);
    max_npk = std::max(max_npk, st.n_pk);
    slots.push_back(s);
  }
  while (slots.size() % BGV_WAVE) {
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.flags = BGV_SLOT_PAD;
    s.hsrc = (uint32_t)slots.size();
    slots.push_back(s);
  }
  const uint32_t nslots = (uint32_t)slots.size(), nt = (uint32_t)ntests;
  const bgv_dgroup first{0u, (uint32_t)nsets, BGV_ALL_SLOTS, 0u, BGV_GROUP_UNIFORM};
  // the tests as a retry round lays them out (retry_launch): groups, then the uniform list
  const uint32_t per = (uint32_t)(sizeof(bgv_dgroup) / sizeof(uint32_t));
  const uint32_t nlist = (nt + per - 1) / per;
  std::vector<bgv_dgroup> tg(nt + nlist);
  bool weighted = false;
  for (uint32_t t = 0; t < nt; ++t) {
    tg[t] = bgv_dgroup{0u, (uint32_t)nsets, test_masks[t], 0u,
                       BGV_GROUP_UNIFORM | (test_weighted[t] ? BGV_GROUP_WEIGHTED : 0u)};
    weighted = weighted || test_weighted[t];
    reinterpret_cast<uint32_t*>(tg.data() + nt)[t] = t;
  }
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  Exec* x = new Exec();
  uint8_t* dout = nullptr;
  int rc = exec_create(x);
  hipStream_t dstream = nullptr;
  if (!rc && hipStreamCreateWithFlags(&dstream, hipStreamNonBlocking) != hipSuccess) rc = -BGV_E_DEVICE;
  x->main = dstream;
  if (!rc) rc = exec_reserve_slots(*x, nslots);
  if (!rc) rc = exec_reserve_groups(*x, std::max<uint32_t>(1, nt + nlist));
  if (!rc) rc = grow(&x->d_idx, &x->idx_cap, idx.size());
  if (!rc && hipMalloc(reinterpret_cast<void**>(&dout), 576ull * (1 + 2 * nt)) != hipSuccess) rc = -BGV_E_DEVICE;
  if (!rc) {
    bgv_dev_batch b = make_batch(d, *x, nslots, 1);
    b.max_npk = max_npk;
    b.path = BGV_PATH_BULK;
    b.uniform = true;
    rc = exec_reserve_lines(*x, b);
    bgv_streams S{x->main, nullptr};
    bool ok = rc == BGV_OK &&
        hipMemcpyAsync(x->d_slots, slots.data(), sizeof(bgv_dslot) * nslots, hipMemcpyHostToDevice, x->main) ==
            hipSuccess &&
        hipMemcpyAsync(x->d_groups, &first, sizeof(bgv_dgroup), hipMemcpyHostToDevice, x->main) == hipSuccess &&
        hipMemcpyAsync(x->d_idx, idx.data(), 4 * idx.size(), hipMemcpyHostToDevice, x->main) == hipSuccess &&
        bgv_launch_sets(b, S) == hipSuccess &&
        bgv_launch_fp12_bytes(b.gpkp, 1, dout, x->main) == hipSuccess;
    if (ok && nt) {
      // the tests over the first pass's per-slot results (r_i sig_i, r_i pk_i, H)
      bgv_dev_batch t = make_batch(d, *x, nslots, nt);
      t.max_npk = max_npk;
      t.path = BGV_PATH_BULK;
      t.uniform = true;
      t.upk = reinterpret_cast<const uint32_t*>(t.groups + nt);
      t.npk = nt;
      t.weighted = weighted;
      ok = hipMemcpyAsync(x->d_groups, tg.data(), sizeof(bgv_dgroup) * tg.size(), hipMemcpyHostToDevice, x->main) ==
               hipSuccess &&
           bgv_launch_gpairs(t, x->main) == hipSuccess &&
           bgv_launch_fp12_bytes(t.gpkp, nt, dout + 576, x->main) == hipSuccess &&
           bgv_launch_fp12_bytes(t.gpair, nt, dout + 576ull * (1 + nt), x->main) == hipSuccess &&
           hipMemcpyAsync(out_pk576, dout + 576, 576ull * nt, hipMemcpyDeviceToHost, x->main) == hipSuccess &&
           hipMemcpyAsync(out_sig576, dout + 576ull * (1 + nt), 576ull * nt, hipMemcpyDeviceToHost, x->main) ==
               hipSuccess;
    }
    ok = ok && hipMemcpyAsync(out_first576, dout, 576, hipMemcpyDeviceToHost, x->main) == hipSuccess &&
         hipStreamSynchronize(x->main) == hipSuccess;
    if (!ok) rc = -BGV_E_DEVICE;
  }
  if (dout) (void)hipFree(dout);
  exec_destroy(x);
  if (dstream) (void)hipStreamDestroy(dstream);
  return rc;
}

int bgv_aggregate_pubkeys(bgv_ctx* c, const uint32_t* idx, size_t n, uint8_t out96[96]) {
  if (!c || !out96 || (n && !idx)) return -BGV_E_ARG;
  if (n == 0) return -BGV_E_EMPTY_AGGREGATE;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  for (size_t i = 0; i < n; ++i)
    if (idx[i] >= c->n_pubkeys || c->bad_pk.count(idx[i])) return -BGV_E_BAD_INDEX;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  // one cached-key slot through the verify path's aggregation (k_pk_agg / pk_sum)
  bgv_dslot s;
  memset(&s, 0, sizeof(s));
  s.flags = BGV_SLOT_PK_CACHED;
  s.n_pk = (uint32_t)n;
  uint32_t* di = nullptr;
  uint8_t* dout = nullptr;
  bgv_dslot* ds = nullptr;
  void* dagg = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&di), 4 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dout), 96));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&ds), sizeof(bgv_dslot)));
  HIPCHK(hipMalloc(&dagg, bgv_g1_point_bytes()));
  HIPCHK(hipMemcpyAsync(di, idx, 4 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(ds, &s, sizeof(s), hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_aggregate(ds, di, (uint32_t)n, d.cache, dagg, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  void* bufs[] = {di, dout, ds, dagg};
  for (void* p : bufs) (void)hipFree(p);
  return BGV_OK;
}

int bgv_aggregate_committee_bits(bgv_ctx* c, uint32_t id, const uint8_t* bits, uint32_t n_bits, uint8_t out96[96]) {
  if (!c || !out96 || (n_bits && !bits)) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  // one committee set through the call's own checks and layout, then k_pk_agg_bits / pk_sum
  const uint8_t zero[96] = {0};
  bgv_set st{};
  st.sig_len = 96;
  st.msg = zero;
  st.sig = zero;
  const bgv_pkbits pb{id, n_bits, bits};
  const bgv_job jb{0, 1, 0};
  Call call;
  call.setcom.assign(1, SetCommittee{});
  int32_t code = 2;
  {
    std::shared_lock<std::shared_mutex> mlk(c->com_mu);
    if (host_job_code(c, jb, &st, &code, &pb, &call) != BGV_OK) return -BGV_E_ARG;
  }
  if (code != 2) return code;
  Layout L;
  std::vector<size_t> todo;
  layout_call(L, todo, &jb, 1, &st, BGV_MODE_PER_JOB, {2}, call.setcom.data());
  const uint32_t list = 0;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  uint32_t* di = nullptr;
  uint8_t* dout = nullptr;
  bgv_dslot* ds = nullptr;
  void* dagg = nullptr;
  const bool ok =
      hipMalloc(reinterpret_cast<void**>(&di), 4 * (L.idx.size() + 1)) == hipSuccess &&
      hipMalloc(reinterpret_cast<void**>(&dout), 96) == hipSuccess &&
      hipMalloc(reinterpret_cast<void**>(&ds), sizeof(bgv_dslot)) == hipSuccess &&
      hipMalloc(&dagg, bgv_g1_point_bytes()) == hipSuccess &&
      hipMemcpyAsync(di, L.idx.data(), 4 * L.idx.size(), hipMemcpyHostToDevice, d.stream) == hipSuccess &&
      hipMemcpyAsync(di + L.idx.size(), &list, 4, hipMemcpyHostToDevice, d.stream) == hipSuccess &&
      hipMemcpyAsync(ds, L.slots.data(), sizeof(bgv_dslot), hipMemcpyHostToDevice, d.stream) == hipSuccess &&
      bgv_launch_aggregate_bits(ds, di, di + L.idx.size(), !L.com_team.empty(), d.com_dir, d.com_pool, d.cache, dagg,
                                dout, d.stream) == hipSuccess &&
      hipMemcpyAsync(out96, dout, 96, hipMemcpyDeviceToHost, d.stream) == hipSuccess;
  // the stream drains before the buffers (and the host arrays the copies read) go, on every path
  const bool done = hipStreamSynchronize(d.stream) == hipSuccess;
  void* bufs[] = {di, dout, ds, dagg};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  return ok && done ? BGV_OK : -BGV_E_DEVICE;
}

int bgv_hash_to_g2(bgv_ctx* c, const uint8_t* msgs, const uint32_t* lens, size_t n, uint8_t* out192) {
  if (!c || (n && (!lens || !out192))) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  std::vector<uint32_t> offs(n);
  size_t tot = 0;
  for (size_t i = 0; i < n; ++i) {
    if (lens[i] > 1024) return -BGV_E_ARG;
    offs[i] = (uint32_t)tot;
    tot += lens[i];
  }
  if (tot && !msgs) return -BGV_E_ARG;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  uint8_t *dm = nullptr, *dout = nullptr;
  uint32_t *doff = nullptr, *dlen = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dm), tot + 1));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&doff), 4 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dlen), 4 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dout), 192 * n));
  if (tot) HIPCHK(hipMemcpyAsync(dm, msgs, tot, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(doff, offs.data(), 4 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dlen, lens, 4 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_hash(dm, doff, dlen, (uint32_t)n, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out192, dout, 192 * n, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  (void)hipFree(dm);
  (void)hipFree(doff);
  (void)hipFree(dlen);
  (void)hipFree(dout);
  return BGV_OK;
}

int bgv_pubkeys_validate(bgv_ctx* c, const uint8_t* keys48, size_t n, int32_t* out_status, uint8_t* out96) {
  if (!c || (n && (!keys48 || !out_status))) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  uint8_t *dk = nullptr, *dout = nullptr;
  int32_t* dst = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dk), 48 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dout), 96 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dst), 4 * n));
  HIPCHK(hipMemcpyAsync(dk, keys48, 48 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_pk_validate(dk, (uint32_t)n, dst, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out_status, dst, 4 * n, hipMemcpyDeviceToHost, d.stream));
  if (out96) HIPCHK(hipMemcpyAsync(out96, dout, 96 * n, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  (void)hipFree(dk);
  (void)hipFree(dout);
  (void)hipFree(dst);
  for (size_t i = 0; i < n; ++i) out_status[i] = -out_status[i];
  return BGV_OK;
}

int bgv_aggregate_signatures(bgv_ctx* c, const uint8_t* sigs96, const uint32_t* lens, const uint32_t* counts,
                             size_t naggs, uint8_t* out96, int32_t* out_status) {
  if (!c || (naggs && (!counts || !out96 || !out_status))) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (naggs == 0) return BGV_OK;
  std::vector<uint32_t> first(naggs);
  size_t n = 0;
  for (size_t a = 0; a < naggs; ++a) {
    first[a] = (uint32_t)n;
    n += counts[a];
  }
  if (n && (!sigs96 || !lens)) return -BGV_E_ARG;
  std::vector<int32_t> st(n);
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  uint8_t *ds = nullptr, *dout = nullptr;
  uint32_t *dl = nullptr, *df = nullptr, *dc = nullptr;
  int32_t* dst = nullptr;
  void* pts = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&ds), 96 * n + 1));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dl), 4 * n + 4));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dst), 4 * n + 4));
  HIPCHK(hipMalloc(&pts, bgv_g2_point_bytes() * n + 1));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&df), 4 * naggs));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dc), 4 * naggs));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dout), 96 * naggs));
  if (n) {
    HIPCHK(hipMemcpyAsync(ds, sigs96, 96 * n, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(dl, lens, 4 * n, hipMemcpyHostToDevice, d.stream));
  }
  HIPCHK(hipMemcpyAsync(df, first.data(), 4 * naggs, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dc, counts, 4 * naggs, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_sig_aggregate(ds, dl, (uint32_t)n, df, dc, (uint32_t)naggs, pts, dst, dout, d.stream));
  if (n) HIPCHK(hipMemcpyAsync(st.data(), dst, 4 * n, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96 * naggs, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  void* bufs[] = {ds, dl, dst, pts, df, dc, dout};
  for (void* b : bufs) (void)hipFree(b);
  // verdict per aggregate: the first signature (in order) that fails to decode or
  // validate, as Signature.fromBytes throws on it; [] -> EMPTY_AGGREGATE_ARRAY
  for (size_t a = 0; a < naggs; ++a) {
    int32_t code = counts[a] ? BGV_OK : -BGV_E_EMPTY_AGGREGATE;
    for (uint32_t k = 0; k < counts[a] && code == BGV_OK; ++k)
      if (st[first[a] + k] != BGV_OK) code = -st[first[a] + k];
    out_status[a] = code;
    if (code != BGV_OK) memset(out96 + 96 * a, 0, 96);
  }
  return BGV_OK;
}

int bgv_deposits_verify(bgv_ctx* c, const uint8_t* keys48, const uint8_t* msgs32, const uint8_t* sigs96, size_t n,
                        int32_t* out_valid) {
  if (!c || (n && (!keys48 || !msgs32 || !sigs96 || !out_valid))) return -BGV_E_ARG;
  if (n == 0) return BGV_OK;
  std::vector<int32_t> ks(n);
  std::vector<uint8_t> pk96(96 * n);
  int rc = bgv_pubkeys_validate(c, keys48, n, ks.data(), pk96.data());
  if (rc) return rc;
  // every deposit with a valid key is its own job (Signature.verify per deposit)
  std::vector<bgv_set> sets;
  std::vector<bgv_job> jobs;
  std::vector<size_t> which;
  for (size_t i = 0; i < n; ++i) {
    out_valid[i] = 0;
    if (ks[i] != BGV_OK) continue;
    bgv_set st{};
    st.n_pk = 1;
    st.sig_len = 96;
    st.pk_bytes = pk96.data() + 96 * i;
    st.msg = msgs32 + 32 * i;
    st.sig = sigs96 + 96 * i;
    jobs.push_back(bgv_job{(uint32_t)sets.size(), 1, 0});
    sets.push_back(st);
    which.push_back(i);
  }
  if (jobs.empty()) return BGV_OK;
  std::vector<int32_t> codes(jobs.size());
  rc = bgv_verify(c, jobs.data(), jobs.size(), sets.data(), sets.size(), BGV_MODE_PER_JOB, codes.data(), nullptr);
  if (rc) return rc;
  // processDeposit.ts:62-70 catches every BLS error: anything but "valid" is invalid
  for (size_t k = 0; k < which.size(); ++k) out_valid[which[k]] = codes[k] == 1 ? 1 : 0;
  return BGV_OK;
}

int bgv_keygen(bgv_ctx* c, const uint8_t* sks, size_t n, int64_t cache_first, uint8_t* out48) {
  if (!c || (n && !sks)) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  std::unique_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  if (cache_first > (int64_t)c->n_pubkeys) return -BGV_E_ARG;
  if (n == 0) return BGV_OK;
  if (cache_first >= 0) {
    int rc = cache_reserve(c, (size_t)cache_first + n);
    if (rc) return rc;
  }
  const size_t esz = bgv_cache_entry_bytes();
  for (size_t di = 0; di < c->devs.size(); ++di) {
    Device& d = c->devs[di];
    if (cache_first < 0 && di > 0) break;
    HIPCHK(hipSetDevice(d.id));
    uint8_t *dsk = nullptr, *dout = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&dsk), 32 * n));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&dout), 48 * n));
    HIPCHK(hipMemcpyAsync(dsk, sks, 32 * n, hipMemcpyHostToDevice, d.stream));
    bgv_cache_entry* dst =
        cache_first >= 0 ? reinterpret_cast<bgv_cache_entry*>(reinterpret_cast<uint8_t*>(d.cache) + esz * cache_first)
                         : nullptr;
    HIPCHK(bgv_launch_keygen(dsk, (uint32_t)n, dst, dout, d.stream));
    if (out48 && di == 0) HIPCHK(hipMemcpyAsync(out48, dout, 48 * n, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    (void)hipFree(dsk);
    (void)hipFree(dout);
  }
  if (cache_first >= 0) {
    const size_t old_n = c->n_pubkeys.load();
    for (size_t i = 0; i < n; ++i) c->bad_pk.erase((uint32_t)(cache_first + i));
    c->n_pubkeys.store(std::max(old_n, (size_t)cache_first + n));
    if ((size_t)cache_first < old_n) return committees_refresh(c, (uint32_t)cache_first, n);
  }
  return BGV_OK;
}

int bgv_sign(bgv_ctx* c, const uint8_t* sks, const uint8_t* msgs, size_t n, uint8_t* out96) {
  if (!c || (n && (!sks || !msgs || !out96))) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  uint8_t *dsk = nullptr, *dm = nullptr, *dout = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dsk), 32 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dm), 32 * n));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dout), 96 * n));
  HIPCHK(hipMemcpyAsync(dsk, sks, 32 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dm, msgs, 32 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_sign(dsk, dm, (uint32_t)n, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96 * n, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  (void)hipFree(dsk);
  (void)hipFree(dm);
  (void)hipFree(dout);
  return BGV_OK;
}

int bgv_profile(bgv_ctx* c, int enable, double* kernel_ms, const char** names, int n, uint64_t* launches) {
  if (!c) return -BGV_E_ARG;
  std::lock_guard<std::mutex> lk(c->prof_mu);
  for (int k = 0; k < n && k < BGV_NKERNELS; ++k) {
    if (kernel_ms) kernel_ms[k] = c->kernel_ms[k];
    if (names) names[k] = BGV_KERNEL_NAMES[k];
  }
  if (launches) *launches = c->kernel_launches;
  if (enable >= 0) {
    c->profile = enable != 0;
    for (double& v : c->kernel_ms) v = 0;
    c->kernel_launches = 0;
  }
  return BGV_NKERNELS;
}

const char* bgv_strerror(int code) {
  if (code < 0) code = -code;
  switch (code) {
    case BGV_OK: return "BLST_SUCCESS";
    case BGV_BLST_BAD_ENCODING: return "BLST_BAD_ENCODING";
    case BGV_BLST_POINT_NOT_ON_CURVE: return "BLST_POINT_NOT_ON_CURVE";
    case BGV_BLST_POINT_NOT_IN_GROUP: return "BLST_POINT_NOT_IN_GROUP";
    case BGV_BLST_AGGR_TYPE_MISMATCH: return "BLST_AGGR_TYPE_MISMATCH";
    case BGV_BLST_VERIFY_FAIL: return "BLST_VERIFY_FAIL";
    case BGV_BLST_PK_IS_INFINITY: return "BLST_PK_IS_INFINITY";
    case BGV_BLST_BAD_SCALAR: return "BLST_BAD_SCALAR";
    case BGV_BLST_INVALID_SIZE: return "BLST_INVALID_SIZE";
    case BGV_E_EMPTY_AGGREGATE: return "EMPTY_AGGREGATE_ARRAY";
    case BGV_E_EMPTY_SET: return "Empty signature set";
    case BGV_E_BAD_INDEX: return "BGV_E_BAD_INDEX: validator index not in the device pubkey cache";
    case BGV_E_ARG: return "BGV_E_ARG: invalid argument";
    case BGV_E_DEVICE: return "BGV_E_DEVICE: HIP device error";
    case BGV_E_NOMEM: return "BGV_E_NOMEM";
    case BGV_E_CLOSED: return "QUEUE_ABORTED";
    default: return "BGV_E_UNKNOWN";
  }
}

}  // extern "C"
