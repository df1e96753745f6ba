// The host state the orchestration units share (bgv_sched.cpp, bgv_registry.cpp, bgv_calls.cpp):
// the context, its devices and their buffers, a call on its way through a dispatcher, and the
// few helpers that cross unit boundaries.  Host-only; no kernel unit includes it.  Everything
// here has hidden visibility: the library exports the C ABI of include/blsgpu.h and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
#include "bgv_devscope.h"

#pragma GCC visibility push(hidden)

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

// bgv_verify_aggregate's aggregation step (bgv_sigagg.cpp; under util_mu): the accepted
// signatures in member order, their points and statuses, per aggregate {first, count} and the
// compressed sums, with the pinned staging of each.  Grown to the largest call seen.
struct SigAggScratch {
  uint8_t* d_sigs = nullptr;  // sig_cap x 96
  void* d_pts = nullptr;      // sig_cap x bgv_g2_point_bytes()
  int32_t* d_st = nullptr;    // sig_cap
  size_t sig_cap = 0;
  uint32_t* d_fc = nullptr;  // first[agg_cap], count[agg_cap]
  uint8_t* d_out = nullptr;  // agg_cap x 96
  size_t agg_cap = 0;
  Pinned<uint8_t> h_sigs, h_out;
  Pinned<int32_t> h_st;
  Pinned<uint32_t> h_fc;
};

// Signature pools (bgv_sigpool.cpp; under util_mu): the accumulators, and the scratch of the
// accumulation step and of bgv_sigpool_get beside SigAggScratch's signatures, points and statuses,
// which the step shares.  Grown to the largest call seen.
struct SigPoolDev {
  void* d_acc = nullptr;       // BGV_MAX_SIGPOOL x bgv_g2_point_bytes(), allocated at the first open
  uint32_t* d_meta = nullptr;  // ids[cap], first[cap], count[cap], fresh[cap] of the touched entries
  int32_t* d_flag = nullptr;   // cap
  size_t cap = 0;
  uint32_t* d_gids = nullptr;  // bgv_sigpool_get: get_cap ids and their compressed sums
  uint8_t* d_gout = nullptr;
  size_t get_cap = 0;
  uint32_t* d_sids = nullptr;  // bgv_sigpool_sum: sid_cap ids of written entries, group after group
  size_t sid_cap = 0;
  uint32_t* d_sfc = nullptr;   // first[sum_cap], count[sum_cap] of the groups the device answers
  uint8_t* d_sout = nullptr;   // sum_cap x 96
  size_t sum_cap = 0;
  Pinned<uint32_t> h_meta, h_gids, h_sids, h_sfc;
  Pinned<int32_t> h_flag;
  Pinned<uint8_t> h_gout, h_sout;
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
struct bgv_ctx;
struct SigPoolFields;  // bgv_sigpool_bits_plan.h
// One bgv_verify_aggregate or bgv_verify_accumulate call between its verdicts and its step on
// device 0's utility stream (the context's aggregation worker runs the asynchronous ones).
struct SigAggTask {
  bgv_ctx* c = nullptr;
  const bgv_job* jobs = nullptr;
  size_t njobs = 0;
  const bgv_set* sets = nullptr;
  size_t nsets = 0;
  const uint32_t* agg_of_set = nullptr;  // bgv_verify_accumulate: pool_of_set
  size_t naggs = 0;
  const int32_t* codes = nullptr;
  uint8_t* out96 = nullptr;
  int32_t* out_status = nullptr;
  uint32_t* out_count = nullptr;
  bgv_stats* stats = nullptr;
  bgv_done_fn done = nullptr;
  void* user = nullptr;
  std::chrono::steady_clock::time_point t0;
  // the step, when it is not the aggregation: bgv_verify_accumulate's, with the generation of every
  // set's entry at submit and out_added
  int (*step)(const SigAggTask&) = nullptr;
  std::vector<uint32_t> gen_of_set;
  uint8_t* out_added = nullptr;
  // bgv_verify_accumulate_bits: the submit's copy of bits_of_set, and out_outcome in out_added's place
  std::shared_ptr<SigPoolFields> fields;
};
// What a super-batch's retry rounds need from its first pass.
struct BatchState {
  std::chrono::steady_clock::time_point tb;
  double t_merge = 0, t_tok = 0, t_sets = 0, t_pass1 = 0, t_post = 0;
  uint32_t nslots = 0, ngroups = 0;
  std::vector<uint32_t> call_gb;  // each call's first group in the merged batch
  bool want_gu = false;           // the first pass's u values are in x.d_gu1 (pattern tests)
  bool uniform = false;           // the first pass ran uniform groups (their slots have no own pair f_i)
  bool bulk = false;              // the first pass took the bulk path: retry rounds feed their teams line records
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
  SigAggScratch sigagg;               // device 0 only
  SigPoolDev sigpool;                 // device 0 only
  std::vector<Exec*> execs;
  // held while one super-batch runs its per-set kernels (pointer: Device stays movable)
  std::unique_ptr<std::mutex> compute_mu = std::make_unique<std::mutex>();
};

// One bgv_verify call travelling through a dispatcher: its host state (layout, codes, retry
// units: CallPlan, bgv_retry_plan.h) and how its caller hears of the end.
struct Call : CallPlan {
  const bgv_set* sets = nullptr;
  std::vector<SetCommittee> setcom;                     // per set once checked (empty for bgv_verify)
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
  // bgv_verify_aggregate_async: calls whose codes are final and whose aggregation waits for the
  // context's aggregation worker (started by the first such call; bgv_sigagg.cpp)
  std::mutex agg_mu;
  std::condition_variable agg_cv;
  std::deque<SigAggTask*> agg_q;
  std::thread agg_worker;
  bool agg_stop = false;
  // aggregation steps launched with the wavefront form [0] and the lane form [1] (bgv_debug_sigagg_launches)
  std::atomic<uint64_t> sigagg_launches[2] = {};
  // Signature pools (bgv_sigpool.cpp): per id whether it is live, its generation (changed by every
  // open), how many signatures it holds and whether its accumulator has been written since it was
  // opened.  pool_mu guards these; whoever also works on the device takes util_mu first.
  std::mutex pool_mu;
  std::vector<uint8_t> pool_live, pool_written;
  std::vector<uint32_t> pool_gen, pool_count;
  // entries with participation bits: positions per id (0: a plain entry) and, allocated by the first
  // bgv_sigpool_open_bits, BGV_MAX_SIGPOOL x BGV_SIGPOOL_BITS_BYTES of fields
  std::vector<uint32_t> pool_nbits;
  std::vector<uint8_t> pool_bits;
  std::atomic<uint64_t> sigpool_launches[2] = {};  // as sigagg_launches (bgv_debug_sigpool_launches)
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

// DevScope's default policy
struct HipDevApi {
  using stream_t = hipStream_t;
  static bool alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }
  static void free(void* p) { (void)hipFree(p); }
  static bool sync(stream_t s) { return hipStreamSynchronize(s) == hipSuccess; }
};

// bgv_sched.cpp
int exec_create(Exec* x);
void exec_destroy(Exec* x);
int exec_reserve_slots(Exec& x, uint32_t slots);
int exec_reserve_groups(Exec& x, uint32_t groups);
int exec_reserve_lines(Exec& x, bgv_dev_batch& b);
int exec_reserve_line_pairs(Exec& x, bgv_dev_batch& b, uint32_t need);  // a retry round's team pairs
bgv_dev_batch make_batch(Device& d, Exec& x, uint32_t nslots, uint32_t ngroups);
int host_job_code(bgv_ctx* c, const bgv_job& jb, const bgv_set* sets, int32_t* code, PkForm pk = PkForm(),
                  Call* call = nullptr);
void fp12_one_bytes(uint8_t out[576]);
// bgv_sigagg.cpp
void sigagg_stop(bgv_ctx* c);   // bgv_close: queued aggregations end with -BGV_E_CLOSED, the worker is joined
void sigagg_free(Device& d);    // ctx_free_devices
size_t sigagg_wave_max();
int sigagg_reserve(SigAggScratch& s, size_t n, size_t naggs);
int sigagg_worker_start(bgv_ctx* c);          // BGV_OK, or -BGV_E_CLOSED once bgv_close has begun
void sigagg_verify_done(void* user, int rc);  // a verify call's done(): hands its SigAggTask to the worker
// bgv_sigpool.cpp
void sigpool_free(Device& d);  // ctx_free_devices

#pragma GCC visibility pop
