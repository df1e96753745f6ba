// libblsgpu: the device-resident registries: the pubkey cache, committees, epoch shuffling, sampling and keygen.
#include "bgv_ctx.h"
#include "bgv_sample.h"   // balance-weighted sampling (bgv_proposers, bgv_sync_committee_put)
#include "bgv_shuffle.h"  // the committee bounds of an epoch shuffling (bgv_shuffling_put)
#include "bls_constants.h"

extern "C" {

size_t bgv_pubkeys_count(const bgv_ctx* c) { return c ? c->n_pubkeys.load() : 0; }

// grow every device's cache to hold `need` entries (contents preserved); caller holds cache_mu exclusively
static int cache_reserve(bgv_ctx* c, size_t need) {
  const size_t esz = bgv_cache_entry_bytes();
  for (Device& d : c->devs) {
    HIPCHK(hipSetDevice(d.id));
    if (need <= d.cache_cap) continue;
    size_t cap = std::max(need, d.cache_cap * 2);
    DevScope<> sc(d.stream);
    void* p = nullptr;
    if (int rc = sc.alloc(&p, esz * cap)) return rc;
    if (d.cache) {
      HIPCHK(hipMemcpyAsync(p, d.cache, esz * c->n_pubkeys, hipMemcpyDeviceToDevice, d.stream));
      if (int rc = sc.sync()) return rc;
      HIPCHK(hipFree(d.cache));
    }
    d.cache = static_cast<bgv_cache_entry*>(sc.release(p));
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
    DevScope<> sc(d.stream);
    uint32_t* p = nullptr;
    if (int rc = sc.alloc(&p, cap)) return rc;
    HIPCHK(hipMemcpyAsync(p, d.com_pool, 4 * old, hipMemcpyDeviceToDevice, d.stream));
    if (int rc = sc.sync()) return rc;
    HIPCHK(hipFree(d.com_pool));
    d.com_pool = sc.release(p);
  }
  std::lock_guard<std::mutex> lk(P.mu);
  P.add_range((uint32_t)old, (uint32_t)(cap - old));
  P.cap = cap;
  return BGV_OK;
}

// bgv_committee_put under put_mu (the caller's): the checks, a handle and a pool range, the list
// and its sum on every device, then the id.  bgv_sync_committee_put stores its picks through it.
static int committee_put_locked(bgv_ctx* c, uint32_t id, const uint32_t* indices, size_t n) {
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

int bgv_committee_put(bgv_ctx* c, uint32_t id, const uint32_t* indices, size_t n) {
  if (!c || id >= BGV_MAX_COMMITTEES || !indices || n < 1 || n > 65536) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  return committee_put_locked(c, id, indices, n);
}

// bgv_committee_drop under put_mu (the caller's)
static int committee_drop_locked(bgv_ctx* c, uint32_t id) {
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

int bgv_committee_drop(bgv_ctx* c, uint32_t id) {
  if (!c) return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  return committee_drop_locked(c, id);
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
        DevScope<> sc(d.stream);
        if (d.shuf_cap < words) {
          uint32_t* p = nullptr;
          if (int rc = sc.alloc(&p, words)) return rc;
          if (d.shuf_buf) (void)hipFree(d.shuf_buf);
          d.shuf_buf = sc.release(p);
          d.shuf_cap = words;
        }
        sc.enqueued();  // from here on the stream reads active and handles and writes shuf
        HIPCHK(hipMemcpyAsync(d.shuf_buf, active, 4 * (size_t)n, hipMemcpyHostToDevice, d.stream));
        HIPCHK(hipMemcpyAsync(d.com_list, handles.data(), 4 * (size_t)m, hipMemcpyHostToDevice, d.stream));
        HIPCHK(bgv_launch_shuffle(seed, n, rounds, d.shuf_buf, d.com_pool + base, d.stream));
        HIPCHK(bgv_launch_shuffle_dir(d.com_dir, d.com_list, m, base, n, count, d.stream));
        HIPCHK(bgv_launch_committee_totals(d.com_dir, d.com_list, m, d.com_pool, d.cache, d.stream));
        if (first)
          HIPCHK(hipMemcpyAsync(shuf.data(), d.com_pool + base, 4 * (size_t)n, hipMemcpyDeviceToHost, d.stream));
        first = false;
        if (int rc = sc.sync()) return rc;
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

}  // extern "C"

static_assert(BGV_SAMPLE_CAP == BGV_SAMPLE_MAX_TRIES, "bgv_sample.h plans its passes within the public cap");

namespace {
// samp_run's device: one pass is k_sample_eval (the rule's: in.rule) + k_sample_pick over the seeds still short, on the
// utility stream, and one synchronize that reads the seeds' states back.
struct SampleDev {
  Device& d;
  DevScope<>& sc;
  bgv_sample_in in;
  uint32_t n_seeds;
  uint32_t* todo = nullptr;  // n_seeds words
  uint32_t* vals = nullptr;  // one pass's results: cap candidates
  uint8_t* flags = nullptr;
  size_t cap = 0;
  int pass(const std::vector<uint32_t>& todo_h, const samp_pass& p, std::vector<samp_state>& st) {
    const size_t items = todo_h.size() * (size_t)p.window;
    if (items > cap) {  // the smaller ones stay with the scope until the call ends
      if (sc.alloc(&vals, items) || sc.alloc(&flags, items)) return -BGV_E_DEVICE;
      cap = items;
    }
    sc.enqueued();  // the stream reads todo_h and writes st
    HIPCHK(hipMemcpyAsync(todo, todo_h.data(), 4 * todo_h.size(), hipMemcpyHostToDevice, d.stream));
    HIPCHK(bgv_launch_sample_pass(in, todo, (uint32_t)todo_h.size(), p.window, p.count, vals, flags, d.stream));
    HIPCHK(hipMemcpyAsync(st.data(), in.state, sizeof(samp_state) * n_seeds, hipMemcpyDeviceToHost, d.stream));
    return sc.sync();
  }
};

// What the rule sets: the balance table's element size and the largest max_incr.
size_t sample_eff_bytes(samp_rule_id rule) {
  return rule == SAMP_RULE_U16 ? sizeof(samp_rule16::eff_t) : sizeof(samp_rule8::eff_t);
}
uint32_t sample_max_incr(samp_rule_id rule) {
  return rule == SAMP_RULE_U16 ? samp_rule16::MAX_INCR : samp_rule8::MAX_INCR;
}

bool sample_args_ok(const uint32_t* active, size_t n_active, const void* eff, size_t n_eff, uint32_t max_incr,
                    uint32_t rounds, samp_rule_id rule) {
  if (!active || !eff || n_active < 1 || n_active > BGV_SHUFFLE_MAX_N || n_eff < 1 || n_eff > (size_t)UINT32_MAX ||
      rounds > BGV_SHUFFLE_MAX_ROUNDS || max_incr < 1 || max_incr > sample_max_incr(rule))
    return false;
  for (size_t i = 0; i < n_active; ++i)
    if (active[i] >= n_eff) return false;
  return true;
}

// The first `want` accepted candidates of each seed, sampled on the first device: st[s].have of
// them at picks[s * want ..).  eff holds n_eff elements of the rule's type.  Under the shared
// cache_mu (the devices stay); takes util_mu.
int sample_run(bgv_ctx* c, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active, uint32_t n,
               const void* eff, size_t n_eff, samp_rule_id rule, uint32_t max_incr, uint32_t rounds, uint32_t want,
               uint32_t limit, std::vector<samp_state>& st, std::vector<uint32_t>& picks) {
  const size_t eff_bytes = n_eff * sample_eff_bytes(rule);
  std::vector<shuf_seed> seeds(n_seeds);
  for (uint32_t s = 0; s < n_seeds; ++s) seeds[s] = shuf_seed_load(seeds32 + 32 * (size_t)s);
  picks.assign((size_t)n_seeds * want, 0);
  std::lock_guard<std::mutex> ulk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  DevScope<> sc(d.stream);
  shuf_seed* dseeds = nullptr;
  samp_state* dstate = nullptr;
  uint32_t *dact = nullptr, *dpicks = nullptr, *dtodo = nullptr;
  uint8_t* deff = nullptr;
  if (sc.alloc(&dseeds, n_seeds) || sc.alloc(&dstate, n_seeds) || sc.alloc(&dact, n) || sc.alloc(&deff, eff_bytes) ||
      sc.alloc(&dpicks, picks.size()) || sc.alloc(&dtodo, n_seeds))
    return -BGV_E_DEVICE;
  HIPCHK(hipMemcpyAsync(dseeds, seeds.data(), sizeof(shuf_seed) * n_seeds, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemsetAsync(dstate, 0, sizeof(samp_state) * n_seeds, d.stream));
  HIPCHK(hipMemcpyAsync(dact, active, 4 * (size_t)n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(deff, eff, eff_bytes, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemsetAsync(dpicks, 0, 4 * picks.size(), d.stream));
  const bgv_sample_in in{dseeds, dstate, dact, n, deff, max_incr, rounds, limit, want, dpicks, rule};
  SampleDev dev{d, sc, in, n_seeds, dtodo};
  if (int rc = samp_run(dev, n_seeds, want, limit, st)) return rc;
  sc.enqueued();
  HIPCHK(hipMemcpyAsync(picks.data(), dpicks, 4 * picks.size(), hipMemcpyDeviceToHost, d.stream));
  return sc.sync();
}

// 96-byte uncompressed G1 record (x | y big-endian, 0x40 for infinity) to the 48 compressed bytes
void g1_compress(uint8_t out48[48], const uint8_t in96[96]) {
  if (in96[0] & 0x40) {
    memset(out48, 0, 48);
    out48[0] = 0xC0;
    return;
  }
  static const uint32_t half[12] = BGV_EXP_P_MINUS_1_DIV_2;  // (p - 1) / 2, little-endian words
  int cmp = 0;  // y against it, from the top byte down
  for (int k = 0; k < 48 && cmp == 0; ++k) {
    const uint8_t h = (uint8_t)(half[11 - k / 4] >> (24 - 8 * (k % 4)));
    cmp = in96[48 + k] > h ? 1 : in96[48 + k] < h ? -1 : 0;
  }
  memcpy(out48, in96, 48);
  out48[0] |= cmp > 0 ? 0xA0 : 0x80;
}

// bgv_proposers / bgv_proposers_electra: the same call under either rule
int proposers_by_rule(bgv_ctx* c, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active, size_t n_active,
                      const void* eff, size_t n_eff, samp_rule_id rule, uint32_t max_incr, uint32_t rounds,
                      uint32_t* out_proposers) {
  if (!c || !seeds32 || !out_proposers || n_seeds < 1 || n_seeds > BGV_SAMPLE_MAX_SEEDS ||
      !sample_args_ok(active, n_active, eff, n_eff, max_incr, rounds, rule))
    return -BGV_E_ARG;
  const uint32_t limit = samp_limit(n_active, true);
  std::vector<samp_state> st;
  std::vector<uint32_t> picks;
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
    if (c->closed) return -BGV_E_CLOSED;
    if (int rc = sample_run(c, seeds32, n_seeds, active, (uint32_t)n_active, eff, n_eff, rule, max_incr, rounds, 1,
                            limit, st, picks))
      return rc;
  }
  // every candidate rejected: the reference's -1 when that was the whole list, else the cap was hit
  for (uint32_t s = 0; s < n_seeds; ++s)
    if (!st[s].have && n_active > limit) return -BGV_E_ARG;
  for (uint32_t s = 0; s < n_seeds; ++s) out_proposers[s] = st[s].have ? picks[s] : BGV_NO_PROPOSER;
  return BGV_OK;
}

// bgv_sync_committee_put / bgv_sync_committee_put_electra.
// The next sync committee: sampled on the first device, then stored on every device exactly as
// bgv_committee_put stores a list (committee_put_locked: checks, pool range, directory entry,
// k_committee_total).  put_mu is held throughout, so neither the cache nor the id changes between
// the sampling and the store; the aggregate is read through bgv_aggregate_committee_bits once
// the committee exists, and the id is dropped again should that fail.
int sync_committee_put_by_rule(bgv_ctx* c, uint32_t id, const uint8_t seed[32], const uint32_t* active,
                               size_t n_active, const void* eff, size_t n_eff, samp_rule_id rule, uint32_t max_incr,
                               uint32_t size, uint32_t rounds, uint32_t* out_indices, uint8_t out_agg48[48]) {
  if (!c || !seed || id >= BGV_MAX_COMMITTEES || size < 1 || size > BGV_SAMPLE_MAX_WANT ||
      !sample_args_ok(active, n_active, eff, n_eff, max_incr, rounds, rule))
    return -BGV_E_ARG;
  std::lock_guard<std::mutex> plk(c->put_mu);
  std::vector<samp_state> st;
  std::vector<uint32_t> picks;
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    if (c->closed) return -BGV_E_CLOSED;
    {
      std::shared_lock<std::shared_mutex> lk(c->com_mu);
      if (c->committees.count(id)) return -BGV_E_ARG;
    }
    const size_t npk = c->n_pubkeys;
    const bool marks = !c->bad_pk.empty();
    for (size_t i = 0; i < n_active; ++i)
      if (active[i] >= npk || (marks && c->bad_pk.count(active[i]))) return -BGV_E_BAD_INDEX;
    if (int rc = sample_run(c, seed, 1, active, (uint32_t)n_active, eff, n_eff, rule, max_incr, rounds, size,
                            samp_limit(n_active, false), st, picks))
      return rc;
    if (st[0].have < size) return -BGV_E_ARG;  // the cap
  }
  if (int rc = committee_put_locked(c, id, picks.data(), size)) return rc;
  if (out_agg48) {
    const std::vector<uint8_t> bits = [&] {
      std::vector<uint8_t> b((size + 7) / 8, 0xff);
      if (size % 8) b.back() = (uint8_t)((1u << (size % 8)) - 1u);
      return b;
    }();
    uint8_t agg96[96];
    if (int rc = bgv_aggregate_committee_bits(c, id, bits.data(), size, agg96)) {
      (void)committee_drop_locked(c, id);
      return rc;
    }
    g1_compress(out_agg48, agg96);
  }
  if (out_indices) memcpy(out_indices, picks.data(), 4 * (size_t)size);
  return BGV_OK;
}
}  // namespace

extern "C" {

int bgv_proposers(bgv_ctx* c, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active, size_t n_active,
                  const uint8_t* eff, size_t n_eff, uint32_t max_incr, uint32_t rounds, uint32_t* out_proposers) {
  return proposers_by_rule(c, seeds32, n_seeds, active, n_active, eff, n_eff, SAMP_RULE_BYTE, max_incr, rounds,
                           out_proposers);
}
int bgv_proposers_electra(bgv_ctx* c, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active,
                          size_t n_active, const uint16_t* eff16, size_t n_eff, uint32_t max_incr, uint32_t rounds,
                          uint32_t* out_proposers) {
  return proposers_by_rule(c, seeds32, n_seeds, active, n_active, eff16, n_eff, SAMP_RULE_U16, max_incr, rounds,
                           out_proposers);
}
int bgv_sync_committee_put(bgv_ctx* c, uint32_t id, const uint8_t seed[32], const uint32_t* active, size_t n_active,
                           const uint8_t* eff, size_t n_eff, uint32_t max_incr, uint32_t size, uint32_t rounds,
                           uint32_t* out_indices, uint8_t out_agg48[48]) {
  return sync_committee_put_by_rule(c, id, seed, active, n_active, eff, n_eff, SAMP_RULE_BYTE, max_incr, size, rounds,
                                    out_indices, out_agg48);
}
int bgv_sync_committee_put_electra(bgv_ctx* c, uint32_t id, const uint8_t seed[32], const uint32_t* active,
                                   size_t n_active, const uint16_t* eff16, size_t n_eff, uint32_t max_incr,
                                   uint32_t size, uint32_t rounds, uint32_t* out_indices, uint8_t out_agg48[48]) {
  return sync_committee_put_by_rule(c, id, seed, active, n_active, eff16, n_eff, SAMP_RULE_U16, max_incr, size,
                                    rounds, out_indices, out_agg48);
}

namespace {
// One device's staged entries (bgv_pubkeys_put): drained and freed with that device current.
struct StagedScope : DevScope<> {
  int dev;
  uint8_t* entries = nullptr;
  explicit StagedScope(const Device& d) : DevScope<>(d.stream), dev(d.id) {}
  ~StagedScope() { (void)hipSetDevice(dev); }
};
}  // namespace

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
  std::vector<int32_t> status(n, 0);
  std::deque<StagedScope> staged;  // per device: the decoded entries, until they are committed
  {
    std::shared_lock<std::shared_mutex> clk(c->cache_mu);
    if (c->closed) return -BGV_E_CLOSED;
    if ((size_t)first > c->n_pubkeys) return -BGV_E_ARG;  // append or overwrite, no holes
    if (n == 0) return BGV_OK;
    std::lock_guard<std::mutex> ulk(c->util_mu);
    for (size_t di = 0; di < c->devs.size(); ++di) {
      Device& d = c->devs[di];
      StagedScope& stg = staged.emplace_back(d);
      HIPCHK(hipSetDevice(d.id));
      if (int rc = stg.alloc(&stg.entries, esz * n)) return rc;
      // zeroed: k_cache_put writes no entry for an undecodable record
      HIPCHK(hipMemsetAsync(stg.entries, 0, esz * n, d.stream));
      const size_t chunk = 1 << 20;
      DevScope<> tmp(d.stream);
      uint8_t* dk = nullptr;
      int32_t* dst = nullptr;
      if (tmp.alloc(&dk, (size_t)fmt * std::min(n, chunk) + 1) || tmp.alloc(&dst, std::min(n, chunk) + 1))
        return -BGV_E_DEVICE;
      for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        tmp.enqueued();  // the previous chunk's synchronize left the scope drained
        bgv_cache_entry* out = reinterpret_cast<bgv_cache_entry*>(stg.entries + esz * off);
        HIPCHK(hipMemcpyAsync(dk, keys + (size_t)fmt * off, (size_t)fmt * m, hipMemcpyHostToDevice, d.stream));
        HIPCHK(bgv_launch_cache_put(dk, (uint32_t)m, fmt, out, dst, d.stream));
        if (di == 0) HIPCHK(hipMemcpyAsync(status.data() + off, dst, 4 * m, hipMemcpyDeviceToHost, d.stream));
        if (int rc = tmp.sync()) return rc;
      }
      stg.drained();  // by tmp's last synchronize: n > 0, so there was one
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
      staged[di].enqueued();
      HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(d.cache) + esz * first, staged[di].entries, esz * n,
                            hipMemcpyDeviceToDevice, d.stream));
      if (int rc = staged[di].sync()) return rc;
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
        staged[di].enqueued();
        for (uint32_t i : bad)
          if (rc == BGV_OK && i < old_n &&
              hipMemcpyAsync(staged[di].entries + esz * (i - first),
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
  if (rc) return rc;
  return first_err ? -first_err : BGV_OK;
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
    DevScope<> sc(d.stream);
    uint8_t *dsk = nullptr, *dout = nullptr;
    if (sc.alloc(&dsk, 32 * n) || sc.alloc(&dout, 48 * n)) return -BGV_E_DEVICE;
    HIPCHK(hipMemcpyAsync(dsk, sks, 32 * n, hipMemcpyHostToDevice, d.stream));
    bgv_cache_entry* dst =
        cache_first >= 0 ? reinterpret_cast<bgv_cache_entry*>(reinterpret_cast<uint8_t*>(d.cache) + esz * cache_first)
                         : nullptr;
    HIPCHK(bgv_launch_keygen(dsk, (uint32_t)n, dst, dout, d.stream));
    if (out48 && di == 0) HIPCHK(hipMemcpyAsync(out48, dout, 48 * n, hipMemcpyDeviceToHost, d.stream));
    if (int rc = sc.sync()) return rc;
  }
  if (cache_first >= 0) {
    const size_t old_n = c->n_pubkeys.load();
    for (size_t i = 0; i < n; ++i) c->bad_pk.erase((uint32_t)(cache_first + i));
    c->n_pubkeys.store(std::max(old_n, (size_t)cache_first + n));
    if ((size_t)cache_first < old_n) return committees_refresh(c, (uint32_t)cache_first, n);
  }
  return BGV_OK;
}

}  // extern "C"
