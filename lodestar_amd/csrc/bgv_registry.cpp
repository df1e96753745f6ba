// libblsgpu: the device-resident registries: the pubkey cache, committees, epoch shuffling and keygen.
#include "bgv_ctx.h"
#include "bgv_shuffle.h"  // the committee bounds of an epoch shuffling (bgv_shuffling_put)

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
