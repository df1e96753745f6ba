// libblsgpu: device-resident signature pools.  The registry (which ids are live, their
// generations, counts and participation bits), the accumulation step of bgv_verify_accumulate and
// bgv_verify_accumulate_bits, bgv_sigpool_get and bgv_sigpool_sum, all on device 0's utility stream
// under util_mu (bgv_sigpool_plan.h, bgv_sigpool_bits_plan.h, bgv_k_sigpool.hip).  The verdicts
// come from the verify path as it is, as bgv_verify_aggregate's do (bgv_sigagg.cpp), and the
// asynchronous form goes through the same aggregation worker.
#include "bgv_ctx.h"
#include "bgv_sigpool_bits_plan.h"

// pool_mu held
static SigPoolView pool_view(bgv_ctx* c) {
  if (c->pool_live.empty()) {
    c->pool_live.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_written.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_gen.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_count.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_nbits.assign(BGV_MAX_SIGPOOL, 0);
  }
  return SigPoolView{c->pool_live.data(), c->pool_gen.data()};
}

// pool_mu held.  pool_bits is allocated by the first bgv_sigpool_open_bits: NULL until then.
static SigPoolBitsView pool_bits_view(bgv_ctx* c) {
  pool_view(c);
  return SigPoolBitsView{c->pool_live.data(), c->pool_gen.data(), c->pool_nbits.data(),
                         c->pool_bits.empty() ? nullptr : c->pool_bits.data()};
}

void sigpool_free(Device& d) {
  SigPoolDev& s = d.sigpool;
  void* bufs[] = {s.d_acc, s.d_meta, s.d_flag, s.d_gids, s.d_gout, s.d_sids, s.d_sfc, s.d_sout};
  for (void* q : bufs)
    if (q) (void)hipFree(q);
  s.h_meta.release();
  s.h_gids.release();
  s.h_flag.release();
  s.h_gout.release();
  s.h_sids.release();
  s.h_sfc.release();
  s.h_sout.release();
  s = SigPoolDev{};
}

// util_mu held, device 0 current
static int sigpool_reserve_step(SigPoolDev& s, size_t nentries) {
  if (nentries > s.cap) {
    void* bufs[] = {s.d_meta, s.d_flag};
    for (void* q : bufs)
      if (q) (void)hipFree(q);
    s.d_meta = nullptr;
    s.d_flag = nullptr;
    const size_t cap = std::max<size_t>(std::max(nentries, 2 * s.cap), 16);
    s.cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_meta), 16 * cap));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_flag), 4 * cap));
    s.cap = cap;
  }
  HIPCHK(s.h_meta.reserve(4 * nentries));
  HIPCHK(s.h_flag.reserve(nentries));
  return BGV_OK;
}

static int sigpool_reserve_get(SigPoolDev& s, size_t n) {
  if (n > s.get_cap) {
    void* bufs[] = {s.d_gids, s.d_gout};
    for (void* q : bufs)
      if (q) (void)hipFree(q);
    s.d_gids = nullptr;
    s.d_gout = nullptr;
    const size_t cap = std::max<size_t>(std::max(n, 2 * s.get_cap), 16);
    s.get_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_gids), 4 * cap));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_gout), 96 * cap));
    s.get_cap = cap;
  }
  HIPCHK(s.h_gids.reserve(n));
  HIPCHK(s.h_gout.reserve(96 * n));
  return BGV_OK;
}

// bgv_sigpool_sum: nids ids in all, ngroups groups for the device
static int sigpool_reserve_sum(SigPoolDev& s, size_t nids, size_t ngroups) {
  if (int rc = grow(&s.d_sids, &s.sid_cap, nids)) return rc;
  if (ngroups > s.sum_cap) {
    void* bufs[] = {s.d_sfc, s.d_sout};
    for (void* q : bufs)
      if (q) (void)hipFree(q);
    s.d_sfc = nullptr;
    s.d_sout = nullptr;
    const size_t cap = std::max<size_t>(std::max(ngroups, 2 * s.sum_cap), 16);
    s.sum_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_sfc), 8 * cap));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_sout), 96 * cap));
    s.sum_cap = cap;
  }
  HIPCHK(s.h_sids.reserve(nids));
  HIPCHK(s.h_sfc.reserve(2 * ngroups));
  HIPCHK(s.h_sout.reserve(96 * ngroups));
  return BGV_OK;
}

// The accumulation step of one call whose codes are final.  Writes out_added (the outcomes, for a
// call with fields), or nothing when it fails.
static int sigpool_run(const SigAggTask& t) {
  bgv_ctx* c = t.c;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  std::lock_guard<std::mutex> lk(c->util_mu);  // one step at a time, and none beside a get or a drop
  SigPoolBitsPlan bp;  // a call without fields uses its plan alone
  SigPoolPlan& plan = bp.plan;
  std::vector<uint32_t> fresh;
  {
    std::lock_guard<std::mutex> pl(c->pool_mu);
    if (t.fields)
      sigpool_plan_bits(t.jobs, t.njobs, t.codes, t.agg_of_set, t.gen_of_set.data(), t.nsets, pool_bits_view(c),
                        *t.fields, sigagg_wave_max(), &bp);
    else
      sigpool_plan(t.jobs, t.njobs, t.codes, t.agg_of_set, t.gen_of_set.data(), t.nsets, pool_view(c),
                   sigagg_wave_max(), &plan);
    for (uint32_t id : plan.ids) fresh.push_back(c->pool_written[id] ? 0u : 1u);
  }
  const size_t n = plan.member.size(), ne = plan.ids.size();
  if (n == 0) {  // nothing to add: no device work
    if (t.out_added && t.fields)
      memcpy(t.out_added, bp.outcome.data(), t.nsets);  // known and overlapping members are still told
    else if (t.out_added)
      memset(t.out_added, 0, t.nsets);
    return BGV_OK;
  }
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  SigAggScratch& s = d.sigagg;
  SigPoolDev& p = d.sigpool;
  if (!p.d_acc) return -BGV_E_DEVICE;  // a live entry implies the array (bgv_sigpool_open)
  if (int rc = sigagg_reserve(s, n, 0)) return rc;
  if (int rc = sigpool_reserve_step(p, ne)) return rc;
  // a signature whose length the caller changed since the verdict does not decode
  for (size_t k = 0; k < n; ++k) {
    const bgv_set& st = t.sets[plan.member[k]];
    if (st.sig_len == 96 && st.sig)
      memcpy(s.h_sigs.p + 96 * k, st.sig, 96);
    else
      memset(s.h_sigs.p + 96 * k, 0, 96);  // no compression flag: BLST_BAD_ENCODING on the device
  }
  memcpy(p.h_meta.p, plan.ids.data(), 4 * ne);
  memcpy(p.h_meta.p + ne, plan.first.data(), 4 * ne);
  memcpy(p.h_meta.p + 2 * ne, plan.count.data(), 4 * ne);
  memcpy(p.h_meta.p + 3 * ne, fresh.data(), 4 * ne);
  DevScope<> sc(d.stream);
  sc.enqueued();  // the stream reads and writes the pinned staging: drained on every path
  HIPCHK(hipMemcpyAsync(s.d_sigs, s.h_sigs.p, 96 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(p.d_meta, p.h_meta.p, 16 * ne, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_sigagg_decode(s.d_sigs, (uint32_t)n, plan.form == SIGAGG_FORM_WAVE, s.d_pts, s.d_st, d.stream));
  HIPCHK(bgv_launch_sigpool_acc(p.d_meta, p.d_meta + ne, p.d_meta + 2 * ne, p.d_meta + 3 * ne, (uint32_t)ne, s.d_pts,
                                s.d_st, p.d_acc, p.d_flag, d.stream));
  ++c->sigpool_launches[plan.form == SIGAGG_FORM_WAVE ? 0 : 1];
  HIPCHK(hipMemcpyAsync(p.h_flag.p, p.d_flag, 4 * ne, hipMemcpyDeviceToHost, d.stream));
  if (int rc = sc.sync()) return rc;
  std::lock_guard<std::mutex> pl(c->pool_mu);
  if (t.fields) {  // nothing changed since the plan: util_mu
    sigpool_commit_bits(&bp, p.h_flag.p, t.agg_of_set, t.nsets, c->pool_written.data(), c->pool_count.data(),
                        c->pool_bits.data());
    if (t.out_added) memcpy(t.out_added, bp.outcome.data(), t.nsets);
    return BGV_OK;
  }
  if (t.out_added) memset(t.out_added, 0, t.nsets);
  for (size_t e = 0; e < ne; ++e) {
    if (p.h_flag.p[e] != BGV_OK) continue;  // a member no longer decodes: the device left the entry as it was
    const uint32_t id = plan.ids[e];
    c->pool_written[id] = 1;
    c->pool_count[id] += plan.count[e];
    if (t.out_added)
      for (uint32_t k = 0; k < plan.count[e]; ++k) t.out_added[plan.member[plan.first[e] + k]] = 1;
  }
  return BGV_OK;
}

// null context, closed context, then the tags against the registry as it stands now
// Then, with fields (bgv_verify_accumulate_bits), bits_of_set against the entries that have bits;
// without, a tag on such an entry is -BGV_E_ARG.
static int sigpool_submit_check(bgv_ctx* c, const uint32_t* pool_of_set, size_t nsets,
                                std::vector<uint32_t>* gen_of_set, const bgv_poolbits* bits_of_set = nullptr,
                                SigPoolFields* fields = nullptr) {
  if (!c) return -BGV_E_ARG;
  if (c->closed) return -BGV_E_CLOSED;
  std::lock_guard<std::mutex> pl(c->pool_mu);
  if (int rc = sigpool_check_tags(pool_of_set, nsets, pool_view(c), gen_of_set)) return rc;
  if (fields) return sigpool_check_bits(pool_of_set, bits_of_set, nsets, pool_bits_view(c), fields);
  for (size_t i = 0; i < nsets; ++i)
    if (pool_of_set[i] != BGV_NO_AGG && c->pool_nbits[pool_of_set[i]]) return -BGV_E_ARG;
  return BGV_OK;
}

// bgv_sigpool_open (n_bits 0) and bgv_sigpool_open_bits
static int sigpool_open_entry(bgv_ctx* c, uint32_t id, uint32_t n_bits) {
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  if (!d.sigpool.d_acc) {
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(hipMalloc(&d.sigpool.d_acc, bgv_g2_point_bytes() * (size_t)BGV_MAX_SIGPOOL));
  }
  std::lock_guard<std::mutex> pl(c->pool_mu);
  pool_view(c);
  if (c->pool_live[id]) return -BGV_E_ARG;
  if (n_bits && c->pool_bits.empty()) c->pool_bits.assign((size_t)BGV_MAX_SIGPOOL * BGV_SIGPOOL_BITS_BYTES, 0);
  c->pool_live[id] = 1;
  c->pool_written[id] = 0;  // the first accumulation starts from infinity
  c->pool_count[id] = 0;
  c->pool_nbits[id] = n_bits;  // the field is clear: bgv_sigpool_drop_range
  ++c->pool_gen[id];
  return BGV_OK;
}

// bgv_sigpool_get, and with out_bits / out_nbits bgv_sigpool_get_bits
static int sigpool_get_entries(bgv_ctx* c, const uint32_t* ids, size_t n, uint8_t* out96, uint32_t* out_count,
                               int32_t* out_status, uint8_t* out_bits, uint32_t* out_nbits) {
  std::lock_guard<std::mutex> lk(c->util_mu);
  std::vector<int32_t> status(n);
  std::vector<uint32_t> counts(n, 0), nbits(n, 0), at;  // at: the requests the device answers
  std::vector<uint8_t> fields(out_bits ? n * BGV_SIGPOOL_BITS_BYTES : 0, 0);
  {
    std::lock_guard<std::mutex> pl(c->pool_mu);
    pool_view(c);
    for (size_t k = 0; k < n; ++k) {
      const uint32_t id = ids[k];
      status[k] = !c->pool_live[id] ? -BGV_E_BAD_INDEX : c->pool_count[id] == 0 ? -BGV_E_EMPTY_AGGREGATE : BGV_OK;
      if (status[k] == BGV_OK) {
        counts[k] = c->pool_count[id];
        at.push_back((uint32_t)k);
      }
      if (out_bits && c->pool_live[id] && c->pool_nbits[id]) {
        nbits[k] = c->pool_nbits[id];
        memcpy(fields.data() + BGV_SIGPOOL_BITS_BYTES * k, c->pool_bits.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * id,
               BGV_SIGPOOL_BITS_BYTES);
      }
    }
  }
  const size_t m = at.size();
  Device& d = c->devs[0];
  SigPoolDev& p = d.sigpool;
  if (m) {
    HIPCHK(hipSetDevice(d.id));
    if (!p.d_acc) return -BGV_E_DEVICE;
    if (int rc = sigpool_reserve_get(p, m)) return rc;
    for (size_t q = 0; q < m; ++q) p.h_gids.p[q] = ids[at[q]];
    DevScope<> sc(d.stream);
    sc.enqueued();
    HIPCHK(hipMemcpyAsync(p.d_gids, p.h_gids.p, 4 * m, hipMemcpyHostToDevice, d.stream));
    HIPCHK(bgv_launch_sigpool_get(p.d_gids, (uint32_t)m, p.d_acc, p.d_gout, d.stream));
    HIPCHK(hipMemcpyAsync(p.h_gout.p, p.d_gout, 96 * m, hipMemcpyDeviceToHost, d.stream));
    if (int rc = sc.sync()) return rc;
  }
  memset(out96, 0, 96 * n);
  for (size_t q = 0; q < m; ++q) memcpy(out96 + 96 * (size_t)at[q], p.h_gout.p + 96 * q, 96);
  memcpy(out_count, counts.data(), 4 * n);
  memcpy(out_status, status.data(), 4 * n);
  if (out_bits) {
    memcpy(out_bits, fields.data(), fields.size());
    memcpy(out_nbits, nbits.data(), 4 * n);
  }
  return BGV_OK;
}

extern "C" {

int bgv_debug_sigpool_launches(bgv_ctx* c, uint64_t out[2]) {
  if (!c || !out) return -BGV_E_ARG;
  if (c->closed) return -BGV_E_CLOSED;
  out[0] = c->sigpool_launches[0];
  out[1] = c->sigpool_launches[1];
  return BGV_OK;
}

int bgv_sigpool_open(bgv_ctx* c, uint32_t id) {
  if (!c) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  if (id >= BGV_MAX_SIGPOOL) return -BGV_E_ARG;
  return sigpool_open_entry(c, id, 0);
}

int bgv_sigpool_open_bits(bgv_ctx* c, uint32_t id, uint32_t n_bits) {
  if (!c) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  if (id >= BGV_MAX_SIGPOOL || n_bits == 0 || n_bits > BGV_SIGPOOL_MAX_BITS) return -BGV_E_ARG;
  return sigpool_open_entry(c, id, n_bits);
}

int bgv_sigpool_drop_range(bgv_ctx* c, uint32_t first_id, uint32_t count) {
  if (!c) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  std::lock_guard<std::mutex> lk(c->util_mu);  // not beside a step
  std::lock_guard<std::mutex> pl(c->pool_mu);
  pool_view(c);
  int dropped = 0;
  const uint64_t end = std::min<uint64_t>((uint64_t)first_id + count, BGV_MAX_SIGPOOL);
  for (uint64_t id = first_id; id < end; ++id)
    if (c->pool_live[id]) {
      c->pool_live[id] = 0;
      c->pool_count[id] = 0;
      if (c->pool_nbits[id]) memset(c->pool_bits.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * id, 0, BGV_SIGPOOL_BITS_BYTES);
      c->pool_nbits[id] = 0;
      ++dropped;
    }
  return dropped;
}

int bgv_sigpool_get(bgv_ctx* c, const uint32_t* ids, size_t n, uint8_t* out96, uint32_t* out_count,
                    int32_t* out_status) {
  if (!c) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  if (!ids || !out96 || !out_count || !out_status) return -BGV_E_ARG;
  for (size_t k = 0; k < n; ++k)
    if (ids[k] >= BGV_MAX_SIGPOOL) return -BGV_E_ARG;
  return sigpool_get_entries(c, ids, n, out96, out_count, out_status, nullptr, nullptr);
}

int bgv_sigpool_get_bits(bgv_ctx* c, const uint32_t* ids, size_t n, uint8_t* out96, uint32_t* out_count,
                         int32_t* out_status, uint8_t* out_bits, uint32_t* out_nbits) {
  if (!c) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  if (!ids || !out96 || !out_count || !out_status || !out_bits || !out_nbits) return -BGV_E_ARG;
  for (size_t k = 0; k < n; ++k)
    if (ids[k] >= BGV_MAX_SIGPOOL) return -BGV_E_ARG;
  return sigpool_get_entries(c, ids, n, out96, out_count, out_status, out_bits, out_nbits);
}

int bgv_sigpool_sum(bgv_ctx* c, const bgv_poolgroup* groups, size_t ngroups, uint8_t* out96, uint32_t* out_count,
                    int32_t* out_status, uint8_t* out_bits, size_t bits_stride, uint32_t* out_nbits) {
  if (!c) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  if (ngroups == 0) return BGV_OK;
  if (ngroups > 65536 || !groups || !out96 || !out_count || !out_status || !out_nbits) return -BGV_E_ARG;
  for (size_t g = 0; g < ngroups; ++g) {
    if (groups[g].n_ids == 0 || groups[g].n_ids > BGV_MAX_SUM_ENTRIES || !groups[g].ids) return -BGV_E_ARG;
    for (uint32_t k = 0; k < groups[g].n_ids; ++k)
      if (groups[g].ids[k] >= BGV_MAX_SIGPOOL) return -BGV_E_ARG;
  }
  std::lock_guard<std::mutex> lk(c->util_mu);
  std::vector<int32_t> status(ngroups);
  std::vector<uint32_t> counts(ngroups, 0), nbits(ngroups, 0), at;  // at: the groups the device answers
  std::vector<uint32_t> sids, sfirst, scount;                        // their written entries
  std::vector<size_t> bits_at(ngroups, 0);                           // where a group's field starts in fields
  std::vector<uint8_t> fields;
  {
    std::lock_guard<std::mutex> pl(c->pool_mu);
    pool_view(c);
    for (size_t g = 0; g < ngroups; ++g) {
      const bgv_poolgroup& gr = groups[g];
      bool live = true;
      uint64_t cnt = 0;
      uint32_t nb = 0;
      for (uint32_t k = 0; k < gr.n_ids; ++k) {
        live = live && c->pool_live[gr.ids[k]];
        cnt += c->pool_count[gr.ids[k]];
        nb += c->pool_nbits[gr.ids[k]];
      }
      if (!live) {
        status[g] = -BGV_E_BAD_INDEX;
        continue;
      }
      if (out_bits && sigpool_bits_bytes(nb) > bits_stride) return -BGV_E_ARG;
      counts[g] = (uint32_t)std::min<uint64_t>(cnt, 0xFFFFFFFFu);
      nbits[g] = nb;
      status[g] = cnt == 0 ? -BGV_E_EMPTY_AGGREGATE : BGV_OK;
      if (out_bits) {
        bits_at[g] = fields.size();
        fields.resize(fields.size() + sigpool_bits_bytes(nb), 0);
        size_t off = 0;
        for (uint32_t k = 0; k < gr.n_ids; ++k) {
          const uint32_t id = gr.ids[k], n = c->pool_nbits[id];
          if (!n) continue;
          sigpool_append_bits(fields.data() + bits_at[g], off, c->pool_bits.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * id, n);
          off += n;
        }
      }
      if (cnt == 0) continue;
      // an entry that is open and empty, or open again after a drop, has a slot that holds stale
      // data: only written ones go to the device
      sfirst.push_back((uint32_t)sids.size());
      for (uint32_t k = 0; k < gr.n_ids; ++k)
        if (c->pool_written[gr.ids[k]]) sids.push_back(gr.ids[k]);
      scount.push_back((uint32_t)sids.size() - sfirst.back());
      at.push_back((uint32_t)g);
    }
  }
  const size_t m = at.size(), ni = sids.size();
  Device& d = c->devs[0];
  SigPoolDev& p = d.sigpool;
  if (m) {
    HIPCHK(hipSetDevice(d.id));
    if (!p.d_acc) return -BGV_E_DEVICE;
    if (int rc = sigpool_reserve_sum(p, ni, m)) return rc;
    memcpy(p.h_sids.p, sids.data(), 4 * ni);
    memcpy(p.h_sfc.p, sfirst.data(), 4 * m);
    memcpy(p.h_sfc.p + m, scount.data(), 4 * m);
    DevScope<> sc(d.stream);
    sc.enqueued();
    HIPCHK(hipMemcpyAsync(p.d_sids, p.h_sids.p, 4 * ni, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(p.d_sfc, p.h_sfc.p, 8 * m, hipMemcpyHostToDevice, d.stream));
    HIPCHK(bgv_launch_sigpool_sum(p.d_sids, p.d_sfc, p.d_sfc + m, (uint32_t)m, p.d_acc, p.d_sout, d.stream));
    HIPCHK(hipMemcpyAsync(p.h_sout.p, p.d_sout, 96 * m, hipMemcpyDeviceToHost, d.stream));
    if (int rc = sc.sync()) return rc;
  }
  memset(out96, 0, 96 * ngroups);
  for (size_t q = 0; q < m; ++q) memcpy(out96 + 96 * (size_t)at[q], p.h_sout.p + 96 * q, 96);
  memcpy(out_count, counts.data(), 4 * ngroups);
  memcpy(out_status, status.data(), 4 * ngroups);
  memcpy(out_nbits, nbits.data(), 4 * ngroups);
  if (out_bits)
    for (size_t g = 0; g < ngroups; ++g) {
      memset(out_bits + g * bits_stride, 0, bits_stride);
      if (nbits[g]) memcpy(out_bits + g * bits_stride, fields.data() + bits_at[g], sigpool_bits_bytes(nbits[g]));
    }
  return BGV_OK;
}

int bgv_verify_accumulate(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                          const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set, int32_t* out,
                          uint8_t* out_added, bgv_stats* stats) {
  if (!pool_of_set) return bgv_verify_spans(c, jobs, njobs, sets, nsets, spans, mode, out, stats);
  SigAggTask t;
  if (int rc = sigpool_submit_check(c, pool_of_set, nsets, &t.gen_of_set)) return rc;
  t.t0 = std::chrono::steady_clock::now();
  int rc = bgv_verify_spans(c, jobs, njobs, sets, nsets, spans, mode, out, stats);
  if (rc != BGV_OK) return rc;
  t.c = c;
  t.jobs = jobs;
  t.njobs = njobs;
  t.sets = sets;
  t.nsets = nsets;
  t.agg_of_set = pool_of_set;
  t.codes = out;
  t.out_added = out_added;
  rc = sigpool_run(t);
  if (stats)
    stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t.t0).count();
  return rc;
}

int bgv_verify_accumulate_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                                const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set, int32_t* out,
                                uint8_t* out_added, bgv_stats* stats, bgv_done_fn done, void* user) {
  if (!pool_of_set) return bgv_verify_spans_async(c, jobs, njobs, sets, nsets, spans, mode, out, stats, done, user);
  std::vector<uint32_t> gens;
  if (int rc = sigpool_submit_check(c, pool_of_set, nsets, &gens)) return rc;
  if (!done) return -BGV_E_ARG;  // nobody to tell of the additions
  if (int rc = sigagg_worker_start(c)) return rc;
  SigAggTask* t = new SigAggTask();
  t->t0 = std::chrono::steady_clock::now();
  t->c = c;
  t->jobs = jobs;
  t->njobs = njobs;
  t->sets = sets;
  t->nsets = nsets;
  t->agg_of_set = pool_of_set;
  t->codes = out;
  t->out_added = out_added;
  t->gen_of_set.swap(gens);
  t->step = sigpool_run;
  t->stats = stats;
  t->done = done;
  t->user = user;
  const int rc = bgv_verify_spans_async(c, jobs, njobs, sets, nsets, spans, mode, out, stats, sigagg_verify_done, t);
  if (rc != BGV_OK) delete t;
  return rc;
}

int bgv_verify_accumulate_bits(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                               const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set,
                               const bgv_poolbits* bits_of_set, int32_t* out, uint8_t* out_outcome, bgv_stats* stats) {
  if (!pool_of_set) return bgv_verify_spans(c, jobs, njobs, sets, nsets, spans, mode, out, stats);
  SigAggTask t;
  t.fields = std::make_shared<SigPoolFields>();
  if (int rc = sigpool_submit_check(c, pool_of_set, nsets, &t.gen_of_set, bits_of_set, t.fields.get())) return rc;
  t.t0 = std::chrono::steady_clock::now();
  int rc = bgv_verify_spans(c, jobs, njobs, sets, nsets, spans, mode, out, stats);
  if (rc != BGV_OK) return rc;
  t.c = c;
  t.jobs = jobs;
  t.njobs = njobs;
  t.sets = sets;
  t.nsets = nsets;
  t.agg_of_set = pool_of_set;
  t.codes = out;
  t.out_added = out_outcome;
  rc = sigpool_run(t);
  if (stats)
    stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t.t0).count();
  return rc;
}

int bgv_verify_accumulate_bits_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                                     const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set,
                                     const bgv_poolbits* bits_of_set, int32_t* out, uint8_t* out_outcome,
                                     bgv_stats* stats, bgv_done_fn done, void* user) {
  if (!pool_of_set) return bgv_verify_spans_async(c, jobs, njobs, sets, nsets, spans, mode, out, stats, done, user);
  std::vector<uint32_t> gens;
  std::shared_ptr<SigPoolFields> fields = std::make_shared<SigPoolFields>();
  if (int rc = sigpool_submit_check(c, pool_of_set, nsets, &gens, bits_of_set, fields.get())) return rc;
  if (!done) return -BGV_E_ARG;  // nobody to tell of the outcomes
  if (int rc = sigagg_worker_start(c)) return rc;
  SigAggTask* t = new SigAggTask();
  t->t0 = std::chrono::steady_clock::now();
  t->c = c;
  t->jobs = jobs;
  t->njobs = njobs;
  t->sets = sets;
  t->nsets = nsets;
  t->agg_of_set = pool_of_set;
  t->codes = out;
  t->out_added = out_outcome;
  t->gen_of_set.swap(gens);
  t->fields.swap(fields);
  t->step = sigpool_run;
  t->stats = stats;
  t->done = done;
  t->user = user;
  const int rc = bgv_verify_spans_async(c, jobs, njobs, sets, nsets, spans, mode, out, stats, sigagg_verify_done, t);
  if (rc != BGV_OK) delete t;
  return rc;
}

}  // extern "C"
