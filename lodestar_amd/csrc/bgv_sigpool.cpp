// libblsgpu: device-resident signature pools.  The registry (which ids are live, their
// generations and counts), the accumulation step of bgv_verify_accumulate and bgv_sigpool_get, all
// on device 0's utility stream under util_mu (bgv_sigpool_plan.h, bgv_k_sigpool.hip).  The verdicts
// come from the verify path as it is, as bgv_verify_aggregate's do (bgv_sigagg.cpp), and the
// asynchronous form goes through the same aggregation worker.
#include "bgv_ctx.h"
#include "bgv_sigpool_plan.h"

// pool_mu held
static SigPoolView pool_view(bgv_ctx* c) {
  if (c->pool_live.empty()) {
    c->pool_live.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_written.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_gen.assign(BGV_MAX_SIGPOOL, 0);
    c->pool_count.assign(BGV_MAX_SIGPOOL, 0);
  }
  return SigPoolView{c->pool_live.data(), c->pool_gen.data()};
}

void sigpool_free(Device& d) {
  SigPoolDev& s = d.sigpool;
  void* bufs[] = {s.d_acc, s.d_meta, s.d_flag, s.d_gids, s.d_gout};
  for (void* q : bufs)
    if (q) (void)hipFree(q);
  s.h_meta.release();
  s.h_gids.release();
  s.h_flag.release();
  s.h_gout.release();
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

// The accumulation step of one call whose codes are final.  Writes out_added, or nothing when it
// fails.
static int sigpool_run(const SigAggTask& t) {
  bgv_ctx* c = t.c;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  std::lock_guard<std::mutex> lk(c->util_mu);  // one step at a time, and none beside a get or a drop
  SigPoolPlan plan;
  std::vector<uint32_t> fresh;
  {
    std::lock_guard<std::mutex> pl(c->pool_mu);
    sigpool_plan(t.jobs, t.njobs, t.codes, t.agg_of_set, t.gen_of_set.data(), t.nsets, pool_view(c), sigagg_wave_max(),
                 &plan);
    for (uint32_t id : plan.ids) fresh.push_back(c->pool_written[id] ? 0u : 1u);
  }
  const size_t n = plan.member.size(), ne = plan.ids.size();
  if (n == 0) {  // nothing to add: no device work
    if (t.out_added) memset(t.out_added, 0, t.nsets);
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
  if (t.out_added) memset(t.out_added, 0, t.nsets);
  std::lock_guard<std::mutex> pl(c->pool_mu);
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
static int sigpool_submit_check(bgv_ctx* c, const uint32_t* pool_of_set, size_t nsets,
                                std::vector<uint32_t>* gen_of_set) {
  if (!c) return -BGV_E_ARG;
  if (c->closed) return -BGV_E_CLOSED;
  std::lock_guard<std::mutex> pl(c->pool_mu);
  return sigpool_check_tags(pool_of_set, nsets, pool_view(c), gen_of_set);
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
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  if (!d.sigpool.d_acc) {
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(hipMalloc(&d.sigpool.d_acc, bgv_g2_point_bytes() * (size_t)BGV_MAX_SIGPOOL));
  }
  std::lock_guard<std::mutex> pl(c->pool_mu);
  pool_view(c);
  if (c->pool_live[id]) return -BGV_E_ARG;
  c->pool_live[id] = 1;
  c->pool_written[id] = 0;  // the first accumulation starts from infinity
  c->pool_count[id] = 0;
  ++c->pool_gen[id];
  return BGV_OK;
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
  std::lock_guard<std::mutex> lk(c->util_mu);
  std::vector<int32_t> status(n);
  std::vector<uint32_t> counts(n, 0), at;  // at: the requests the device answers
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

}  // extern "C"
