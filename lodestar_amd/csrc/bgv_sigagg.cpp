// libblsgpu: bgv_verify_aggregate.  The verdicts come from the verify path as it is
// (bgv_verify_spans / bgv_verify_spans_async: the same submit, super-batches and retry rounds);
// once a call's codes are final, the aggregation step sums the signatures it accepted per
// aggregate on device 0's utility stream (bgv_sigagg_plan.h, bgv_k_sigagg.hip).
#include "bgv_ctx.h"
#include "bgv_sigagg_plan.h"

// accepted signatures up to which a call decodes one per wavefront: the header's value unless
// BGV_SIGAGG_WAVE_MAX is set in the environment (0: always one per lane).  Not env_size, which
// reads an unset variable as 0 when 0 is allowed.
size_t sigagg_wave_max() {
  static const size_t v = [] {
    const char* e = getenv("BGV_SIGAGG_WAVE_MAX");
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : (size_t)BGV_SIGAGG_WAVE_MAX;
  }();
  return v;
}

int sigagg_reserve(SigAggScratch& s, size_t n, size_t naggs) {
  if (n > s.sig_cap) {
    void* bufs[] = {s.d_sigs, s.d_pts, s.d_st};
    for (void* q : bufs)
      if (q) (void)hipFree(q);
    s.d_sigs = nullptr;
    s.d_pts = nullptr;
    s.d_st = nullptr;
    const size_t cap = std::max<size_t>(std::max(n, 2 * s.sig_cap), 64);
    s.sig_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_sigs), 96 * cap));
    HIPCHK(hipMalloc(&s.d_pts, bgv_g2_point_bytes() * cap));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_st), 4 * cap));
    s.sig_cap = cap;
  }
  if (naggs > s.agg_cap) {
    void* bufs[] = {s.d_fc, s.d_out};
    for (void* q : bufs)
      if (q) (void)hipFree(q);
    s.d_fc = nullptr;
    s.d_out = nullptr;
    s.agg_cap = 0;
    const size_t cap = std::max<size_t>(naggs, 16);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_fc), 8 * cap));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s.d_out), 96 * cap));
    s.agg_cap = cap;
  }
  HIPCHK(s.h_sigs.reserve(96 * std::max<size_t>(n, 1)));
  HIPCHK(s.h_st.reserve(std::max<size_t>(n, 1)));
  HIPCHK(s.h_fc.reserve(2 * naggs));
  HIPCHK(s.h_out.reserve(96 * naggs));
  return BGV_OK;
}

void sigagg_free(Device& d) {
  SigAggScratch& s = d.sigagg;
  void* bufs[] = {s.d_sigs, s.d_pts, s.d_st, s.d_fc, s.d_out};
  for (void* q : bufs)
    if (q) (void)hipFree(q);
  s.h_sigs.release();
  s.h_out.release();
  s.h_st.release();
  s.h_fc.release();
  s = SigAggScratch{};
}

// The aggregation step of one call whose codes are final.  Writes the three aggregate outputs,
// or none of them when it fails.
static int sigagg_run(const SigAggTask& t) {
  bgv_ctx* c = t.c;
  if (t.naggs == 0) return BGV_OK;
  SigAggPlan plan;
  sigagg_plan(t.jobs, t.njobs, t.codes, t.agg_of_set, t.nsets, t.naggs, sigagg_wave_max(), &plan);
  const size_t n = plan.member.size(), naggs = t.naggs;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (n) {
    std::lock_guard<std::mutex> lk(c->util_mu);
    Device& d = c->devs[0];
    HIPCHK(hipSetDevice(d.id));
    SigAggScratch& s = d.sigagg;
    if (int rc = sigagg_reserve(s, n, naggs)) return rc;
    // a signature whose length the caller changed since the verdict does not decode
    for (size_t k = 0; k < n; ++k) {
      const bgv_set& st = t.sets[plan.member[k]];
      if (st.sig_len == 96 && st.sig)
        memcpy(s.h_sigs.p + 96 * k, st.sig, 96);
      else
        memset(s.h_sigs.p + 96 * k, 0, 96);  // no compression flag: BLST_BAD_ENCODING, overridden below
    }
    memcpy(s.h_fc.p, plan.first.data(), 4 * naggs);
    memcpy(s.h_fc.p + naggs, plan.count.data(), 4 * naggs);
    DevScope<> sc(d.stream);
    sc.enqueued();  // the stream reads and writes the pinned staging: drained on every path
    HIPCHK(hipMemcpyAsync(s.d_sigs, s.h_sigs.p, 96 * n, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(s.d_fc, s.h_fc.p, 4 * naggs, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(s.d_fc + s.agg_cap, s.h_fc.p + naggs, 4 * naggs, hipMemcpyHostToDevice, d.stream));
    HIPCHK(bgv_launch_sigagg(s.d_sigs, (uint32_t)n, plan.form == SIGAGG_FORM_WAVE, s.d_fc, s.d_fc + s.agg_cap,
                             (uint32_t)naggs, s.d_pts, s.d_st, s.d_out, d.stream));
    ++c->sigagg_launches[plan.form == SIGAGG_FORM_WAVE ? 0 : 1];
    HIPCHK(hipMemcpyAsync(s.h_st.p, s.d_st, 4 * n, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipMemcpyAsync(s.h_out.p, s.d_out, 96 * naggs, hipMemcpyDeviceToHost, d.stream));
    if (int rc = sc.sync()) return rc;
    for (size_t a = 0; a < naggs; ++a) {
      int32_t code = plan.count[a] ? BGV_OK : -BGV_E_EMPTY_AGGREGATE;
      for (uint32_t k = 0; k < plan.count[a] && code == BGV_OK; ++k) {
        const size_t m = plan.first[a] + k;
        if (t.sets[plan.member[m]].sig_len != 96)
          code = -BGV_BLST_INVALID_SIZE;
        else if (s.h_st.p[m] != BGV_OK)
          code = -s.h_st.p[m];
      }
      t.out_status[a] = code;
      t.out_count[a] = plan.count[a];
      if (code == BGV_OK)
        memcpy(t.out96 + 96 * a, s.h_out.p + 96 * a, 96);
      else
        memset(t.out96 + 96 * a, 0, 96);
    }
    return BGV_OK;
  }
  for (size_t a = 0; a < naggs; ++a) {  // nothing accepted: no device work
    t.out_status[a] = -BGV_E_EMPTY_AGGREGATE;
    t.out_count[a] = 0;
  }
  memset(t.out96, 0, 96 * naggs);
  return BGV_OK;
}

static void sigagg_task_end(SigAggTask* t, int rc) {
  if (t->stats)
    t->stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t->t0).count();
  t->done(t->user, rc);
  delete t;
}

static void sigagg_worker_loop(bgv_ctx* c) {
  for (;;) {
    SigAggTask* t = nullptr;
    bool stop;
    {
      std::unique_lock<std::mutex> lk(c->agg_mu);
      c->agg_cv.wait(lk, [c] { return c->agg_stop || !c->agg_q.empty(); });
      if (c->agg_q.empty()) return;
      t = c->agg_q.front();
      c->agg_q.pop_front();
      stop = c->agg_stop;
    }
    // bgv_close ends queued work: the verdicts stand, the aggregates are not written
    sigagg_task_end(t, stop ? -BGV_E_CLOSED : t->step ? t->step(*t) : sigagg_run(*t));
  }
}

// The verify call's done(): on a dispatcher or retry thread (or a split call's own thread), which
// never waits for the device here -- the call goes to the context's aggregation worker.
void sigagg_verify_done(void* user, int rc) {
  SigAggTask* t = static_cast<SigAggTask*>(user);
  bgv_ctx* c = t->c;
  if (rc == BGV_OK) {
    std::lock_guard<std::mutex> lk(c->agg_mu);
    if (c->agg_stop)
      rc = -BGV_E_CLOSED;
    else
      c->agg_q.push_back(t);
  }
  if (rc != BGV_OK) {  // the call failed, or the context is closing: nothing to aggregate
    sigagg_task_end(t, rc);
    return;
  }
  c->agg_cv.notify_one();
}

int sigagg_worker_start(bgv_ctx* c) {
  std::lock_guard<std::mutex> lk(c->agg_mu);
  if (c->agg_stop) return -BGV_E_CLOSED;
  if (!c->agg_worker.joinable()) c->agg_worker = std::thread(sigagg_worker_loop, c);
  return BGV_OK;
}

void sigagg_stop(bgv_ctx* c) {
  {
    std::lock_guard<std::mutex> lk(c->agg_mu);
    c->agg_stop = true;
  }
  c->agg_cv.notify_all();
  if (c->agg_worker.joinable()) c->agg_worker.join();
}

static int sigagg_check_args(bgv_ctx* c, size_t nsets, const uint32_t* agg_of_set, size_t naggs, uint8_t* out96,
                             int32_t* out_status, uint32_t* out_count) {
  if (!c) return -BGV_E_ARG;
  if (naggs && (!out96 || !out_status || !out_count)) return -BGV_E_ARG;
  return sigagg_check_tags(agg_of_set, nsets, naggs);
}

extern "C" {

int bgv_debug_sigagg_launches(bgv_ctx* c, uint64_t out[2]) {
  if (!c || !out) return -BGV_E_ARG;
  out[0] = c->sigagg_launches[0];
  out[1] = c->sigagg_launches[1];
  return BGV_OK;
}

int bgv_verify_aggregate(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                         const bgv_pkspan* spans, int mode, const uint32_t* agg_of_set, size_t naggs, int32_t* out,
                         uint8_t* out_agg96, int32_t* out_agg_status, uint32_t* out_agg_count, bgv_stats* stats) {
  if (int rc = sigagg_check_args(c, nsets, agg_of_set, naggs, out_agg96, out_agg_status, out_agg_count)) return rc;
  SigAggTask t;
  t.t0 = std::chrono::steady_clock::now();
  int rc = bgv_verify_spans(c, jobs, njobs, sets, nsets, spans, mode, out, stats);
  if (rc != BGV_OK || naggs == 0) return rc;
  t.c = c;
  t.jobs = jobs;
  t.njobs = njobs;
  t.sets = sets;
  t.nsets = nsets;
  t.agg_of_set = agg_of_set;
  t.naggs = naggs;
  t.codes = out;
  t.out96 = out_agg96;
  t.out_status = out_agg_status;
  t.out_count = out_agg_count;
  rc = sigagg_run(t);
  if (stats)
    stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t.t0).count();
  return rc;
}

int bgv_verify_aggregate_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                               const bgv_pkspan* spans, int mode, const uint32_t* agg_of_set, size_t naggs,
                               int32_t* out, uint8_t* out_agg96, int32_t* out_agg_status, uint32_t* out_agg_count,
                               bgv_stats* stats, bgv_done_fn done, void* user) {
  if (int rc = sigagg_check_args(c, nsets, agg_of_set, naggs, out_agg96, out_agg_status, out_agg_count)) return rc;
  if (naggs == 0) return bgv_verify_spans_async(c, jobs, njobs, sets, nsets, spans, mode, out, stats, done, user);
  if (!done) return -BGV_E_ARG;  // nobody to tell of the aggregates
  if (int rc = sigagg_worker_start(c)) return rc;
  SigAggTask* t = new SigAggTask();
  t->t0 = std::chrono::steady_clock::now();
  t->c = c;
  t->jobs = jobs;
  t->njobs = njobs;
  t->sets = sets;
  t->nsets = nsets;
  t->agg_of_set = agg_of_set;
  t->naggs = naggs;
  t->codes = out;
  t->out96 = out_agg96;
  t->out_status = out_agg_status;
  t->out_count = out_agg_count;
  t->stats = stats;
  t->done = done;
  t->user = user;
  const int rc = bgv_verify_spans_async(c, jobs, njobs, sets, nsets, spans, mode, out, stats, sigagg_verify_done, t);
  if (rc != BGV_OK) delete t;
  return rc;
}

}  // extern "C"
