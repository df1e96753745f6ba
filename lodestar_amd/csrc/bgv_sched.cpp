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
#include <sys/mman.h>
#include <sys/random.h>

#include "bgv_ctx.h"
#include "bls_field.h"  // fp12_t (sizes of the per-group u copies)

extern "C" int bgv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
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

int exec_reserve_slots(Exec& x, uint32_t slots) {
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

int exec_reserve_groups(Exec& x, uint32_t groups) {
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
int exec_reserve_lines(Exec& x, bgv_dev_batch& b) { return exec_reserve_line_pairs(x, b, bgv_lines_pairs(b)); }
int exec_reserve_line_pairs(Exec& x, bgv_dev_batch& b, uint32_t need) {
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

int exec_create(Exec* x) {
  HIPCHK(hipEventCreate(&x->ev0));
  HIPCHK(hipEventCreate(&x->ev1));
  HIPCHK(hipEventCreateWithFlags(&x->ev_sets, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&x->ev_prep, hipEventDisableTiming));
  for (auto& e : x->kev) HIPCHK(hipEventCreate(&e));
  return BGV_OK;
}

void exec_destroy(Exec* x) {
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
    if (hipEventElapsedTime(&km, x.kev[2 * k], x.kev[2 * k + 1]) == hipSuccess)
      c->kernel_ms[k] += km;
    else
      // A failed query stays this thread's last error, and the next launch check on the thread
      // (hipGetLastError in bgv_launch_prep) would fail a later call with it.
      (void)hipGetLastError();
  }
  if (sets) c->kernel_launches++;
}

bgv_dev_batch make_batch(Device& d, Exec& x, uint32_t nslots, uint32_t ngroups) {
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

void fp12_one_bytes(uint8_t out[576]) {
  memset(out, 0, 576);
  out[47] = 1;  // c0.c0.c0 = 1, big-endian
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
// A committee set (pk.is_com(i)) is checked against the live committee of its id
// (committee_set_check), a span set against every committee of its list (span_set_check); with a call, what the layout needs of it goes to
// call->setcom and the call takes a reference to the committee.  The caller holds com_mu (shared)
// when pkbits is given.
int host_job_code(bgv_ctx* c, const bgv_job& jb, const bgv_set* sets, int32_t* code, PkForm pk, Call* call) {
  *code = 2;
  if (jb.n_sets == 0) {
    *code = -BGV_E_EMPTY_SET;
    return BGV_OK;
  }
  for (uint32_t k = 0; k < jb.n_sets && *code == 2; ++k) {
    const bgv_set& s = sets[jb.first_set + k];
    if (pk.spans && pk.is_com(jb.first_set + k)) {
      const bgv_pkspan& sp = pk.spans[jb.first_set + k];
      if (!s.msg || (!s.sig && s.sig_len) || !sp.committees || (!sp.bits && sp.n_bits)) return -BGV_E_ARG;
      std::vector<std::shared_ptr<CommitteeRec>> recs;  // the listed committees, once each
      SetCommittee sc;
      *code = span_set_check(
          [&](uint32_t id, CommitteeInfo* ci) {
            const auto it = c->committees.find(id);
            if (it == c->committees.end()) return false;
            *ci = CommitteeInfo{it->second->handle, (uint32_t)it->second->idx.size(), it->second->bad};
            if (call && (recs.empty() || recs.back() != it->second)) recs.push_back(it->second);
            return true;
          },
          sp, &sc);
      if (*code == 2 && call) {
        call->setcom[jb.first_set + k] = std::move(sc);
        call->com_refs.insert(call->com_refs.end(), recs.begin(), recs.end());
      }
      continue;
    }
    if (pk.bits && pk.is_com(jb.first_set + k)) {
      const bgv_pkbits& pb = pk.bits[jb.first_set + k];
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
                       PkForm pkbits = PkForm()) {
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
  const auto is_com = [pkbits](size_t i) { return pkbits.is_com(i); };
  // pass-1 layout (bgv_host_layout.h)
  Layout& L = call->L;
  {
    size_t npk = 0;
    for (size_t i = 0; i < nsets; ++i)
      if (is_com(i))  // the handle and the bit words (a refused set: n = 0); a span's run has its header
                      // and at most two words per bit word and three per committee
        npk += PKB_SPAN_HEAD + (call->setcom[i].parts.empty() ? 1 : 2) * pkb_nwords(call->setcom[i].n) +
               3 * call->setcom[i].parts.size();
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
  size_t nidx = 0, npkb = 0, nuniq = 0, ncom_team = 0, ncom_wave = 0, nspan_team = 0, nspan_wave = 0;
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
    nspan_team += call->L.span_team.size();
    nspan_wave += call->L.span_wave.size();
    for (char u : call->L.group_uniform) any_uniform = any_uniform || u;
  }
  const size_t ncom = ncom_team + ncom_wave, nspan = nspan_team + nspan_wave;
  const size_t nlist = nuniq + ncom + nspan;  // the lists after the indices
  const bool bulk = nslots + ngroups > bgv_fold_pairs_max();
  // uniform groups (BGV_GROUP_UNIFORM): bulk batches (the two-phase Miller stage)
  const bool uniform = uniform_enabled() && any_uniform && bulk;
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
    for (Call* call : calls)
      for (uint32_t v : call->L.span_team) *u++ = v + call->slot_base;
    for (Call* call : calls)
      for (uint32_t v : call->L.span_wave) *u++ = v + call->slot_base;
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
  bs.bulk = bgv_lines_pairs(b) != 0;
  b.uniq = x.d_idx + nidx;
  b.nuniq = (uint32_t)nuniq;
  b.com = x.d_idx + nidx + nuniq;
  b.ncom_team = (uint32_t)ncom_team;
  b.ncom_wave = (uint32_t)ncom_wave;
  b.span = b.com + ncom;
  b.nspan_team = (uint32_t)nspan_team;
  b.nspan_wave = (uint32_t)nspan_wave;
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
  // after a bulk first pass without uniform groups the round's signature pairs read line records
  // (bgv_launch_gpairs); the first pass's records are dead, and this thread holds the Exec
  if (bs.bulk && !b.uniform && (rc = exec_reserve_line_pairs(x, b, nrg))) return rc;
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
      sigagg_free(d);
      sigpool_free(d);
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
  // every verify call has finished: what still waits for its aggregation ends here
  sigagg_stop(c);
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
// One job's sets -> its Fp12 Miller-loop product and status codes on device dev (-1: any).
static int partial_submit(bgv_ctx* c, Call* call, const bgv_set* sets, size_t nsets, uint8_t* out576,
                          int32_t* out_codes, int dev, PkForm pkbits = PkForm()) {
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
                        PkForm pkbits, int mode, int32_t* out, bgv_stats* stats) {
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
                              pkbits.from(jobs[j].first_set + lo));
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

static int verify_sync(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, PkForm pkbits,
                       int mode, int32_t* out, bgv_stats* stats);
static int verify_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                        PkForm pkbits, int mode, int32_t* out, bgv_stats* stats, bgv_done_fn done, void* user);

int bgv_verify(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, int mode,
               int32_t* out, bgv_stats* stats) {
  return verify_sync(c, jobs, njobs, sets, nsets, PkForm(), mode, out, stats);
}

int bgv_verify_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, int mode,
                     int32_t* out, bgv_stats* stats, bgv_done_fn done, void* user) {
  return verify_async(c, jobs, njobs, sets, nsets, PkForm(), mode, out, stats, done, user);
}

// pkbits: how the sets name their pubkeys (bgv_verify, bgv_verify_bits, bgv_verify_spans)
static int verify_sync(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, PkForm pkbits,
                       int mode, int32_t* out, bgv_stats* stats) {
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

static int verify_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                        PkForm pkbits, int mode, int32_t* out, bgv_stats* stats, bgv_done_fn done, void* user) {
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

int bgv_verify_bits(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                    const bgv_pkbits* pkbits, int mode, int32_t* out, bgv_stats* stats) {
  return verify_sync(c, jobs, njobs, sets, nsets, PkForm(pkbits), mode, out, stats);
}

int bgv_verify_bits_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                          const bgv_pkbits* pkbits, int mode, int32_t* out, bgv_stats* stats, bgv_done_fn done,
                          void* user) {
  return verify_async(c, jobs, njobs, sets, nsets, PkForm(pkbits), mode, out, stats, done, user);
}

int bgv_verify_spans(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                     const bgv_pkspan* spans, int mode, int32_t* out, bgv_stats* stats) {
  return verify_sync(c, jobs, njobs, sets, nsets, PkForm(spans), mode, out, stats);
}

int bgv_verify_spans_async(bgv_ctx* c, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                           const bgv_pkspan* spans, int mode, int32_t* out, bgv_stats* stats, bgv_done_fn done,
                           void* user) {
  return verify_async(c, jobs, njobs, sets, nsets, PkForm(spans), mode, out, stats, done, user);
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

}  // extern "C"
