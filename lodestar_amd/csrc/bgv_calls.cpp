// libblsgpu: the one-shot utility calls and the debug hooks the GPU tests lean on.
#include "bgv_ctx.h"

extern "C" {

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
  std::vector<int32_t> st(m);
  int32_t v = 0;
  DevScope<> sc(d.stream);
  sc.enqueued();  // the stream reads in and g and writes st and v: drained on every path
  HIPCHK(hipMemcpyAsync(fs.din, in.data(), 576 * m, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(fs.dg, &g, sizeof(g), hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_final_verify(fs.din, (uint32_t)m, fs.vals, fs.one, fs.dg, fs.dst, fs.dv, d.stream));
  HIPCHK(hipMemcpyAsync(st.data(), fs.dst, 4 * m, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(&v, fs.dv, 4, hipMemcpyDeviceToHost, d.stream));
  if (int rc = sc.sync()) return rc;
  for (int32_t x : st)
    if (x) return -BGV_E_ARG;  // a coefficient >= p: not a serialized partial
  *out_verdict = v;
  return BGV_OK;
}

namespace {
// An Exec with a private non-blocking stream, like the dispatchers' (not the legacy null stream):
// the debug hooks run the verify path's launchers on it.
struct PrivateExec {
  Exec* x = new Exec();
  hipStream_t stream = nullptr;
  int rc;
  PrivateExec() : rc(exec_create(x)) {
    if (!rc && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) rc = -BGV_E_DEVICE;
    x->main = stream;
  }
  ~PrivateExec() {
    exec_destroy(x);  // synchronizes x->main first
    if (stream) (void)hipStreamDestroy(stream);
  }
};
}  // namespace

// The cached-key slots of a debug hook's sets, padded to a wave; slot i's randomizer is the i-th
// nonzero splitmix64 word of seed (tools/gen_golden_r04.py draws them in the same order).
// uniform (bgv_debug_uniform): every set carries a 96-byte signature over the first set's root,
// in group 0 with hsrc 0.  Otherwise (bgv_debug_prepare): groups of 64 consecutive slots, every
// slot hashes its own root, and a signature of length 0 passes.  Per set, in set order: argument
// errors before BGV_E_BAD_INDEX.  The caller holds cache_mu.
static int debug_slots(bgv_ctx* c, const bgv_set* sets, size_t nsets, uint64_t seed, bool uniform,
                       std::vector<bgv_dslot>& slots, std::vector<uint32_t>& idx, uint32_t* max_npk) {
  uint64_t state = seed;
  *max_npk = 0;
  for (size_t i = 0; i < nsets; ++i) {
    const bgv_set& st = sets[i];
    if (!st.pk_indices || st.n_pk == 0 || !st.msg || (st.sig_len && !st.sig)) return -BGV_E_ARG;
    if (uniform && (st.sig_len != 96 || memcmp(st.msg, sets[0].msg, 32) != 0)) return -BGV_E_ARG;
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
    s.group = uniform ? 0u : (uint32_t)(i / BGV_WAVE);
    s.hsrc = uniform ? 0u : (uint32_t)i;
    do s.scalar = splitmix64(&state);
    while (s.scalar == 0);
    *max_npk = std::max(*max_npk, st.n_pk);
    slots.push_back(s);
  }
  while (slots.size() % BGV_WAVE) {
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.flags = BGV_SLOT_PAD;
    s.hsrc = (uint32_t)slots.size();
    slots.push_back(s);
  }
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
  uint32_t max_npk = 0;
  int rc = debug_slots(c, sets, nsets, seed, false, slots, idx, &max_npk);
  if (rc) return rc;
  for (size_t g = 0; g * BGV_WAVE < nsets; ++g)
    groups.push_back(bgv_dgroup{(uint32_t)(g * BGV_WAVE), (uint32_t)std::min<size_t>(BGV_WAVE, nsets - g * BGV_WAVE),
                                BGV_ALL_SLOTS});
  const uint32_t nslots = (uint32_t)slots.size(), ngroups = (uint32_t)groups.size();
  std::vector<int32_t> ss(nslots), ps(nslots);
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  PrivateExec px;
  Exec& x = *px.x;
  DevScope<> sc(px.stream);
  uint8_t *dh = nullptr, *df = nullptr;
  if ((rc = px.rc) || (rc = exec_reserve_slots(x, nslots)) || (rc = exec_reserve_groups(x, ngroups)) ||
      (rc = grow(&x.d_idx, &x.idx_cap, idx.size())) || (rc = sc.alloc(&dh, 192ull * nslots)) ||
      (rc = sc.alloc(&df, 576ull * nslots)))
    return rc;
  bgv_dev_batch b = make_batch(d, x, nslots, ngroups);
  b.max_npk = max_npk;
  b.path = path;
  if ((rc = exec_reserve_lines(x, b))) return rc;
  bgv_streams S{x.main, nullptr};
  HIPCHK(hipMemcpyAsync(x.d_slots, slots.data(), sizeof(bgv_dslot) * nslots, hipMemcpyHostToDevice, x.main));
  HIPCHK(hipMemcpyAsync(x.d_groups, groups.data(), sizeof(bgv_dgroup) * ngroups, hipMemcpyHostToDevice, x.main));
  HIPCHK(hipMemcpyAsync(x.d_idx, idx.data(), 4 * idx.size(), hipMemcpyHostToDevice, x.main));
  HIPCHK(bgv_launch_sets(b, S));
  HIPCHK(bgv_launch_debug_out(b, dh, df, x.main));
  HIPCHK(hipMemcpyAsync(out_h192, dh, 192 * nsets, hipMemcpyDeviceToHost, x.main));
  HIPCHK(hipMemcpyAsync(out_f576, df, 576 * nsets, hipMemcpyDeviceToHost, x.main));
  HIPCHK(hipMemcpyAsync(ss.data(), b.sig_status, 4ull * nslots, hipMemcpyDeviceToHost, x.main));
  HIPCHK(hipMemcpyAsync(ps.data(), b.pk_status, 4ull * nslots, hipMemcpyDeviceToHost, x.main));
  if ((rc = sc.sync())) return rc;
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
  uint32_t max_npk = 0;
  int rc = debug_slots(c, sets, nsets, seed, true, slots, idx, &max_npk);
  if (rc) return rc;
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
  PrivateExec px;
  Exec& x = *px.x;
  DevScope<> sc(px.stream);
  uint8_t* dout = nullptr;
  if ((rc = px.rc) || (rc = exec_reserve_slots(x, nslots)) ||
      (rc = exec_reserve_groups(x, std::max<uint32_t>(1, nt + nlist))) ||
      (rc = grow(&x.d_idx, &x.idx_cap, idx.size())) || (rc = sc.alloc(&dout, 576ull * (1 + 2 * nt))))
    return rc;
  bgv_dev_batch b = make_batch(d, x, nslots, 1);
  b.max_npk = max_npk;
  b.path = BGV_PATH_BULK;
  b.uniform = true;
  if ((rc = exec_reserve_lines(x, b))) return rc;
  bgv_streams S{x.main, nullptr};
  HIPCHK(hipMemcpyAsync(x.d_slots, slots.data(), sizeof(bgv_dslot) * nslots, hipMemcpyHostToDevice, x.main));
  HIPCHK(hipMemcpyAsync(x.d_groups, &first, sizeof(bgv_dgroup), hipMemcpyHostToDevice, x.main));
  HIPCHK(hipMemcpyAsync(x.d_idx, idx.data(), 4 * idx.size(), hipMemcpyHostToDevice, x.main));
  HIPCHK(bgv_launch_sets(b, S));
  HIPCHK(bgv_launch_fp12_bytes(b.gpkp, 1, dout, x.main));
  if (nt) {
    // the tests over the first pass's per-slot results (r_i sig_i, r_i pk_i, H)
    bgv_dev_batch t = make_batch(d, x, nslots, nt);
    t.max_npk = max_npk;
    t.path = BGV_PATH_BULK;
    t.uniform = true;
    t.upk = reinterpret_cast<const uint32_t*>(t.groups + nt);
    t.npk = nt;
    t.weighted = weighted;
    HIPCHK(hipMemcpyAsync(x.d_groups, tg.data(), sizeof(bgv_dgroup) * tg.size(), hipMemcpyHostToDevice, x.main));
    HIPCHK(bgv_launch_gpairs(t, x.main));
    HIPCHK(bgv_launch_fp12_bytes(t.gpkp, nt, dout + 576, x.main));
    HIPCHK(bgv_launch_fp12_bytes(t.gpair, nt, dout + 576ull * (1 + nt), x.main));
    HIPCHK(hipMemcpyAsync(out_pk576, dout + 576, 576ull * nt, hipMemcpyDeviceToHost, x.main));
    HIPCHK(hipMemcpyAsync(out_sig576, dout + 576ull * (1 + nt), 576ull * nt, hipMemcpyDeviceToHost, x.main));
  }
  HIPCHK(hipMemcpyAsync(out_first576, dout, 576, hipMemcpyDeviceToHost, x.main));
  return sc.sync();
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
  DevScope<> sc(d.stream);
  uint32_t* di = nullptr;
  uint8_t* dout = nullptr;
  bgv_dslot* ds = nullptr;
  void* dagg = nullptr;
  if (sc.alloc(&di, n) || sc.alloc(&dout, 96) || sc.alloc(&ds, 1) || sc.alloc(&dagg, bgv_g1_point_bytes()))
    return -BGV_E_DEVICE;
  HIPCHK(hipMemcpyAsync(di, idx, 4 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(ds, &s, sizeof(s), hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_aggregate(ds, di, (uint32_t)n, d.cache, dagg, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96, hipMemcpyDeviceToHost, d.stream));
  return sc.sync();
}

// The aggregate of one committee or span set (pk names it for set 0) through the call's own
// checks and layout, then k_pk_agg_bits / k_pk_agg_span and pk_sum
static int aggregate_one(bgv_ctx* c, PkForm pk, uint8_t out96[96]) {
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);
  if (c->closed) return -BGV_E_CLOSED;
  const uint8_t zero[96] = {0};
  bgv_set st{};
  st.sig_len = 96;
  st.msg = zero;
  st.sig = zero;
  const bgv_job jb{0, 1, 0};
  Call call;
  call.setcom.assign(1, SetCommittee{});
  int32_t code = 2;
  {
    std::shared_lock<std::shared_mutex> mlk(c->com_mu);
    if (host_job_code(c, jb, &st, &code, pk, &call) != BGV_OK) return -BGV_E_ARG;
  }
  if (code != 2) return code;
  Layout L;
  std::vector<size_t> todo;
  layout_call(L, todo, &jb, 1, &st, BGV_MODE_PER_JOB, {2}, call.setcom.data());
  const uint32_t list = 0;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  DevScope<> sc(d.stream);
  uint32_t* di = nullptr;
  uint8_t* dout = nullptr;
  bgv_dslot* ds = nullptr;
  void* dagg = nullptr;
  if (sc.alloc(&di, L.idx.size() + 1) || sc.alloc(&dout, 96) || sc.alloc(&ds, 1) ||
      sc.alloc(&dagg, bgv_g1_point_bytes()))
    return -BGV_E_DEVICE;
  HIPCHK(hipMemcpyAsync(di, L.idx.data(), 4 * L.idx.size(), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(di + L.idx.size(), &list, 4, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(ds, L.slots.data(), sizeof(bgv_dslot), hipMemcpyHostToDevice, d.stream));
  const bool span = !(L.span_team.empty() && L.span_wave.empty());
  HIPCHK(bgv_launch_aggregate_bits(ds, di, di + L.idx.size(), !(L.com_team.empty() && L.span_team.empty()), span,
                                   d.com_dir, d.com_pool, d.cache, dagg, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96, hipMemcpyDeviceToHost, d.stream));
  return sc.sync();
}

int bgv_aggregate_committee_bits(bgv_ctx* c, uint32_t id, const uint8_t* bits, uint32_t n_bits, uint8_t out96[96]) {
  if (!c || !out96 || (n_bits && !bits)) return -BGV_E_ARG;
  const bgv_pkbits pb{id, n_bits, bits};
  return aggregate_one(c, PkForm(&pb), out96);
}

int bgv_aggregate_span(bgv_ctx* c, const bgv_pkspan* span, uint8_t out96[96]) {
  if (!c || !out96 || !span || !span->committees || (span->n_bits && !span->bits)) return -BGV_E_ARG;
  if (span->n_committees == 0) return -BGV_E_EMPTY_AGGREGATE;  // names no committee
  return aggregate_one(c, PkForm(span), out96);
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
  DevScope<> sc(d.stream);
  uint8_t *dm = nullptr, *dout = nullptr;
  uint32_t *doff = nullptr, *dlen = nullptr;
  if (sc.alloc(&dm, tot + 1) || sc.alloc(&doff, n) || sc.alloc(&dlen, n) || sc.alloc(&dout, 192 * n))
    return -BGV_E_DEVICE;
  if (tot) HIPCHK(hipMemcpyAsync(dm, msgs, tot, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(doff, offs.data(), 4 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dlen, lens, 4 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_hash(dm, doff, dlen, (uint32_t)n, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out192, dout, 192 * n, hipMemcpyDeviceToHost, d.stream));
  return sc.sync();
}

int bgv_pubkeys_validate(bgv_ctx* c, const uint8_t* keys48, size_t n, int32_t* out_status, uint8_t* out96) {
  if (!c || (n && (!keys48 || !out_status))) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  DevScope<> sc(d.stream);
  uint8_t *dk = nullptr, *dout = nullptr;
  int32_t* dst = nullptr;
  if (sc.alloc(&dk, 48 * n) || sc.alloc(&dout, 96 * n) || sc.alloc(&dst, n)) return -BGV_E_DEVICE;
  HIPCHK(hipMemcpyAsync(dk, keys48, 48 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_pk_validate(dk, (uint32_t)n, dst, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out_status, dst, 4 * n, hipMemcpyDeviceToHost, d.stream));
  if (out96) HIPCHK(hipMemcpyAsync(out96, dout, 96 * n, hipMemcpyDeviceToHost, d.stream));
  if (int rc = sc.sync()) return rc;
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
  DevScope<> sc(d.stream);
  uint8_t *ds = nullptr, *dout = nullptr;
  uint32_t *dl = nullptr, *df = nullptr, *dc = nullptr;
  int32_t* dst = nullptr;
  void* pts = nullptr;
  if (sc.alloc(&ds, 96 * n + 1) || sc.alloc(&dl, n + 1) || sc.alloc(&dst, n + 1) ||
      sc.alloc(&pts, bgv_g2_point_bytes() * n + 1) || sc.alloc(&df, naggs) || sc.alloc(&dc, naggs) ||
      sc.alloc(&dout, 96 * naggs))
    return -BGV_E_DEVICE;
  if (n) {
    HIPCHK(hipMemcpyAsync(ds, sigs96, 96 * n, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(dl, lens, 4 * n, hipMemcpyHostToDevice, d.stream));
  }
  HIPCHK(hipMemcpyAsync(df, first.data(), 4 * naggs, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dc, counts, 4 * naggs, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_sig_aggregate(ds, dl, (uint32_t)n, df, dc, (uint32_t)naggs, pts, dst, dout, d.stream));
  if (n) HIPCHK(hipMemcpyAsync(st.data(), dst, 4 * n, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96 * naggs, hipMemcpyDeviceToHost, d.stream));
  if (int rc = sc.sync()) return rc;
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

int bgv_sign(bgv_ctx* c, const uint8_t* sks, const uint8_t* msgs, size_t n, uint8_t* out96) {
  if (!c || (n && (!sks || !msgs || !out96))) return -BGV_E_ARG;
  std::shared_lock<std::shared_mutex> clk(c->cache_mu);  // bgv_close frees the devices under the exclusive lock
  if (c->closed) return -BGV_E_CLOSED;
  if (n == 0) return BGV_OK;
  std::lock_guard<std::mutex> lk(c->util_mu);
  Device& d = c->devs[0];
  HIPCHK(hipSetDevice(d.id));
  DevScope<> sc(d.stream);
  uint8_t *dsk = nullptr, *dm = nullptr, *dout = nullptr;
  if (sc.alloc(&dsk, 32 * n) || sc.alloc(&dm, 32 * n) || sc.alloc(&dout, 96 * n)) return -BGV_E_DEVICE;
  HIPCHK(hipMemcpyAsync(dsk, sks, 32 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dm, msgs, 32 * n, hipMemcpyHostToDevice, d.stream));
  HIPCHK(bgv_launch_sign(dsk, dm, (uint32_t)n, dout, d.stream));
  HIPCHK(hipMemcpyAsync(out96, dout, 96 * n, hipMemcpyDeviceToHost, d.stream));
  return sc.sync();
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
