// Host-only layout of one verify call: its jobs' sets -> slots and device groups (bgv_layout.h).
// No HIP here: bgv_ctx.h includes it for the library, tests/native/retrysim.cpp for a CPU
// simulation of the layout and the retry planner (bgv_retry_plan.h).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/blsgpu.h"
#include "bgv_layout.h"
#include "bgv_pk_bits.h"

// How a call names its sets' pubkeys beside the sets: a bgv_pkbits per set (bgv_verify_bits), a
// bgv_pkspan per set (bgv_verify_spans), or neither (bgv_verify).
struct PkForm {
  const bgv_pkbits* bits = nullptr;
  const bgv_pkspan* spans = nullptr;
  PkForm() = default;
  PkForm(const bgv_pkbits* b) : bits(b) {}
  PkForm(const bgv_pkspan* s) : spans(s) {}
  explicit operator bool() const { return bits || spans; }
  // set i names committees, not its own pk_indices / pk_bytes
  bool is_com(size_t i) const {
    return bits ? bits[i].committee != BGV_NO_COMMITTEE : spans && spans[i].n_committees != 0;
  }
  PkForm from(size_t i) const {  // for the sets from set i on
    PkForm f;
    f.bits = bits ? bits + i : nullptr;
    f.spans = spans ? spans + i : nullptr;
    return f;
  }
};

namespace {

inline size_t env_size(const char* name, size_t dflt, size_t lo) {
  const char* e = getenv(name);
  long n = e ? atol(e) : 0;
  return n >= (long)lo ? (size_t)n : dflt;
}
// sets per first-pass device group, a power of two <= 64 (BGV_GROUP_SLOTS env).
// Smaller groups fail less often under invalid signatures (fewer retried jobs)
// at the price of more final exponentiations when every set is valid.
#define BGV_GROUP_SLOTS 64
inline uint32_t group_slots() {
  static const uint32_t v = [] {
    size_t n = env_size("BGV_GROUP_SLOTS", BGV_GROUP_SLOTS, 1);
    uint32_t p = 1;
    while (p * 2 <= n && p * 2 <= BGV_WAVE) p *= 2;
    return p;
  }();
  return v;
}
// BGV_UNIFORM=0 turns off uniform groups (BGV_GROUP_UNIFORM: one Miller loop per group whose sets
// share a signing root, and the grouping of a call's batchable one-set jobs by root that makes
// them), for A/B measurements; on by default
inline bool uniform_enabled() {
  static const bool v = [] {
    const char* e = getenv("BGV_UNIFORM");
    return !(e && atoi(e) == 0);
  }();
  return v;
}
// calls with fewer batchable one-set jobs take the latency path: their jobs keep their order
#define BGV_UNIFORM_MIN_JOBS 1024
// A signing root with at least this many one-set jobs starts its own device group (layout_call).
// Measured against roots laid back to back (profiles/r06/layout/): mainnet-shaped roots at 1 %
// corruption 3.58 -> 4.52-4.81 M sets/s and ~3,840 -> ~1,545 retry test groups per 131,072-slot
// super-batch; the distinct-root headline unchanged (2.65-2.66 vs 2.65-2.72 M).
static const size_t kUniformAlignMin = 32;

// fn(lo, hi) over [0, n) in up to 8 host threads when n is large (a 2^20-set call: the
// merge's 168 MB of slot records and 8 MB of getrandom output), else inline
template <class F>
inline void par_ranges(size_t n, F fn) {
  const size_t kMin = size_t(1) << 17;
  const unsigned nt = n >= kMin ? std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
  if (nt <= 1) {
    fn(size_t(0), n);
    return;
  }
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(fn, n * t / nt, n * (t + 1) / nt);
  fn(size_t(0), n / nt);
  for (auto& t : th) t.join();
}

// An allocator whose value-less construct leaves the element uninitialized: resizing a vector of
// slot records then writes nothing (layout_one_job_fast fills every record itself)
template <class T>
struct uninit_alloc : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = uninit_alloc<U>;
  };
  uninit_alloc() = default;
  template <class U>
  uninit_alloc(const uninit_alloc<U>&) {}
  template <class U>
  void construct(U* p) noexcept {
    ::new (static_cast<void*>(p)) U;
  }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
  }
};

// What the host keeps of a live committee for a set's checks (bgv_committee_put): its length,
// its directory handle on the devices, and whether one of its members is a marked key.
struct CommitteeInfo {
  uint32_t handle;
  uint32_t n;
  bool bad;
};
// A set's pubkeys once its bgv_pkbits passed the checks: handle == BGV_NO_COMMITTEE for a set
// that brings its own pk_indices / pk_bytes.
struct SetCommittee {
  uint32_t handle = BGV_NO_COMMITTEE;
  uint32_t n = 0;  // members (= n_bits)
  uint32_t k = 0;  // bits set
  const uint8_t* bits = nullptr;
  // a span over two or more committees (bgv_pkspan): handle, n, k of each, in bitfield order;
  // handle above is then the first one's, n the bitfield's length and k its set bits
  std::vector<pkb_part> parts;
};
// The argument checks of one committee set (blsgpu.h bgv_verify_bits): 2 and *out filled when it
// goes to the device, else the code its job gets.  ci: the live committee of pb.committee, or
// null when the id is unknown or dropped.
inline int32_t committee_set_check(const CommitteeInfo* ci, const bgv_pkbits& pb, SetCommittee* out) {
  if (!ci) return -BGV_E_BAD_INDEX;
  if (pb.n_bits != ci->n) return -BGV_E_ARG;
  const uint32_t nbytes = (pb.n_bits + 7u) / 8u;
  if ((pb.n_bits & 7u) && (pb.bits[nbytes - 1] >> (pb.n_bits & 7u))) return -BGV_E_ARG;
  uint32_t k = 0;
  for (uint32_t i = 0; i < nbytes; ++i) k += (uint32_t)__builtin_popcount(pb.bits[i]);
  if (k == 0) return -BGV_E_EMPTY_AGGREGATE;
  if (ci->bad) return -BGV_E_BAD_INDEX;
  *out = SetCommittee{ci->handle, ci->n, k, pb.bits};
  return 2;
}
// The same for a span set (blsgpu.h bgv_verify_spans), in committee_set_check's order with the
// whole list in place of the one committee.  look(id, &ci): whether committee id is live, and
// then the host's mirror of it.  One listed committee is committee_set_check itself, so such a
// span lays out the very slot bgv_verify_bits does.
template <class Look>
inline int32_t span_set_check(Look look, const bgv_pkspan& sp, SetCommittee* out) {
  CommitteeInfo ci{};
  if (sp.n_committees == 1) {
    const bool live = look(sp.committees[0], &ci);
    return committee_set_check(live ? &ci : nullptr, bgv_pkbits{sp.committees[0], sp.n_bits, sp.bits}, out);
  }
  uint64_t total = 0;
  bool bad = false;
  std::vector<pkb_part> parts;
  parts.reserve(std::min<uint32_t>(sp.n_committees, BGV_MAX_SET_COMMITTEES));
  for (uint32_t c = 0; c < sp.n_committees; ++c) {
    if (!look(sp.committees[c], &ci)) return -BGV_E_BAD_INDEX;
    total += ci.n;
    bad = bad || ci.bad;
    if (c < BGV_MAX_SET_COMMITTEES) parts.push_back(pkb_part{ci.handle, ci.n, 0u});
  }
  if (sp.n_committees > BGV_MAX_SET_COMMITTEES || sp.n_bits > BGV_MAX_SPAN_BITS || sp.n_bits != total)
    return -BGV_E_ARG;
  const uint32_t nbytes = (sp.n_bits + 7u) / 8u;
  if ((sp.n_bits & 7u) && (sp.bits[nbytes - 1] >> (sp.n_bits & 7u))) return -BGV_E_ARG;
  uint32_t k = 0, off = 0;
  for (pkb_part& p : parts) {
    p.k = pkb_span_count(sp.bits, nbytes, off, p.n);
    k += p.k;
    off += p.n;
  }
  if (k == 0) return -BGV_E_EMPTY_AGGREGATE;
  if (bad) return -BGV_E_BAD_INDEX;
  *out = SetCommittee{parts[0].handle, sp.n_bits, k, sp.bits};
  out->parts = std::move(parts);
  return 2;
}

// jobs -> slots/groups of one call
struct Layout {
  std::vector<bgv_dslot, uninit_alloc<bgv_dslot>> slots;
  std::vector<bgv_dgroup> groups;
  std::vector<int32_t> slot_set;  // set index per slot (-1 = pad)
  std::vector<std::vector<uint32_t>> job_groups;
  std::vector<uint32_t> job_first_slot;  // first slot of each laid-out job (its slots are contiguous)
  std::vector<char> group_shared;        // group holds sets of more than one job
  std::vector<char> group_uniform;       // every set of the group shares one signing root and no
                                         // batchable job in it spans groups (BGV_GROUP_UNIFORM in bulk
                                         // batches)
  std::vector<uint32_t> idx;             // concatenated pubkey indices
  std::vector<uint8_t> pkb;              // concatenated 96-B pubkey records
  std::vector<uint32_t> uniq;            // first slot of each distinct signing root (hash_to_G2 once)
  // the committee slots (BGV_SLOT_PK_COMMITTEE) k_pk_agg_bits sums: those whose chosen side has
  // at most BGV_PK_TEAM_MAX terms (a 16-lane team each), and the others (a wave each)
  std::vector<uint32_t> com_team, com_wave;
  // the same for the span slots (BGV_SLOT_PK_SPAN) k_pk_agg_span sums, by the span's term count M
  std::vector<uint32_t> span_team, span_wave;
};

// A call's slot as it stands in a merged super-batch (bgv_sched.cpp run_pass1): after slot_base
// slots, ib words of the index array, pb 96-byte pubkey records and gb groups of earlier calls.
// A committee slot's run (handle and bit words; a span's records, which hold handles and no
// offsets) lies in the index array like a run of indices.
inline bgv_dslot rebase_slot(bgv_dslot s, uint32_t slot_base, uint32_t ib, uint32_t pb, uint32_t gb) {
  s.hsrc += slot_base;
  if (s.flags & (BGV_SLOT_PK_CACHED | BGV_SLOT_PK_COMMITTEE)) s.pk_off += ib;
  if (s.flags & BGV_SLOT_PK_BYTES) s.pk_off += pb;
  if (!(s.flags & BGV_SLOT_PAD)) s.group += gb;
  return s;
}

// Which earlier item (slot) shares an item's signing root: the previous item when it has the
// same root (committees arrive together), else the first item with that root, found by the
// root's first 8 bytes (a SHA-256 output).  A key collision between different roots opens a
// root of its own and only costs one extra hash.
struct RootIndex {
  std::unordered_map<uint64_t, uint32_t> first;
  // The item whose H(msg) item self uses: self itself for a new root.  prev_msg, prev_src: the
  // previous item's root and source (null: no previous item); msg_of(i): the root of item i < self
  template <class MsgOf>
  uint32_t source(uint32_t self, const uint8_t* msg, const uint8_t* prev_msg, uint32_t prev_src, MsgOf msg_of) {
    if (prev_msg && memcmp(prev_msg, msg, 32) == 0) return prev_src;
    uint64_t key;
    memcpy(&key, msg, 8);
    auto it = first.find(key);
    if (it == first.end()) it = first.emplace(key, self).first;
    return it->second != self && memcmp(msg_of(it->second), msg, 32) == 0 ? it->second : self;
  }
};

struct Builder {
  Layout& L;
  bool open = false;  // a group is open for appending
  uint32_t open_group = 0;
  int open_job = -1;
  RootIndex roots;
  explicit Builder(Layout& l) : L(l) {}

  void close_group() { open = false; }
  void new_group() {
    // start at the next wave boundary
    uint32_t first = (uint32_t)L.slots.size();
    const uint32_t gs = group_slots();
    uint32_t aligned = (first + gs - 1) / gs * gs;
    while (L.slots.size() < aligned) pad();
    L.groups.push_back(bgv_dgroup{aligned, 0, BGV_ALL_SLOTS});
    L.group_shared.push_back(0);
    L.group_uniform.push_back(1);
    open_group = (uint32_t)L.groups.size() - 1;
    open = true;
    open_job = -1;
  }
  void pad() {
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.flags = BGV_SLOT_PAD;
    s.hsrc = (uint32_t)L.slots.size();
    L.slots.push_back(s);
    L.slot_set.push_back(-1);
  }
  void pad_to_wave() {
    while (L.slots.size() % BGV_WAVE) pad();
  }
  void add(int job, uint32_t set_index, const bgv_set& st, bool first_of_job, const SetCommittee* sc = nullptr) {
    if (!open || L.groups[open_group].n_slots == group_slots()) new_group();
    bgv_dgroup& g = L.groups[open_group];
    if (open_job >= 0 && open_job != job) L.group_shared[open_group] = 1;
    open_job = job;
    std::vector<uint32_t>& jg = L.job_groups[job];
    if (jg.empty() || jg.back() != open_group) jg.push_back(open_group);
    if (first_of_job) L.job_first_slot[job] = (uint32_t)L.slots.size();
    bgv_dslot s;
    memset(&s, 0, sizeof(s));
    s.n_pk = st.n_pk;
    s.sig_len = st.sig_len;
    s.group = open_group;
    if (sc && !sc->parts.empty()) {
      // the span's run (bgv_pk_bits.h pkb_span_build) in the call's index array
      s.flags = BGV_SLOT_PK_COMMITTEE | BGV_SLOT_PK_SPAN;
      s.n_pk = sc->k;
      s.pk_off = (uint32_t)L.idx.size();
      const uint32_t m = pkb_span_build(sc->parts.data(), (uint32_t)sc->parts.size(), sc->bits, (sc->n + 7u) / 8u,
                                        [&](uint32_t v) { L.idx.push_back(v); });
      (m <= BGV_PK_TEAM_MAX ? L.span_team : L.span_wave).push_back((uint32_t)L.slots.size());
    } else if (sc && sc->handle != BGV_NO_COMMITTEE) {
      // the handle, then the bitfield as 32-bit little-endian words, in the call's index array
      const bool comp = pkb_use_complement(sc->n, sc->k);
      s.flags = BGV_SLOT_PK_COMMITTEE | (comp ? BGV_SLOT_PK_COMPLEMENT : 0u);
      s.n_pk = sc->k;
      s.pk_off = (uint32_t)L.idx.size();
      L.idx.push_back(sc->handle);
      const uint32_t nbytes = (sc->n + 7u) / 8u;
      for (uint32_t w = 0; w < pkb_nwords(sc->n); ++w) {
        uint32_t v = 0;
        for (uint32_t q = 0; q < 4 && 4 * w + q < nbytes; ++q) v |= (uint32_t)sc->bits[4 * w + q] << (8 * q);
        L.idx.push_back(v);
      }
      (pkb_terms(sc->n, sc->k, comp) <= BGV_PK_TEAM_MAX ? L.com_team : L.com_wave).push_back((uint32_t)L.slots.size());
    } else if (st.pk_indices) {
      s.flags = BGV_SLOT_PK_CACHED;
      s.pk_off = (uint32_t)L.idx.size();
      L.idx.insert(L.idx.end(), st.pk_indices, st.pk_indices + st.n_pk);
    } else {
      s.flags = BGV_SLOT_PK_BYTES;
      s.pk_off = (uint32_t)(L.pkb.size() / 96);
      L.pkb.insert(L.pkb.end(), st.pk_bytes, st.pk_bytes + 96ull * st.n_pk);
    }
    memcpy(s.msg, st.msg, 32);
    if (st.sig_len == 96) memcpy(s.sig, st.sig, 96);
    const uint32_t self = (uint32_t)L.slots.size();
    const bgv_dslot* prev = self > 0 && !(L.slots[self - 1].flags & BGV_SLOT_PAD) ? &L.slots[self - 1] : nullptr;
    s.hsrc = roots.source(self, st.msg, prev ? prev->msg : nullptr, prev ? prev->hsrc : 0,
                          [&](uint32_t i) { return L.slots[i].msg; });
    if (s.hsrc == self) L.uniq.push_back(self);
    if (g.n_slots > 0 && L.slots[g.first_slot].hsrc != s.hsrc) L.group_uniform[open_group] = 0;
    L.slots.push_back(s);
    L.slot_set.push_back((int32_t)set_index);
    g.n_slots++;
  }
};

// The layout Builder makes for a call of ONE non-batchable job of cached-key sets (slots in set
// order from slot 0, groups of group_slots() consecutive slots, pads to the wave boundary),
// with the per-slot records filled by several host threads: the config-5 sweep's 2^20-set
// job took ~50 ms on one thread.  false: not such a call (the Builder lays it out).
inline bool layout_one_job_fast(Layout& L, const bgv_job& jb, const bgv_set* sets, const SetCommittee* sc = nullptr) {
  const uint32_t n = jb.n_sets, gs = group_slots();
  const bgv_set* S = sets + jb.first_set;
  if (n < (1u << 17)) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (!S[i].pk_indices || (sc && sc[jb.first_set + i].handle != BGV_NO_COMMITTEE)) return false;
  // signing roots in order, as Builder::add (set i is slot i)
  std::vector<uint32_t> hsrc(n), pk_off(n);
  RootIndex roots;
  uint32_t npk = 0;
  for (uint32_t i = 0; i < n; ++i) {
    pk_off[i] = npk;
    npk += S[i].n_pk;
    hsrc[i] = roots.source(i, S[i].msg, i > 0 ? S[i - 1].msg : nullptr, i > 0 ? hsrc[i - 1] : 0,
                           [&](uint32_t q) { return S[q].msg; });
    if (hsrc[i] == i) L.uniq.push_back(i);
  }
  const uint32_t nslots = (n + BGV_WAVE - 1) / BGV_WAVE * BGV_WAVE, ng = (n + gs - 1) / gs;
  L.slots.resize(nslots);
  L.slot_set.resize(nslots);
  L.idx.resize(npk);
  par_ranges(nslots, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      bgv_dslot& s = L.slots[i];
      memset(&s, 0, sizeof(s));
      if (i >= n) {
        s.flags = BGV_SLOT_PAD;
        s.hsrc = (uint32_t)i;
        L.slot_set[i] = -1;
        continue;
      }
      const bgv_set& st = S[i];
      s.n_pk = st.n_pk;
      s.sig_len = st.sig_len;
      s.group = (uint32_t)(i / gs);
      s.flags = BGV_SLOT_PK_CACHED;
      s.pk_off = pk_off[i];
      memcpy(L.idx.data() + pk_off[i], st.pk_indices, 4ull * st.n_pk);
      memcpy(s.msg, st.msg, 32);
      if (st.sig_len == 96) memcpy(s.sig, st.sig, 96);
      s.hsrc = hsrc[i];
      L.slot_set[i] = (int32_t)(jb.first_set + i);
    }
  });
  L.groups.resize(ng);
  L.group_shared.assign(ng, 0);
  L.group_uniform.assign(ng, 1);
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t f = g * gs, m = std::min(gs, n - f);
    L.groups[g] = bgv_dgroup{f, m, BGV_ALL_SLOTS};
    for (uint32_t k = 1; k < m; ++k)
      if (hsrc[f + k] != hsrc[f]) {
        L.group_uniform[g] = 0;
        break;
      }
  }
  L.job_groups[0].resize(ng);
  for (uint32_t g = 0; g < ng; ++g) L.job_groups[0][g] = g;
  L.job_first_slot[0] = 0;
  return true;
}

// The first-pass layout of one call.  code[j] == 2 marks the jobs that go to the device (the
// others were decided by the host's argument checks); they are listed in todo.  Non-batchable
// jobs own their groups; batchable jobs (worker mode) share.
// sc (may be null): per set, the committee form of its pubkeys (committee_set_check).
inline void layout_call(Layout& L, std::vector<size_t>& todo, const bgv_job* jobs, size_t njobs, const bgv_set* sets,
                        int mode, const std::vector<int32_t>& code, const SetCommittee* sc = nullptr) {
  auto shared_job = [&](size_t j) { return mode == BGV_MODE_WORKER && jobs[j].batchable; };
  L.job_groups.resize(njobs);
  L.job_first_slot.assign(njobs, 0);
  Builder B(L);
  for (size_t j = 0; j < njobs; ++j)
    if (code[j] == 2) todo.push_back(j);
  const bool fast = njobs == 1 && todo.size() == 1 && !shared_job(0) && layout_one_job_fast(L, jobs[0], sets, sc);
  auto add_job = [&](size_t j) {
    for (uint32_t k = 0; k < jobs[j].n_sets; ++k)
      B.add((int)j, jobs[j].first_set + k, sets[jobs[j].first_set + k], k == 0,
            sc ? sc + jobs[j].first_set + k : nullptr);
  };
  for (size_t j : todo) {
    if (shared_job(j) || fast) continue;
    B.close_group();
    add_job(j);
    B.close_group();
  }
  B.close_group();
  // Batchable jobs share groups in any order (verdicts map by job).  One-set jobs go grouped by
  // signing root -- the roots in order of first appearance, each root's jobs in call order -- so
  // that the sets of a root fill whole groups (BGV_GROUP_UNIFORM: one Miller loop for the group;
  // gossip attestations of one committee share a root); then multi-set jobs.
  std::vector<size_t> shared_order;
  std::vector<size_t> breaks;  // positions in shared_order where a new device group starts
  size_t n_one = 0;
  for (size_t j : todo)
    if (shared_job(j) && jobs[j].n_sets == 1) ++n_one;
  if (uniform_enabled() && n_one >= BGV_UNIFORM_MIN_JOBS) {
    std::unordered_map<uint64_t, uint32_t> bucket_of;
    bucket_of.reserve(2 * n_one);
    std::vector<std::vector<size_t>> buckets;
    std::vector<const uint8_t*> broot;
    bool grouped = false;  // some root recurs after another root: the order changes
    uint32_t last = UINT32_MAX;
    for (size_t j : todo) {
      if (!shared_job(j) || jobs[j].n_sets != 1) continue;
      const uint8_t* m = sets[jobs[j].first_set].msg;
      uint64_t key;
      memcpy(&key, m, 8);
      auto it = bucket_of.find(key);
      uint32_t b;
      if (it != bucket_of.end() && memcmp(broot[it->second], m, 32) == 0) {
        b = it->second;
      } else {  // a new root (a key collision between different roots just opens another bucket)
        b = (uint32_t)buckets.size();
        buckets.emplace_back();
        broot.push_back(m);
        if (it == bucket_of.end()) bucket_of.emplace(key, b);
      }
      grouped = grouped || (b != last && !buckets[b].empty());
      last = b;
      buckets[b].push_back(j);
    }
    if (grouped) {
      // A root with at least half a group of jobs starts a group of its own, so its groups stay
      // uniform whatever the roots before it held (a committee one set short -- a corrupted
      // message, a late attestation -- would otherwise shift every later root across a group
      // boundary: both groups mixed, per-slot Miller loops, pattern tests instead of the weighted
      // one); the roots with fewer jobs share mixed groups after them, in order of appearance.
      for (const auto& bk : buckets)
        if (bk.size() >= kUniformAlignMin) {
          breaks.push_back(shared_order.size());
          shared_order.insert(shared_order.end(), bk.begin(), bk.end());
        }
      breaks.push_back(shared_order.size());
      for (const auto& bk : buckets)
        if (bk.size() < kUniformAlignMin) shared_order.insert(shared_order.end(), bk.begin(), bk.end());
      for (size_t j : todo)
        if (shared_job(j) && jobs[j].n_sets != 1) shared_order.push_back(j);
    }
  }
  if (shared_order.empty())  // call order
    for (size_t j : todo)
      if (shared_job(j)) shared_order.push_back(j);
  size_t bi = 0;
  for (size_t q = 0; q < shared_order.size(); ++q) {
    if (bi < breaks.size() && breaks[bi] == q) B.close_group();
    while (bi < breaks.size() && breaks[bi] <= q) ++bi;
    add_job(shared_order[q]);
  }
  B.pad_to_wave();
  // A batchable job over several groups may be retried by fanout over its slots, which needs
  // their own pairs: its groups are not uniform.  A non-batchable job is never retried (its
  // verdict is its groups' AND, CallPlan::after_pass1), so its groups stay uniform where their
  // sets share a root: the config-5 sweep's one 2^20-set job, committee by committee.
  for (size_t j : todo)
    if (L.job_groups[j].size() > 1 && shared_job(j))
      for (uint32_t g : L.job_groups[j]) L.group_uniform[g] = 0;
}

}  // namespace
