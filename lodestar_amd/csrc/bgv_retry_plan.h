// Host-only retry planning of one verify call: from the first pass's statuses and group
// verdicts to per-job codes, through rounds of group tests over the per-set results already on
// the device.  No HIP here: bgv_sched.cpp uploads the bgv_dgroup records a round asks for and
// hands back the verdict words; tests/native/retrysim.cpp does the same with a model of the
// closing kernels.
#pragma once
#include <stdio.h>

#include "bgv_host_layout.h"

namespace {

// parts a failing mixed group is split into per retry round (BGV_RETRY_FANOUT env).
// Group closings are team-parallel and cheap in latency, so bisecting (64 -> 8 -> 1)
// costs an extra round but ~4x fewer final exponentiations than going per job at once.
#define BGV_RETRY_FANOUT 8
inline size_t retry_fanout() {
  static const size_t v = env_size("BGV_RETRY_FANOUT", BGV_RETRY_FANOUT, 2);
  return v;
}
// BGV_WEIGHTED_UNIFORM=0: failing uniform groups take the pattern tests at once (no weighted
// test first; CallPlan::build_parts), for A/B measurements
inline bool weighted_uniform_enabled() {
  static const bool v = [] {
    const char* e = getenv("BGV_WEIGHTED_UNIFORM");
    return !(e && atoi(e) == 0);
  }();
  return v;
}
inline bool trace_on() {
  static const bool v = getenv("BGV_TRACE") != nullptr;
  return v;
}

// Outcome of one job from its slots' statuses (maybeBatch.ts:16-39 + blst semantics):
//   any undecodable / not-in-group signature -> error of the first such set (fromBytes throws)
//   any infinity public key                  -> 1 set: false (core verify), >= 2 sets: BLST_PK_IS_INFINITY
// returns 2 when the verdict depends on the groups.
inline int32_t job_precheck(const std::vector<int32_t>& set_sig, const std::vector<int32_t>& set_pk,
                            const bgv_job& j) {
  for (uint32_t k = 0; k < j.n_sets; ++k) {
    const int32_t s = set_sig[j.first_set + k];
    if (s != BGV_OK && s != BGV_ST_INFINITY) return -s;
  }
  for (uint32_t k = 0; k < j.n_sets; ++k) {
    const int32_t p = set_pk[j.first_set + k];
    if (p == BGV_ST_INFINITY) return j.n_sets >= 2 ? -BGV_BLST_PK_IS_INFINITY : 0;
    if (p != BGV_OK) return -p;  // undecodable uncompressed pubkey record
  }
  return 2;
}

struct Part {  // one retry test: consecutive jobs of one failing unit, and the device groups covering them
  std::vector<size_t> jobs;
  std::vector<uint32_t> groups;  // indices into the round's merged group list
  int pattern = -1;              // pattern test: index into CallPlan::punits (its bit is the part's order)
};

// A failing first-pass group whose jobs all lie inside it (gossip: one-set jobs) is retried
// by pattern tests in ONE round: test S_j = the jobs whose index in the group has bit j set,
// j < ceil(log2 n).  The complement's verdict comes for free: the group's pairing value is
// the product of S_j's and its complement's, so with u = gprod^((p^2+1) 3 (p^4-p^2+1)/r) (the
// pairing value is conj(u)/u, bls_team.h tm_final_exp_u) the complement passes iff
// u_group * conj(u_j) lies in Fp6.  A job inside any passing set is valid; every invalid
// job lies in no passing set, so one remaining candidate is the invalid job, and two or
// more go to the next round (usually as singletons).  k tests per failing group instead of
// fanout-bisection's 8 + 8 over two rounds.
//
// The remaining candidates (two or more invalid jobs: 2^h of them for two jobs whose indices
// differ in h bits) are tested one job per device group in the next round, so a failing
// group is resolved in at most two rounds: a round costs about the same latency whether it
// tests hundreds or thousands of groups, while a second pattern round over the candidates
// need not shrink them (two invalid jobs at the first and last candidate index).
//
// Two invalid jobs i, j (the usual case of a second round) leave as candidates the 2^h jobs
// that agree with both where i and j agree, h = the number of bits D where S_b and its
// complement both failed; the candidates pair up as x, x ^ D.  The next round tests the pairs
// (2^(h-1) tests instead of 2^h single jobs): when exactly one test fails and it is a pair,
// both its jobs are invalid (for b in D, S_b and its complement each hold an invalid job, and
// every invalid job is a candidate of that one pair); a failing single job is invalid; jobs of
// a failing pair next to other failures are tested alone in one more round.
struct PatternUnit {
  enum class Kind { Pattern, Pairs, Weighted };  // pattern tests S_j; pairs and single jobs; one weighted test
  uint32_t group = 0;              // the call's first-pass group
  Kind kind = Kind::Pattern;
  std::vector<size_t> jobs;        // Pattern, Weighted: its jobs in slot order
  std::vector<uint32_t> tests;     // round group index of each test
  std::vector<std::vector<size_t>> test_jobs;  // Pairs: each test's jobs
};
// units from the first pass of at most this many jobs (not pattern-testable) are tested one
// job per device group
static const size_t kSingletonMax = 8;
// A pattern unit whose every index bit failed both ways (every job a candidate) goes to single
// jobs next round, not to pairs.  Measured with the root-aligned layout against pairs for every
// unit with a D (profiles/r06/layout/): mainnet-shaped roots at 1 % corruption 3.58 ->
// 4.52-4.81 M sets/s, the distinct-root headline unchanged (2.65-2.66 vs 2.65-2.72 M).
static const bool kAllBitsSingles = true;

// Jobs a retry round still has to decide, and what is known about them.
struct Unit {
  // what its jobs have been through: nothing yet (from the first pass, or a failed fanout part);
  // a weighted test that named no lone slot; a pattern round; a pairs round
  enum class Stage { Fresh, AfterWeighted, AfterPattern, AfterPairs };
  std::vector<size_t> jobs;
  int group = -1;               // first-pass group the jobs lie in (-1: not known)
  Stage stage = Stage::Fresh;
  std::vector<uint32_t> idx;    // AfterPattern: the candidates' pattern indices
  uint32_t dmask = 0;           // ... and the index bits D of their pairing (0: none)
  bool pattern_tested() const { return stage == Stage::AfterPattern || stage == Stage::AfterPairs; }
};

// The host state of one verify call: its layout, its per-job codes and what its retry rounds
// still have to decide.
struct CallPlan {
  const bgv_job* jobs = nullptr;
  size_t njobs = 0;
  size_t nsets = 0;
  int mode = 0;
  // bgv_verify_partial: the call's Miller-loop product (576 B) and its two status codes
  uint8_t* partial_out = nullptr;
  int32_t* partial_codes = nullptr;
  Layout L;
  std::vector<int32_t> code;  // 2 = pending
  std::vector<size_t> todo;
  std::vector<int32_t> set_sig, set_pk;
  std::vector<Unit> units;                 // pending retry units
  std::vector<Part> parts;
  std::vector<PatternUnit> punits;         // this round's pattern-tested units
  bgv_stats st{};
  uint32_t slot_base = 0;  // offset of this call's slots in the merged batch

  bool shared_job(size_t j) const { return mode == BGV_MODE_WORKER && jobs[j].batchable; }

  Unit& add_unit(std::vector<size_t> unit_jobs, int group, Unit::Stage stage) {
    units.push_back(Unit{std::move(unit_jobs), group, stage, {}, 0});
    return units.back();
  }

  // After pass 1: statuses, verdicts and the retry units of the call.
  void after_pass1(const int32_t* ss, const int32_t* ps, const int32_t* verdict) {
    const uint32_t nslots = (uint32_t)L.slots.size(), ngroups = (uint32_t)L.groups.size();
    for (uint32_t i = 0; i < nslots; ++i)
      if (L.slot_set[i] >= 0) {
        set_sig[L.slot_set[i]] = ss[i];
        set_pk[L.slot_set[i]] = ps[i];
        st.sets_verified++;
      }
    st.device_groups += ngroups;
    if (partial_out) {
      // first signature error and first pubkey condition in set order (the caller combines
      // the shards' codes in rank order, as job_precheck does within one job)
      int32_t sig = 0, pk = 0;
      for (size_t i = 0; i < nsets; ++i) {
        const int32_t a = set_sig[i], q = set_pk[i];
        if (!sig && a != BGV_OK && a != BGV_ST_INFINITY) sig = -a;
        if (!pk && q == BGV_ST_INFINITY) pk = 1;
        if (!pk && q != BGV_OK && q != BGV_ST_INFINITY) pk = -q;
      }
      partial_codes[0] = sig;
      partial_codes[1] = pk;
      for (size_t j : todo) code[j] = 1;
      return;
    }
    std::vector<int> unit_of_group(ngroups, -1);  // the unit of each failing shared group
    for (size_t j : todo) {
      const int32_t pre = job_precheck(set_sig, set_pk, jobs[j]);
      if (pre != 2) {
        code[j] = pre;
        continue;
      }
      bool ok = true;
      int first_bad_shared = -1;
      for (uint32_t g : L.job_groups[j])
        if (!(verdict[g] & 1)) {
          ok = false;
          if (L.group_shared[g] && first_bad_shared < 0) first_bad_shared = (int)g;
        }
      if (first_bad_shared >= 0) {
        if (unit_of_group[first_bad_shared] < 0) {
          unit_of_group[first_bad_shared] = (int)units.size();
          add_unit({}, first_bad_shared, Unit::Stage::Fresh);
        }
        units[unit_of_group[first_bad_shared]].jobs.push_back(j);
      } else {
        code[j] = ok ? 1 : 0;
        if (ok && shared_job(j)) st.batch_sigs_success += jobs[j].n_sets;
      }
    }
    st.batch_retries += units.size();  // one unit per failing shared group
  }

  // A job's slots within its (single) group g, as a device-group mask
  uint64_t job_mask(size_t j, const bgv_dgroup& g) const {
    const uint32_t off = L.job_first_slot[j] - g.first_slot, n = jobs[j].n_sets;
    return (n >= 64 ? ~0ull : ((1ull << n) - 1)) << off;
  }

  // every job of the unit lies in the call's group g alone
  bool unit_in_group(const std::vector<size_t>& uj, int g) const {
    if (g < 0) return false;
    for (size_t j : uj) {
      const auto& jg = L.job_groups[j];
      if (jg.size() != 1 || jg[0] != (uint32_t)g) return false;
    }
    return true;
  }

  // A unit from pass 1 is pattern-testable when its jobs lie only in its group and cover every
  // slot of the group that takes part in the group's product (the others -- sets of jobs that
  // failed their precheck -- contribute 1): then a test S_j and its complement partition the
  // group's product.
  bool pattern_eligible(const Unit& u) const {
    if (u.jobs.size() < 2 || !unit_in_group(u.jobs, u.group)) return false;
    const bgv_dgroup& G = L.groups[u.group];
    uint64_t covered = 0;
    for (size_t j : u.jobs) covered |= job_mask(j, G);
    for (uint32_t k = 0; k < G.n_slots; ++k) {
      if ((covered >> k) & 1) continue;
      const int32_t si = L.slot_set[G.first_slot + k];
      if (si < 0) continue;
      const int32_t a = set_sig[si], q = set_pk[si];
      if ((a == BGV_OK || a == BGV_ST_INFINITY) && q == BGV_OK) return false;  // live, outside the unit
    }
    return true;
  }
  // some pending unit is pattern-testable: the retry rounds need the first pass's u values
  bool any_pattern_eligible() const {
    for (const Unit& u : units)
      if (pattern_eligible(u)) return true;
    return false;
  }

  std::vector<size_t> in_slot_order(std::vector<size_t> uj) const {
    std::sort(uj.begin(), uj.end(), [&](size_t a, size_t b) { return L.job_first_slot[a] < L.job_first_slot[b]; });
    return uj;
  }

  // Group testing for one retry round: split every pending unit into parts.  gb: the call's
  // first group in the batch when the first pass's u values are on the device (pattern tests
  // possible), else -1.
  void build_parts(std::vector<bgv_dgroup>& rg, int64_t gb, bool uniform) {
    // A test inside a uniform first-pass group (whose slots have no own pair f_i) pairs the sum
    // of its slots' r_i pk_i with the group's one H instead: prod_S e(r_i pk_i, H) =
    // e(sum_S r_i pk_i, H), the same pairing value, so the complement verdicts hold too
    auto uflag = [&](uint32_t g) { return uniform && L.group_uniform[g] ? BGV_GROUP_UNIFORM : 0u; };
    // one test over the masked slots of first-pass group g, for pattern unit pu if any
    auto add_test = [&](std::vector<size_t> tj, const bgv_dgroup& g, uint64_t mask, uint32_t ref1, uint32_t flags,
                        PatternUnit* pu) {
      Part part;
      part.jobs = std::move(tj);
      part.groups.push_back((uint32_t)rg.size());
      if (pu) {
        part.pattern = (int)punits.size();
        pu->tests.push_back((uint32_t)rg.size());
      }
      rg.push_back(bgv_dgroup{slot_base + g.first_slot, g.n_slots, mask, ref1, flags});
      parts.push_back(std::move(part));
    };
    parts.clear();
    punits.clear();
    for (const Unit& unit : units) {
      const std::vector<size_t>& u = unit.jobs;
      const int ug = unit.group;
      const bool in_group = unit_in_group(u, ug);
      const bool eligible = gb >= 0 && !unit.pattern_tested() && pattern_eligible(unit);
      const uint32_t ref1 = (uint32_t)(gb + ug + 1);  // eligible: the unit's first-pass group in the batch
      if (eligible && unit.stage == Unit::Stage::Fresh && uflag((uint32_t)ug) && weighted_uniform_enabled()) {
        // a failing uniform group almost always holds ONE invalid slot (a wrong key): one test with
        // slot k weighted by k + 1 names it (BGV_GROUP_WEIGHTED; k_final12 finds w with V^w = W)
        // instead of ~6 pattern tests of two Miller loops each; otherwise the pattern tests follow
        // (Stage::AfterWeighted).  Soundness with two or more invalid slots: write slot k's pairing
        // defect as g^(e_k) in the prime-order group GT (e_k != 0 for an invalid slot; the
        // signatures, hence the e_k, are the attacker's, fixed before the secret randomizers are
        // drawn).  V^w = W means sum_k (k + 1 - w) r_k e_k = 0 (mod r), a linear equation in the
        // secret r_k with a nonzero coefficient on at least one of them; r_k takes 2^64 distinct
        // values mod r, so for one w it holds with probability <= 2^-64, and over the 64 candidate
        // w with <= 64 * 2^-64 per failing group (a match would accept the other invalid jobs).
        PatternUnit pu;
        pu.group = (uint32_t)ug;
        pu.kind = PatternUnit::Kind::Weighted;
        pu.jobs = in_slot_order(u);
        const bgv_dgroup& g = L.groups[ug];
        uint64_t m = 0;
        for (size_t j : pu.jobs) m |= job_mask(j, g);
        add_test(pu.jobs, g, m, ref1, BGV_GROUP_UNIFORM | BGV_GROUP_WEIGHTED, &pu);
        punits.push_back(std::move(pu));
        continue;
      }
      if (eligible) {
        PatternUnit pu;
        pu.group = (uint32_t)ug;
        pu.jobs = in_slot_order(u);
        const bgv_dgroup& g = L.groups[ug];
        const size_t n = pu.jobs.size();
        for (int b = 0; (1ull << b) < n; ++b) {  // S_b: the jobs whose index has bit b set
          uint64_t m = 0;
          std::vector<size_t> tj;
          for (size_t i = 0; i < n; ++i)
            if ((i >> b) & 1) {
              m |= job_mask(pu.jobs[i], g);
              tj.push_back(pu.jobs[i]);
            }
          add_test(std::move(tj), g, m, ref1, uflag(ug), &pu);
        }
        punits.push_back(std::move(pu));
        continue;
      }
      if (in_group && unit.pattern_tested() && unit.dmask && unit.idx.size() == u.size()) {
        // pairs x, x ^ D of a pattern round's candidates (see PatternUnit), single jobs otherwise
        const bgv_dgroup& g = L.groups[ug];
        const uint32_t D = unit.dmask;
        const uint32_t b0 = D & (~D + 1);  // lowest bit of D
        std::unordered_map<uint32_t, size_t> at;
        for (size_t k = 0; k < u.size(); ++k) at[unit.idx[k]] = u[k];
        PatternUnit pu;
        pu.group = (uint32_t)ug;
        pu.kind = PatternUnit::Kind::Pairs;
        for (size_t k = 0; k < u.size(); ++k) {
          const uint32_t x = unit.idx[k];
          const auto partner = at.find(x ^ D);
          if (partner != at.end() && (x & b0)) continue;  // tested with its partner
          std::vector<size_t> tj{u[k]};
          uint64_t m = job_mask(u[k], g);
          if (partner != at.end()) {
            tj.push_back(partner->second);
            m |= job_mask(partner->second, g);
          }
          pu.test_jobs.push_back(tj);
          add_test(std::move(tj), g, m, 0, uflag(ug), &pu);
        }
        punits.push_back(std::move(pu));
        continue;
      }
      if (in_group && (unit.pattern_tested() || u.size() <= kSingletonMax)) {
        // one device group per job, each masked to the job's slots: every verdict in this round
        const bgv_dgroup& g = L.groups[ug];
        for (size_t j : u) add_test({j}, g, job_mask(j, g), 0, uflag(ug), nullptr);
        continue;
      }
      const size_t k = std::min<size_t>(retry_fanout(), u.size());
      for (size_t p = 0; p < k; ++p) {
        Part part;
        const size_t lo = u.size() * p / k, hi = u.size() * (p + 1) / k;
        part.jobs.assign(u.begin() + lo, u.begin() + hi);
        for (size_t q = 0; q < part.jobs.size();) {  // maximal runs of consecutive slots
          const uint32_t first = L.job_first_slot[part.jobs[q]];
          uint32_t n = 0;
          size_t q2 = q;
          while (q2 < part.jobs.size() && L.job_first_slot[part.jobs[q2]] == first + n) {
            n += jobs[part.jobs[q2]].n_sets;
            ++q2;
          }
          // chunks within one first-pass group each, so a chunk of a uniform group takes its flag
          // and its root: bounded by the end of slot s0's own group (with BGV_GROUP_SLOTS < 64 a
          // wave holds several groups) and by the wave
          for (uint32_t off = 0; off < n;) {
            const uint32_t s0 = first + off;
            const bgv_dgroup& g0 = L.groups[L.slots[s0].group];
            const uint32_t len = std::min<uint32_t>(std::min<uint32_t>(n - off, BGV_WAVE - s0 % BGV_WAVE),
                                                    g0.first_slot + g0.n_slots - s0);
            part.groups.push_back((uint32_t)rg.size());
            rg.push_back(bgv_dgroup{slot_base + s0, len, BGV_ALL_SLOTS, 0, uflag(L.slots[s0].group)});
            off += len;
          }
          q = q2;
        }
        parts.push_back(std::move(part));
      }
    }
    units.clear();
  }

  // rv: the round's verdict bits (bgv_layout.h: bit 0 the group passes, bit 1 its pairing value
  // equals its reference's, i.e. the complement passes), indexed as build_parts numbered rg
  void after_round(const int32_t* rv) {
    for (const Part& part : parts) st.device_groups += part.groups.size();
    for (const Part& part : parts) {
      if (part.pattern >= 0) continue;
      bool ok = true;
      for (uint32_t g : part.groups) ok = ok && (rv[g] & 1);
      if (ok || part.jobs.size() == 1) {
        for (size_t j : part.jobs) code[j] = ok ? 1 : 0;
      } else {
        add_unit(part.jobs, -1, Unit::Stage::Fresh);
      }
    }
    for (const PatternUnit& pu : punits) {
      if (pu.kind == PatternUnit::Kind::Weighted) {  // one weighted test: bits 8..15 = w, slot w - 1 the lone invalid one
        const int32_t v = rv[pu.tests[0]];
        const uint32_t w = ((uint32_t)v >> 8) & 0xffu;
        const bgv_dgroup& g = L.groups[pu.group];
        size_t bad = SIZE_MAX;
        if (w >= 1 && w <= g.n_slots)
          for (size_t j : pu.jobs)
            if ((job_mask(j, g) >> (w - 1)) & 1) bad = j;
        if (bad != SIZE_MAX) {
          for (size_t j : pu.jobs) code[j] = j == bad ? 0 : 1;
        } else {  // not a lone invalid slot: the pattern tests next round
          add_unit(pu.jobs, (int)pu.group, Unit::Stage::AfterWeighted);
        }
        continue;
      }
      if (pu.kind == PatternUnit::Kind::Pairs) {  // pairs and single jobs (see PatternUnit)
        std::vector<size_t> failing;
        for (size_t t = 0; t < pu.tests.size(); ++t)
          if (!(rv[pu.tests[t]] & 1)) failing.push_back(t);
        std::vector<size_t> again;
        for (size_t t = 0; t < pu.tests.size(); ++t) {
          const auto& tj = pu.test_jobs[t];
          const bool pass = rv[pu.tests[t]] & 1;
          if (pass || tj.size() == 1 || failing.size() == 1) {
            for (size_t j : tj) code[j] = pass ? 1 : 0;
          } else {
            again.insert(again.end(), tj.begin(), tj.end());
          }
        }
        if (failing.empty())  // never expected (then nothing is in again yet): every job alone
          for (const auto& tj : pu.test_jobs) again.insert(again.end(), tj.begin(), tj.end());
        if (!again.empty()) {
          add_unit(std::move(again), (int)pu.group, Unit::Stage::AfterPairs);
        }
        continue;
      }
      const size_t n = pu.jobs.size(), k = pu.tests.size();
      std::vector<size_t> cand;
      std::vector<uint32_t> idx;  // the candidates' pattern indices
      for (size_t i = 0; i < n; ++i) {
        bool in_passing = false;  // in S_b (bit b of i set) or its complement, and that set passed
        for (size_t b = 0; b < k && !in_passing; ++b) in_passing = (rv[pu.tests[b]] >> (((i >> b) & 1) ? 0 : 1)) & 1;
        if (in_passing) {
          code[pu.jobs[i]] = 1;
        } else {
          cand.push_back(pu.jobs[i]);
          idx.push_back((uint32_t)i);
        }
      }
      if (trace_on()) fprintf(stderr, "[bgv]   pattern unit: %zu jobs, %zu tests, %zu candidates\n", n, k, cand.size());
      if (cand.size() == 1) {
        code[cand[0]] = 0;  // the group failed and every invalid job is a candidate
      } else {
        // two or more invalid jobs (or, never expected, none left: test every job alone); D =
        // the bits where S_b and its complement both failed
        uint32_t D = 0;
        for (size_t b = 0; b < k; ++b)
          if (!(rv[pu.tests[b]] & 1) && !((rv[pu.tests[b]] >> 1) & 1)) D |= 1u << b;
        // every index bit with both S_b and its complement failing (D covers all k bits: every
        // job a candidate) means many invalid jobs (two have all their index bits apart with
        // probability 1/(n-1)): the next round tests them one by one (no D: singles) instead of
        // pairs whose failures would need a third round (kAllBitsSingles)
        const bool all_bits = kAllBitsSingles && k > 0 && D == (k >= 32 ? 0xffffffffu : ((1u << k) - 1u));
        Unit& next = add_unit(cand.empty() ? pu.jobs : cand, (int)pu.group, Unit::Stage::AfterPattern);
        next.dmask = cand.empty() || all_bits ? 0 : D;
        next.idx = std::move(idx);
      }
    }
    parts.clear();
    punits.clear();
  }
};

}  // namespace
