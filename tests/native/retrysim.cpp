// CPU simulation of one verify call's host logic: the real layout (bgv_host_layout.h) and the
// real retry planner (bgv_retry_plan.h) driven through the first pass and the retry rounds,
// with the verdict words coming from a model of the closing kernels (bgv_k_final.hip
// verdict_bits, k_final_wident) instead of a device.
//
//   retrysim [scenarios.json]      (stdin without an argument)
//
// The input is a JSON list of scenarios:
//   {"name": str, "mode": 0|1, "seed": int, "uniform": bool, "layout": bool,
//    "jobs": [[n_sets, batchable], ...],           sets are taken in order
//    "sets": [[root, kind, code], ...]}            kind: 0 valid, 1 wrong, 2 undecodable signature
//                                                  (BLST code), 3 infinity signature, 4 infinity pubkey
// or {"name": str, "op": "fast_layout", "n": int}: layout_one_job_fast against Builder.
// One JSON line comes out per scenario: the per-job codes, the number of retry rounds, per
// round the number of device groups and an FNV-1a digest of their bgv_dgroup records, and the
// bgv_stats counters the planner keeps.
//
// The device model: GT is the additive group modulo the prime 2^61 - 1.  A live slot (signature
// status OK or infinity, pubkey status OK) carries a defect d: 0 for a valid set, else a fixed
// nonzero residue drawn from the scenario's seed.  A group's value V is the sum of d over its
// masked live slots, weighted by k + 1 with BGV_GROUP_WEIGHTED.  Bit 0: V == 0.  Bit 1 (a round
// with pattern units, ref1 != 0): V_ref - V == 0.  A weighted test: bits 8..15 hold the first
// w <= n_slots with w V_ref == V, and bit 1 is cleared.  BGV_GROUP_UNIFORM changes no value.
#include <stdio.h>

#include <string>

#include "../../lodestar_amd/csrc/bgv_host_layout.h"
#include "../../lodestar_amd/csrc/bgv_retry_plan.h"

namespace {

const uint64_t kP = (1ull << 61) - 1;
const int kMaxRounds = 16;

[[noreturn]] void die(const std::string& why) {
  fprintf(stderr, "retrysim: %s\n", why.c_str());
  exit(2);
}

uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
uint64_t addm(uint64_t a, uint64_t b) { return (a + b) % kP; }
uint64_t mulm(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % kP); }

// ---- a JSON reader for what the scenarios use: objects, arrays, integers, strings, booleans
struct Json {
  enum Kind { Null, Bool, Int, Str, Arr, Obj } kind = Null;
  int64_t i = 0;
  std::string s;
  std::vector<Json> a;
  std::vector<std::pair<std::string, Json>> o;
  const Json* get(const char* key) const {
    for (const auto& kv : o)
      if (kv.first == key) return &kv.second;
    return nullptr;
  }
  int64_t num(const char* key, int64_t dflt) const {
    const Json* v = get(key);
    return v ? v->i : dflt;
  }
};

struct Reader {
  const std::string& t;
  size_t p = 0;
  explicit Reader(const std::string& text) : t(text) {}
  void ws() {
    while (p < t.size() && (t[p] == ' ' || t[p] == '\n' || t[p] == '\t' || t[p] == '\r')) ++p;
  }
  char peek() {
    ws();
    if (p >= t.size()) die("JSON ends early");
    return t[p];
  }
  void expect(char c) {
    if (peek() != c) die(std::string("JSON: expected '") + c + "' at " + std::to_string(p));
    ++p;
  }
  bool word(const char* w) {
    const size_t n = strlen(w);
    if (t.compare(p, n, w) != 0) return false;
    p += n;
    return true;
  }
  std::string str() {
    expect('"');
    std::string out;
    while (p < t.size() && t[p] != '"') {
      if (t[p] == '\\') die("JSON: escapes are not supported");
      out += t[p++];
    }
    expect('"');
    return out;
  }
  Json value() {
    Json v;
    const char c = peek();
    if (c == '{') {
      v.kind = Json::Obj;
      ++p;
      while (peek() != '}') {
        std::string k = str();
        expect(':');
        v.o.emplace_back(std::move(k), value());
        if (peek() == ',') ++p;
      }
      ++p;
    } else if (c == '[') {
      v.kind = Json::Arr;
      ++p;
      while (peek() != ']') {
        v.a.push_back(value());
        if (peek() == ',') ++p;
      }
      ++p;
    } else if (c == '"') {
      v.kind = Json::Str;
      v.s = str();
    } else if (word("true") || word("false")) {
      v.kind = Json::Bool;
      v.i = t[p - 2] == 'u';
    } else if (word("null")) {
    } else {
      v.kind = Json::Int;
      size_t used = 0;
      v.i = std::stoll(t.substr(p, 24), &used);
      p += used;
    }
    return v;
  }
};

// ---- the sets of a scenario as the library sees them
enum SetKind { kValid = 0, kWrong = 1, kUndecodable = 2, kInfSig = 3, kInfPk = 4 };

struct Sets {
  std::vector<std::vector<uint8_t>> msg;
  std::vector<uint32_t> pk;
  std::vector<uint8_t> sig = std::vector<uint8_t>(96, 0xA5);
  std::vector<bgv_set> rec;
  void add(uint64_t root) {
    // roots that differ by a multiple of 2^32 share their first 8 bytes (the layout's hash key)
    std::vector<uint8_t> m(32);
    for (int q = 0; q < 4; ++q) {
      const uint64_t w = splitmix((q ? root : root & 0xffffffffu) * 4 + q);
      memcpy(m.data() + 8 * q, &w, 8);
    }
    msg.push_back(std::move(m));
  }
  void finish() {
    pk.resize(msg.size());
    for (size_t i = 0; i < msg.size(); ++i) {
      pk[i] = (uint32_t)i;
      rec.push_back(bgv_set{1, 96, &pk[i], nullptr, msg[i].data(), sig.data()});
    }
  }
};

uint64_t fnv(uint64_t h, uint64_t v, int bytes) {
  for (int b = 0; b < bytes; ++b) {
    h ^= (v >> (8 * b)) & 0xff;
    h *= 0x100000001B3ull;
  }
  return h;
}
uint64_t digest(const std::vector<bgv_dgroup>& rg) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (const bgv_dgroup& g : rg) {
    h = fnv(h, g.first_slot, 4);
    h = fnv(h, g.n_slots, 4);
    h = fnv(h, g.mask, 8);
    h = fnv(h, g.ref1, 4);
    h = fnv(h, g.flags, 4);
  }
  return h;
}

void print_list(const char* key, const std::vector<int64_t>& v) {
  printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)v[i]);
  printf("]");
}

void run_scenario(const Json& sc) {
  const std::string name = sc.get("name") ? sc.get("name")->s : "";
  const Json *jj = sc.get("jobs"), *js = sc.get("sets");
  if (!jj || !js) die(name + ": jobs and sets are required");
  const uint64_t seed = (uint64_t)sc.num("seed", 1);
  std::vector<bgv_job> jobs;
  uint32_t at = 0;
  for (const Json& j : jj->a) {
    if (j.a.size() != 2) die(name + ": a job is [n_sets, batchable]");
    jobs.push_back(bgv_job{at, (uint32_t)j.a[0].i, (uint32_t)j.a[1].i});
    at += (uint32_t)j.a[0].i;
  }
  const size_t nsets = js->a.size();
  if (at != nsets) die(name + ": the jobs' set counts do not add up to the sets");
  Sets S;
  std::vector<int> kind(nsets), bcode(nsets);
  std::vector<int64_t> root(nsets);
  for (size_t i = 0; i < nsets; ++i) {
    const Json& s = js->a[i];
    if (s.a.size() != 3) die(name + ": a set is [root, kind, code]");
    root[i] = s.a[0].i;
    kind[i] = (int)s.a[1].i;
    bcode[i] = (int)s.a[2].i;
    S.add((uint64_t)root[i]);
  }
  S.finish();

  CallPlan plan;
  plan.jobs = jobs.data();
  plan.njobs = jobs.size();
  plan.nsets = nsets;
  plan.mode = (int)sc.num("mode", BGV_MODE_WORKER);
  plan.code.assign(jobs.size(), 2);
  for (size_t j = 0; j < jobs.size(); ++j)
    if (jobs[j].n_sets == 0) plan.code[j] = -BGV_E_EMPTY_SET;  // the host's argument check
  layout_call(plan.L, plan.todo, jobs.data(), jobs.size(), S.rec.data(), plan.mode, plan.code);
  plan.set_sig.assign(nsets, 0);
  plan.set_pk.assign(nsets, 0);
  const Layout& L = plan.L;
  const uint32_t nslots = (uint32_t)L.slots.size(), ngroups = (uint32_t)L.groups.size();
  if (nslots % BGV_WAVE) die(name + ": the layout does not end on a wave boundary");

  // the device's per-slot results
  std::vector<int32_t> ss(nslots, 0), ps(nslots, 0);
  std::vector<char> live(nslots, 0);
  std::vector<uint64_t> defect(nslots, 0);
  for (uint32_t i = 0; i < nslots; ++i) {
    const int32_t si = L.slot_set[i];
    if (si < 0) continue;
    if (kind[si] == kUndecodable) ss[i] = bcode[si];
    if (kind[si] == kInfSig) ss[i] = BGV_ST_INFINITY;
    if (kind[si] == kInfPk) ps[i] = BGV_ST_INFINITY;
    live[i] = (ss[i] == BGV_OK || ss[i] == BGV_ST_INFINITY) && ps[i] == BGV_OK;
    if (kind[si] == kWrong || kind[si] == kInfSig) defect[i] = 1 + splitmix(seed * 0x10001 + (uint64_t)si) % (kP - 1);
  }
  auto value = [&](const bgv_dgroup& g, uint32_t base) {
    if (g.first_slot < base || g.first_slot - base + g.n_slots > nslots || g.n_slots > BGV_WAVE)
      die(name + ": a group reaches outside the call's slots");
    uint64_t v = 0;
    for (uint32_t k = 0; k < g.n_slots; ++k) {
      const uint32_t s = g.first_slot - base + k;
      if (!((g.mask >> k) & 1) || !live[s]) continue;
      v = addm(v, (g.flags & BGV_GROUP_WEIGHTED) ? mulm(k + 1, defect[s]) : defect[s]);
    }
    return v;
  };

  // first pass
  std::vector<uint64_t> v1(ngroups);
  std::vector<int32_t> verdict(ngroups);
  for (uint32_t g = 0; g < ngroups; ++g) {
    v1[g] = value(L.groups[g], 0);
    verdict[g] = v1[g] == 0 ? 1 : 0;
  }
  plan.slot_base = 0;
  plan.after_pass1(ss.data(), ps.data(), verdict.data());
  bool any_uniform = false;
  for (char u : L.group_uniform) any_uniform = any_uniform || u;
  const Json* ju = sc.get("uniform");
  const bool uniform = uniform_enabled() && any_uniform && ju && ju->i;
  const bool want_gu = plan.any_pattern_eligible();

  // retry rounds
  std::vector<int64_t> round_groups;
  std::vector<uint64_t> round_digest;
  for (;;) {
    std::vector<bgv_dgroup> rg;
    plan.build_parts(rg, want_gu ? 0 : -1, uniform);
    if (rg.empty()) break;
    if ((int)round_groups.size() == kMaxRounds) die(name + ": not finished after 16 rounds");
    round_groups.push_back((int64_t)rg.size());
    round_digest.push_back(digest(rg));
    const bool gu1 = !plan.punits.empty();  // retry_launch hands the first pass's u values over
    std::vector<int32_t> rv(rg.size());
    for (size_t t = 0; t < rg.size(); ++t) {
      const bgv_dgroup& g = rg[t];
      if (g.ref1 > ngroups) die(name + ": a test's reference is no first-pass group");
      if (g.ref1 && !want_gu) die(name + ": a reference without the first pass's u values");
      const uint64_t v = value(g, plan.slot_base);
      int32_t bits = v == 0 ? 1 : 0;
      if (gu1 && g.ref1 && addm(v1[g.ref1 - 1], kP - v) == 0) bits |= 2;
      if ((g.flags & BGV_GROUP_WEIGHTED) && g.ref1) {
        int32_t found = 0;
        for (uint32_t w = 1; w <= g.n_slots && !found; ++w)
          if (mulm(w, v1[g.ref1 - 1]) == v) found = (int32_t)w;
        bits = (bits & 1) | (found << 8);
      }
      rv[t] = bits;
    }
    plan.after_round(rv.data());
  }

  printf("{\"name\": \"%s\", ", name.c_str());
  print_list("codes", std::vector<int64_t>(plan.code.begin(), plan.code.end()));
  printf(", \"rounds\": %zu, ", round_groups.size());
  print_list("groups", round_groups);
  printf(", \"digest\": [");
  for (size_t r = 0; r < round_digest.size(); ++r) printf("%s\"%016llx\"", r ? ", " : "", (unsigned long long)round_digest[r]);
  printf("], \"batch_retries\": %llu, \"device_groups\": %llu, \"sets_verified\": %llu, \"batch_sigs_success\": %llu",
         (unsigned long long)plan.st.batch_retries, (unsigned long long)plan.st.device_groups,
         (unsigned long long)plan.st.sets_verified, (unsigned long long)plan.st.batch_sigs_success);
  const Json* jl = sc.get("layout");
  if (jl && jl->i) {
    // first-pass groups as [first_slot, n_slots, shared, uniform]; per slot its set's root (-1: a
    // pad) and the root of the slot whose H(msg) it uses; the slots hashed
    printf(", \"nslots\": %u, \"layout_groups\": [", nslots);
    for (uint32_t g = 0; g < ngroups; ++g)
      printf("%s[%u, %u, %d, %d]", g ? ", " : "", L.groups[g].first_slot, L.groups[g].n_slots, (int)L.group_shared[g],
             (int)L.group_uniform[g]);
    printf("], ");
    std::vector<int64_t> slot_root(nslots, -1), hsrc_root(nslots, -1);
    for (uint32_t i = 0; i < nslots; ++i) {
      if (L.slot_set[i] < 0) continue;
      slot_root[i] = root[L.slot_set[i]];
      const uint32_t h = L.slots[i].hsrc;
      if (h >= nslots || L.slot_set[h] < 0) die(name + ": hsrc names no set's slot");
      hsrc_root[i] = root[L.slot_set[h]];
    }
    print_list("slot_root", slot_root);
    printf(", ");
    print_list("hsrc_root", hsrc_root);
    printf(", ");
    print_list("uniq", std::vector<int64_t>(L.uniq.begin(), L.uniq.end()));
  }
  printf("}\n");
}

// layout_one_job_fast against the Builder on one non-batchable job of n sets: committees of 127
// sets per root, every 5th committee repeating an earlier root, every 7th colliding with one
void run_fast_layout(const Json& sc) {
  const uint32_t n = (uint32_t)sc.num("n", 1 << 17);
  Sets S;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = i / 127;
    S.add(c % 5 == 4 ? c / 2 : c % 7 == 3 ? c / 2 + (1ull << 32) : c);
  }
  S.finish();
  const bgv_job job{0, n, 0};
  Layout a, b;
  for (Layout* L : {&a, &b}) {
    L->job_groups.resize(1);
    L->job_first_slot.assign(1, 0);
  }
  const bool fast = layout_one_job_fast(a, job, S.rec.data());
  Builder B(b);
  for (uint32_t k = 0; k < n; ++k) B.add(0, k, S.rec[k], k == 0);
  B.pad_to_wave();
  size_t differ = 0;
  if (a.slots.size() != b.slots.size() || a.groups.size() != b.groups.size()) {
    differ = 1;
  } else {
    for (size_t i = 0; i < a.slots.size(); ++i) differ += memcmp(&a.slots[i], &b.slots[i], sizeof(bgv_dslot)) != 0;
    for (size_t g = 0; g < a.groups.size(); ++g)
      differ += a.groups[g].first_slot != b.groups[g].first_slot || a.groups[g].n_slots != b.groups[g].n_slots ||
                a.groups[g].mask != b.groups[g].mask || a.groups[g].ref1 != b.groups[g].ref1 ||
                a.groups[g].flags != b.groups[g].flags;
    differ += a.slot_set != b.slot_set;
    differ += a.job_groups != b.job_groups;
    differ += a.job_first_slot != b.job_first_slot;
    differ += a.group_shared != b.group_shared;
    differ += a.group_uniform != b.group_uniform;
    differ += a.idx != b.idx;
    differ += a.pkb != b.pkb;
    differ += a.uniq != b.uniq;
  }
  printf("{\"name\": \"%s\", \"fast\": %s, \"nslots\": %zu, \"ngroups\": %zu, \"nuniq\": %zu, \"differ\": %zu}\n",
         sc.get("name") ? sc.get("name")->s.c_str() : "", fast ? "true" : "false", a.slots.size(), a.groups.size(),
         a.uniq.size(), differ);
}

}  // namespace

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : stdin;
  if (!f) die(std::string("cannot open ") + argv[1]);
  std::string text;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
  if (f != stdin) fclose(f);
  Reader rd(text);
  const Json all = rd.value();
  if (all.kind != Json::Arr) die("the input is a JSON list of scenarios");
  for (const Json& sc : all.a) {
    const Json* op = sc.get("op");
    if (op && op->s == "fast_layout")
      run_fast_layout(sc);
    else
      run_scenario(sc);
  }
  return 0;
}
