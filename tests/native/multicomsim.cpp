// CPU simulation of the span sets -- one bitfield over several committees (blsgpu.h bgv_pkspan):
// the host's cut of the bitfield into a slot's run and the per-lane walk over it (bgv_pk_bits.h)
// with the host build of the G1 arithmetic (bls_curve.h), and the host checks and layout of calls
// that hold span sets (bgv_host_layout.h).  Test infrastructure only; it reads a line protocol
// from stdin (tests/test_multi_committee_cpu.py writes it) and prints what it computed.
//
//   multicomsim agg
//     keys <N>                          then N lines of 48-byte compressed pubkeys (hex)
//     committee <handle> <n> <i_0> ...  a committee's members as key numbers
//     case <T> <n_bits> <bitshex> <nc> <handle_0> ...
//     -> one line per case: the 96-byte uncompressed aggregate (hex), then M
//   Each case emulates k_pk_agg_span serially: pkb_span_build makes the run, lane l of the team
//   of T walks it with pkb_span_next and sums its terms as the kernel does (members negated on
//   the complement side, then the totals of its rank), and the lanes' sums are combined by the
//   xor butterfly.
//
//   multicomsim layout
//     committee <id> <handle> <n> <bad>     the host's mirror of a live committee
//     call <mode>                           a call of one-set non-batchable jobs
//     set idx <n_pk> <i_0> ...  |  set com <id> <n_bits> <bitshex or ->
//       |  set span <n_bits> <bitshex or -> <nc> <id_0> ...
//     end
//     -> per call: "code <set> <code>" per set, "slot <s> <set> <flags> <n_pk> <pk_off> <group>"
//        per non-pad slot, "idx ...", "team ...", "wave ...", "steam ...", "swave ..."; after the
//        last call the merged super-batch as run_pass1 forms it: "mslot ...", "midx ...",
//        "mlist ..." (committee teams, committee waves, span teams, span waves)
//   A call with a span set goes through span_set_check for all its committee sets (a "com" set as
//   a span of one committee), as bgv_verify_spans does; one without, through committee_set_check.
#include <stdio.h>

#include <map>
#include <sstream>
#include <string>

// -DMULTICOMSIM_LAYOUT_ONLY leaves the G1 arithmetic and the agg mode out (the sanitizer build)
#ifndef MULTICOMSIM_LAYOUT_ONLY
#define BGV_OK BGV_CURVE_OK
#include "../../lodestar_amd/csrc/bls_curve.h"
#undef BGV_OK
#endif
#include "../../lodestar_amd/csrc/bgv_host_layout.h"

namespace {

[[noreturn]] void die(const std::string& why) {
  fprintf(stderr, "multicomsim: %s\n", why.c_str());
  exit(2);
}

std::vector<uint8_t> unhex(const std::string& h) {
  if (h == "-") return {};
  if (h.size() % 2) die("odd hex length");
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

#ifndef MULTICOMSIM_LAYOUT_ONLY
int run_agg() {
  std::vector<g1_aff> cache;
  std::map<uint32_t, std::vector<uint32_t>> members;  // by handle
  std::map<uint32_t, g1_jac> total;
  static char buf[1 << 20];
  while (fgets(buf, sizeof(buf), stdin)) {
    std::istringstream in(buf);
    std::string op;
    if (!(in >> op)) continue;
    if (op == "keys") {
      size_t nk;
      in >> nk;
      for (size_t i = 0; i < nk; ++i) {
        if (!fgets(buf, sizeof(buf), stdin)) die("keys end early");
        std::istringstream kin(buf);
        std::string h;
        kin >> h;
        const std::vector<uint8_t> b = unhex(h);
        g1_aff a;
        bool inf;
        if (b.size() != 48 || g1_decompress(&a, &inf, b.data()) != 0 || inf) die("bad key");
        cache.push_back(a);
      }
    } else if (op == "committee") {
      uint32_t h, n;
      in >> h >> n;
      std::vector<uint32_t> m(n);
      g1_jac t = jac_infinity<fp_t>();
      for (uint32_t& v : m) {
        in >> v;
        if (v >= cache.size()) die("member past the keys");
        t = jac_add_aff(t, cache[v]);
      }
      if (!in || n == 0) die("bad committee line");
      members[h] = m;
      total[h] = t;
    } else if (op == "case") {
      uint32_t T, n_bits, nc;
      std::string bh;
      in >> T >> n_bits >> bh >> nc;
      const std::vector<uint8_t> bits = unhex(bh);
      std::vector<pkb_part> parts(nc);
      uint32_t off = 0;
      for (pkb_part& p : parts) {
        in >> p.handle;
        if (!members.count(p.handle)) die("unknown handle");
        p.n = (uint32_t)members[p.handle].size();
        p.k = pkb_span_count(bits.data(), (uint32_t)bits.size(), off, p.n);
        off += p.n;
      }
      if (!in || (T != 16 && T != 64) || off != n_bits || bits.size() != (n_bits + 7) / 8) die("bad case line");
      std::vector<uint32_t> run;
      const uint32_t M = pkb_span_build(parts.data(), nc, bits.data(), (uint32_t)bits.size(),
                                        [&](uint32_t v) { run.push_back(v); });
      const uint32_t nrec = run[0], ncomp = run[1];
      if (run[2] != M || run.size() != PKB_SPAN_HEAD + ncomp + 2 * nrec) die("run header");
      const uint32_t* tot = run.data() + PKB_SPAN_HEAD;
      const uint32_t* recs = tot + ncomp;
      std::vector<g1_jac> acc(T, jac_infinity<fp_t>());
      uint32_t taken = 0;
      for (uint32_t l = 0; l < T; ++l) {
        pkb_span_cursor c = pkb_span_begin(l);
        uint32_t meta, pos, mine = 0;
        while (pkb_span_next(c, recs, nrec, T, &meta, &pos)) {
          const std::vector<uint32_t>& m = members[pkb_meta_handle(meta)];
          if (pos >= m.size()) die("selected position past its committee");
          g1_aff a = cache[m[pos]];
          if (pkb_meta_complement(meta)) a.y = fp_neg(a.y);
          acc[l] = mine ? jac_add_aff(acc[l], a) : jac_from_aff(a);
          ++mine;
        }
        for (uint32_t t = c.want - c.base; t < ncomp; t += T, ++mine) acc[l] = jac_add(acc[l], total[tot[t]]);
        if (mine != (M > l ? (M - l + T - 1) / T : 0u)) die("a lane's additions must be ceil((M - l) / T)");
        taken += mine;
      }
      if (taken != M) die("the lanes together must take every term once");
      for (uint32_t m = T / 2; m >= 1; m /= 2) {
        std::vector<g1_jac> nx(T);
        for (uint32_t l = 0; l < T; ++l) nx[l] = jac_add(acc[l], acc[l ^ m]);
        acc = nx;
      }
      g1_aff a;
      const bool fin = jac_to_aff(&a, acc[0]);
      uint8_t out[96];
      g1_serialize(out, a, !fin);
      for (uint8_t v : out) printf("%02x", v);
      printf(" %u\n", M);
    } else {
      die("unknown line: " + op);
    }
  }
  return 0;
}
#endif  // MULTICOMSIM_LAYOUT_ONLY

struct SimSet {
  int kind = 0;  // 0 idx, 1 com, 2 span
  std::vector<uint32_t> idx, ids;
  uint32_t n_bits = 0;
  std::vector<uint8_t> bits;
};

int run_layout() {
  std::map<uint32_t, CommitteeInfo> mirror;
  std::vector<std::unique_ptr<Layout>> layouts;
  static const uint8_t msg[32] = {1}, sig[96] = {2};
  static char buf[1 << 18];
  while (fgets(buf, sizeof(buf), stdin)) {
    std::istringstream in(buf);
    std::string op;
    if (!(in >> op)) continue;
    if (op == "committee") {
      uint32_t id, h, n, bad;
      in >> id >> h >> n >> bad;
      mirror[id] = CommitteeInfo{h, n, bad != 0};
    } else if (op == "call") {
      int mode;
      in >> mode;
      std::vector<SimSet> S;
      bool any_span = false;
      while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream sin(buf);
        std::string w, kind, bh;
        sin >> w;
        if (w == "end") break;
        sin >> kind;
        SimSet s;
        if (kind == "idx") {
          size_t n;
          sin >> n;
          s.idx.resize(n);
          for (uint32_t& v : s.idx) sin >> v;
        } else if (kind == "com") {
          s.kind = 1;
          s.ids.resize(1);
          sin >> s.ids[0] >> s.n_bits >> bh;
          s.bits = unhex(bh);
        } else {
          s.kind = 2;
          size_t nc;
          sin >> s.n_bits >> bh >> nc;
          s.ids.resize(nc);
          for (uint32_t& v : s.ids) sin >> v;
          s.bits = unhex(bh);
          any_span = true;
        }
        if (!sin || (s.kind && s.bits.size() != (s.n_bits + 7) / 8)) die("bad set line");
        S.push_back(std::move(s));
      }
      // the call as bgv_sched.cpp's call_submit sees it
      const size_t n = S.size();
      std::vector<bgv_set> sets(n);
      std::vector<bgv_job> jobs(n);
      std::vector<SetCommittee> sc(n);
      std::vector<int32_t> code(n, 2);
      const auto look = [&](uint32_t id, CommitteeInfo* ci) {
        const auto it = mirror.find(id);
        if (it == mirror.end()) return false;
        *ci = it->second;
        return true;
      };
      for (size_t i = 0; i < n; ++i) {
        sets[i] = bgv_set{(uint32_t)S[i].idx.size(), 96, S[i].kind ? nullptr : S[i].idx.data(), nullptr, msg, sig};
        if (S[i].kind) sets[i].n_pk = 0xDEAD;  // ignored for a committee set
        jobs[i] = bgv_job{(uint32_t)i, 1, 0};
        if (S[i].kind && any_span) {
          const bgv_pkspan sp{S[i].ids.data(), (uint32_t)S[i].ids.size(), S[i].n_bits, S[i].bits.data()};
          code[i] = span_set_check(look, sp, &sc[i]);
        } else if (S[i].kind) {
          const bgv_pkbits pb{S[i].ids[0], S[i].n_bits, S[i].bits.data()};
          CommitteeInfo ci{};
          const bool live = look(pb.committee, &ci);
          code[i] = committee_set_check(live ? &ci : nullptr, pb, &sc[i]);
        }
        printf("code %zu %d\n", i, code[i]);
      }
      layouts.push_back(std::make_unique<Layout>());
      Layout& L = *layouts.back();
      std::vector<size_t> todo;
      layout_call(L, todo, jobs.data(), n, sets.data(), mode, code, sc.data());
      for (size_t s = 0; s < L.slots.size(); ++s)
        if (!(L.slots[s].flags & BGV_SLOT_PAD))
          printf("slot %zu %d %u %u %u %u\n", s, L.slot_set[s], L.slots[s].flags, L.slots[s].n_pk, L.slots[s].pk_off,
                 L.slots[s].group);
      const auto list = [](const char* name, const std::vector<uint32_t>& v) {
        printf("%s", name);
        for (uint32_t x : v) printf(" %u", x);
        printf("\n");
      };
      list("idx", L.idx);
      list("team", L.com_team);
      list("wave", L.com_wave);
      list("steam", L.span_team);
      list("swave", L.span_wave);
    } else {
      die("unknown line: " + op);
    }
  }
  // the calls merged into one super-batch (bgv_sched.cpp run_pass1)
  uint32_t ns = 0, ni = 0, npb = 0, ng = 0;
  std::vector<uint32_t> midx, lists[4];
  for (const auto& Lp : layouts) {
    const Layout& L = *Lp;
    for (size_t s = 0; s < L.slots.size(); ++s) {
      const bgv_dslot d = rebase_slot(L.slots[s], ns, ni, npb / 96, ng);
      if (!(d.flags & BGV_SLOT_PAD)) printf("mslot %zu %u %u %u %u\n", ns + s, d.flags, d.n_pk, d.pk_off, d.group);
    }
    const std::vector<uint32_t>* src[4] = {&L.com_team, &L.com_wave, &L.span_team, &L.span_wave};
    for (int q = 0; q < 4; ++q)
      for (uint32_t v : *src[q]) lists[q].push_back(v + ns);
    midx.insert(midx.end(), L.idx.begin(), L.idx.end());
    ns += (uint32_t)L.slots.size();
    ni += (uint32_t)L.idx.size();
    npb += (uint32_t)L.pkb.size();
    ng += (uint32_t)L.groups.size();
  }
  printf("midx");
  for (uint32_t v : midx) printf(" %u", v);
  printf("\nmlist");
  for (int q = 0; q < 4; ++q)
    for (uint32_t v : lists[q]) printf(" %u", v);
  printf("\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
#ifndef MULTICOMSIM_LAYOUT_ONLY
  if (mode == "agg") return run_agg();
#endif
  if (mode == "layout") return run_layout();
  die("usage: multicomsim agg|layout < input");
}
