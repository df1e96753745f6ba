// CPU simulation of the committee-bitfield sets: the per-lane selection and the mode decision
// (bgv_pk_bits.h) with the host build of the G1 arithmetic (bls_curve.h), and the host layout of
// calls that hold committee sets (bgv_host_layout.h).  Test infrastructure only; it reads a line
// protocol from stdin (tests/test_committee_bits_cpu.py writes it) and prints what it computed.
//
//   committeesim agg
//     keys <N>                      then N lines of 48-byte compressed pubkeys (hex)
//     case <T> <mode> <n> <bitshex> <i_0> ... <i_{n-1}>
//                                   T lanes per team (16 / 64); mode 0 direct, 1 complement,
//                                   2 the derived one; the committee's members as key numbers
//     -> one line per case: the 96-byte uncompressed aggregate (hex)
//   Each case emulates k_pk_agg_bits serially: lane l of the team walks the selection with
//   pkb_next and sums its members as the kernel does, the lanes' sums are combined by the xor
//   butterfly, and complement mode subtracts from the committee's total (all bits, T = 64).
//
//   committeesim layout
//     committee <id> <handle> <n> <bad>     the host's mirror of a live committee
//     call <mode>                           a call of one-set non-batchable jobs
//     set idx <n_pk> <i_0> ...              | set com <id> <n_bits> <bitshex or ->
//     end
//     -> per call: "code <set> <code>" per set, "slot <s> <set> <flags> <n_pk> <pk_off> <group>"
//        per non-pad slot, "idx ...", "team ...", "wave ..."; after the last call the merged
//        super-batch as run_pass1 forms it: "mslot <s> <flags> <n_pk> <pk_off> <group>",
//        "midx ...", "mcom ..."
#include <stdio.h>

#include <map>
#include <sstream>
#include <string>

// -DCOMMITTEESIM_LAYOUT_ONLY leaves the G1 arithmetic and the agg mode out (the sanitizer build:
// the layout driver alone compiles in seconds, the arithmetic headers take minutes there)
#ifndef COMMITTEESIM_LAYOUT_ONLY
// the device arithmetic first (it defines BGV_HD); its status enum and blsgpu.h's both name
// the value 0 BGV_OK, which no kernel unit sees together
#define BGV_OK BGV_CURVE_OK
#include "../../lodestar_amd/csrc/bls_curve.h"
#undef BGV_OK
#endif
#include "../../lodestar_amd/csrc/bgv_host_layout.h"

namespace {

[[noreturn]] void die(const std::string& why) {
  fprintf(stderr, "committeesim: %s\n", why.c_str());
  exit(2);
}

std::vector<uint8_t> unhex(const std::string& h) {
  if (h == "-") return {};
  if (h.size() % 2) die("odd hex length");
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

std::vector<uint32_t> bit_words(const std::vector<uint8_t>& bits, uint32_t n) {
  std::vector<uint32_t> w(pkb_nwords(n), 0u);
  for (size_t i = 0; i < bits.size() && i / 4 < w.size(); ++i) w[i / 4] |= (uint32_t)bits[i] << (8 * (i % 4));
  return w;
}

#ifndef COMMITTEESIM_LAYOUT_ONLY
// k_pk_agg_bits' sum of one side on a team of T lanes (bgv_k_prep.hip pk_bits_sum), lane by lane
g1_jac team_sum(uint32_t T, const uint32_t* words, const std::vector<uint32_t>& members, bool comp,
                const std::vector<g1_aff>& cache) {
  const uint32_t n = (uint32_t)members.size();
  std::vector<g1_jac> acc(T, jac_infinity<fp_t>());
  uint32_t taken = 0;
  for (uint32_t l = 0; l < T; ++l) {
    pkb_cursor c = pkb_begin(l);
    uint32_t pos, mine = 0, last = 0;
    while (pkb_next(c, words, n, comp, T, &pos)) {
      if (pos >= n) die("selected position past the committee");
      if (mine && pos <= last) die("positions of one lane must increase");
      acc[l] = mine ? jac_add_aff(acc[l], cache[members[pos]]) : jac_from_aff(cache[members[pos]]);
      last = pos;
      ++mine;
    }
    taken += mine;
  }
  uint32_t want = 0;
  for (uint32_t w = 0; w < pkb_nwords(n); ++w) want += pkb_popc(pkb_word(words, n, comp, w));
  if (taken != want) die("the lanes together must take every selected member once");
  for (uint32_t m = T / 2; m >= 1; m /= 2) {
    std::vector<g1_jac> nx(T);
    for (uint32_t l = 0; l < T; ++l) nx[l] = jac_add(acc[l], acc[l ^ m]);
    acc = nx;
  }
  return acc[0];
}

int run_agg() {
  std::vector<g1_aff> cache;
  std::string line;
  char buf[1 << 20];
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
    } else if (op == "case") {
      uint32_t T, mode, n;
      std::string bh;
      in >> T >> mode >> n >> bh;
      std::vector<uint32_t> members(n);
      for (uint32_t& m : members) {
        in >> m;
        if (m >= cache.size()) die("member past the keys");
      }
      if (!in || (T != 16 && T != 64) || n == 0) die("bad case line");
      const std::vector<uint32_t> words = bit_words(unhex(bh), n);
      uint32_t k = 0;
      for (uint32_t w = 0; w < pkb_nwords(n); ++w) k += pkb_popc(pkb_word(words.data(), n, false, w));
      const bool comp = mode == 2 ? pkb_use_complement(n, k) : mode == 1;
      g1_jac acc = team_sum(T, words.data(), members, comp, cache);
      if (comp) acc = jac_add(team_sum(64, nullptr, members, false, cache), jac_neg(acc));
      g1_aff a;
      const bool fin = jac_to_aff(&a, acc);
      uint8_t out[96];
      g1_serialize(out, a, !fin);
      for (uint8_t v : out) printf("%02x", v);
      printf(" %d\n", comp ? 1 : 0);
    } else {
      die("unknown line: " + op);
    }
  }
  return 0;
}

#endif  // COMMITTEESIM_LAYOUT_ONLY

struct SimSet {
  bool com = false;
  std::vector<uint32_t> idx;
  uint32_t id = 0, n_bits = 0;
  std::vector<uint8_t> bits;
};

int run_layout() {
  std::map<uint32_t, CommitteeInfo> mirror;
  std::vector<std::unique_ptr<Layout>> layouts;
  static const uint8_t msg[32] = {1}, sig[96] = {2};
  char buf[1 << 16];
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
      while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream sin(buf);
        std::string w, kind;
        sin >> w;
        if (w == "end") break;
        sin >> kind;
        SimSet s;
        if (kind == "idx") {
          size_t n;
          sin >> n;
          s.idx.resize(n);
          for (uint32_t& v : s.idx) sin >> v;
        } else {
          std::string bh;
          s.com = true;
          sin >> s.id >> s.n_bits >> bh;
          s.bits = unhex(bh);
          if (s.bits.size() != (s.n_bits + 7) / 8) die("bits length");
        }
        if (!sin) die("bad set line");
        S.push_back(std::move(s));
      }
      // the call as bgv_sched.cpp's call_submit sees it
      const size_t n = S.size();
      std::vector<bgv_set> sets(n);
      std::vector<bgv_pkbits> pkb(n);
      std::vector<bgv_job> jobs(n);
      std::vector<SetCommittee> sc(n);
      std::vector<int32_t> code(n, 2);
      for (size_t i = 0; i < n; ++i) {
        sets[i] = bgv_set{(uint32_t)S[i].idx.size(), 96, S[i].com ? nullptr : S[i].idx.data(), nullptr, msg, sig};
        if (S[i].com) sets[i].n_pk = 0xDEAD;  // ignored for a committee set
        pkb[i] = bgv_pkbits{S[i].com ? S[i].id : BGV_NO_COMMITTEE, S[i].n_bits, S[i].bits.data()};
        jobs[i] = bgv_job{(uint32_t)i, 1, 0};
        if (S[i].com) {
          auto it = mirror.find(S[i].id);
          code[i] = committee_set_check(it == mirror.end() ? nullptr : &it->second, pkb[i], &sc[i]);
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
      printf("idx");
      for (uint32_t v : L.idx) printf(" %u", v);
      printf("\nteam");
      for (uint32_t v : L.com_team) printf(" %u", v);
      printf("\nwave");
      for (uint32_t v : L.com_wave) printf(" %u", v);
      printf("\n");
    } else {
      die("unknown line: " + op);
    }
  }
  // the calls merged into one super-batch (bgv_sched.cpp run_pass1)
  uint32_t ns = 0, ni = 0, npb = 0, ng = 0;
  std::vector<uint32_t> midx, team, wave;
  for (const auto& Lp : layouts) {
    const Layout& L = *Lp;
    for (size_t s = 0; s < L.slots.size(); ++s) {
      const bgv_dslot d = rebase_slot(L.slots[s], ns, ni, npb / 96, ng);
      if (!(d.flags & BGV_SLOT_PAD)) printf("mslot %zu %u %u %u %u\n", ns + s, d.flags, d.n_pk, d.pk_off, d.group);
    }
    for (uint32_t v : L.com_team) team.push_back(v + ns);
    for (uint32_t v : L.com_wave) wave.push_back(v + ns);
    midx.insert(midx.end(), L.idx.begin(), L.idx.end());
    ns += (uint32_t)L.slots.size();
    ni += (uint32_t)L.idx.size();
    npb += (uint32_t)L.pkb.size();
    ng += (uint32_t)L.groups.size();
  }
  printf("midx");
  for (uint32_t v : midx) printf(" %u", v);
  printf("\nmcom");
  for (uint32_t v : team) printf(" %u", v);
  for (uint32_t v : wave) printf(" %u", v);
  printf("\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
#ifndef COMMITTEESIM_LAYOUT_ONLY
  if (mode == "agg") return run_agg();
#endif
  if (mode == "layout") return run_layout();
  die("usage: committeesim agg|layout < input");
}
