// CPU driver of the host plan of pool entries with bits (lodestar_amd/csrc/bgv_sigpool_bits_plan.h):
// reads cases from stdin, runs the tag check, the bits check, the plan and the commit, and prints
// what they decided.  Test infrastructure only (tests/sigpoolbitssim.py).
//
//   stdin:  T, then per case:  njobs nsets nentries nchanged nflags wave_max have_bits
//                              njobs x (first_set n_sets code)
//                              nsets x tag
//                              have_bits ? nsets x (n_bits bit hex|-)      hex: the field, '-': bits == NULL
//                              nentries x (id generation count n_bits hex|-)   the registry at submit
//                              nchanged x (id live generation count n_bits hex|-)  what changed before the step
//                              nflags x (id flag)                          entries the device flags
//   stdout: per case one line: rc form n | ids | first | count | member | outcome[nsets] | id:count:n_bits:hex ...
//           (rc: the first check that fails; then the line ends after it.  The last field lists
//           every live entry after the commit, ascending.)
//   `consts` prints BGV_NO_AGG, BGV_SIGAGG_WAVE_MAX, BGV_MAX_SIGPOOL, BGV_SIGPOOL_MAX_BITS,
//   BGV_SIGPOOL_BITS_BYTES, BGV_MAX_SUM_ENTRIES and the four BGV_POOL_* values.
//   `concat` reads T, then per case n, n x (n_bits hex|-), and prints total_bits hex of
//   sigpool_append_bits over the list.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../lodestar_amd/csrc/bgv_sigpool_bits_plan.h"

static bool read_hex(std::vector<uint8_t>* out, bool* null) {
  char buf[2 * BGV_SIGPOOL_BITS_BYTES + 8];
  if (scanf("%519s", buf) != 1) return false;
  out->clear();
  *null = !strcmp(buf, "-");
  if (*null) return true;
  const size_t n = strlen(buf);
  if (n % 2) return false;
  for (size_t k = 0; k < n; k += 2) {
    unsigned v;
    if (sscanf(buf + k, "%2x", &v) != 1) return false;
    out->push_back((uint8_t)v);
  }
  return true;
}

static void print_hex(const uint8_t* p, size_t n) {
  for (size_t k = 0; k < n; ++k) printf("%02x", p[k]);
  if (!n) printf("-");
}

struct Registry {
  std::vector<uint8_t> live, written, bits;
  std::vector<uint32_t> gen, count, nbits;
  Registry()
      : live(BGV_MAX_SIGPOOL, 0), written(BGV_MAX_SIGPOOL, 0), bits((size_t)BGV_MAX_SIGPOOL * BGV_SIGPOOL_BITS_BYTES, 0),
        gen(BGV_MAX_SIGPOOL, 0), count(BGV_MAX_SIGPOOL, 0), nbits(BGV_MAX_SIGPOOL, 0) {}
  bool read_entry(bool with_live) {
    unsigned id, l = 1, g, cnt, nb;
    if (scanf("%u", &id) != 1 || id >= BGV_MAX_SIGPOOL) return false;
    if (with_live && scanf("%u", &l) != 1) return false;
    if (scanf("%u %u %u", &g, &cnt, &nb) != 3 || nb > BGV_SIGPOOL_MAX_BITS) return false;
    std::vector<uint8_t> f;
    bool null;
    if (!read_hex(&f, &null) || f.size() > BGV_SIGPOOL_BITS_BYTES) return false;
    live[id] = l != 0;
    gen[id] = g;
    count[id] = cnt;
    written[id] = cnt != 0;
    nbits[id] = nb;
    uint8_t* b = bits.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * id;
    memset(b, 0, BGV_SIGPOOL_BITS_BYTES);
    if (!f.empty()) memcpy(b, f.data(), f.size());
    return true;
  }
  SigPoolBitsView view() const { return SigPoolBitsView{live.data(), gen.data(), nbits.data(), bits.data()}; }
};

static int run_concat() {
  unsigned T = 0;
  if (scanf("%u", &T) != 1) return 2;
  for (unsigned t = 0; t < T; ++t) {
    unsigned n;
    if (scanf("%u", &n) != 1) return 2;
    std::vector<std::vector<uint8_t>> src(n);
    std::vector<uint32_t> nb(n);
    size_t total = 0;
    for (unsigned k = 0; k < n; ++k) {
      bool null;
      if (scanf("%u", &nb[k]) != 1 || !read_hex(&src[k], &null)) return 2;
      if (src[k].size() != sigpool_bits_bytes(nb[k])) return 3;
      total += nb[k];
    }
    // exactly ceil(total / 8) bytes on the heap: the sanitized build sees a write past them
    std::vector<uint8_t> dst((total + 7) / 8, 0);
    size_t off = 0;
    for (unsigned k = 0; k < n; ++k) {
      if (nb[k]) sigpool_append_bits(dst.data(), off, src[k].data(), nb[k]);
      off += nb[k];
    }
    printf("%zu ", total);
    print_hex(dst.data(), dst.size());
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "consts")) {
    printf("%u %u %u %u %u %u %d %d %d %d\n", BGV_NO_AGG, (unsigned)BGV_SIGAGG_WAVE_MAX, (unsigned)BGV_MAX_SIGPOOL,
           (unsigned)BGV_SIGPOOL_MAX_BITS, (unsigned)BGV_SIGPOOL_BITS_BYTES, (unsigned)BGV_MAX_SUM_ENTRIES,
           BGV_POOL_NOT_ADDED, BGV_POOL_ADDED, BGV_POOL_KNOWN, BGV_POOL_OVERLAP);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "concat")) return run_concat();
  unsigned T = 0;
  if (scanf("%u", &T) != 1) return 2;
  for (unsigned t = 0; t < T; ++t) {
    unsigned long njobs, nsets, nentries, nchanged, nflags, wave_max, have_bits;
    if (scanf("%lu %lu %lu %lu %lu %lu %lu", &njobs, &nsets, &nentries, &nchanged, &nflags, &wave_max, &have_bits) != 7)
      return 2;
    std::vector<bgv_job> jobs(njobs);
    std::vector<int32_t> codes(njobs);
    for (size_t j = 0; j < njobs; ++j) {
      jobs[j].batchable = 1;
      if (scanf("%u %u %d", &jobs[j].first_set, &jobs[j].n_sets, &codes[j]) != 3) return 2;
      if ((size_t)jobs[j].first_set + jobs[j].n_sets > nsets) return 3;
    }
    std::vector<uint32_t> tags(nsets);
    for (size_t i = 0; i < nsets; ++i)
      if (scanf("%u", &tags[i]) != 1) return 2;
    // every field on the heap with exactly the bytes the caller gave: the sanitized build sees any
    // read past ceil(n_bits / 8)
    std::vector<bgv_poolbits> pb(have_bits ? nsets : 0);
    std::vector<std::unique_ptr<uint8_t[]>> store(pb.size());
    for (size_t i = 0; i < pb.size(); ++i) {
      std::vector<uint8_t> f;
      bool null;
      if (scanf("%u %u", &pb[i].n_bits, &pb[i].bit) != 2 || !read_hex(&f, &null)) return 2;
      pb[i].bits = nullptr;
      if (!null) {
        store[i].reset(new uint8_t[f.size() ? f.size() : 1]);
        if (!f.empty()) memcpy(store[i].get(), f.data(), f.size());
        pb[i].bits = store[i].get();
      }
    }
    Registry r;
    for (size_t k = 0; k < nentries; ++k)
      if (!r.read_entry(false)) return 2;
    std::vector<uint32_t> gen_of_set;
    SigPoolFields fields;
    int rc = sigpool_check_tags(tags.data(), nsets, SigPoolView{r.live.data(), r.gen.data()}, &gen_of_set);
    if (rc == BGV_OK) rc = sigpool_check_bits(tags.data(), have_bits ? pb.data() : nullptr, nsets, r.view(), &fields);
    // the submit has its copy: what the caller does to its buffers afterwards changes nothing
    for (size_t i = 0; i < pb.size(); ++i) {
      if (store[i]) store[i][0] ^= 0xFF;
      store[i].reset();
      pb[i].n_bits = 0;
    }
    for (size_t k = 0; k < nchanged; ++k)
      if (!r.read_entry(true)) return 2;
    std::vector<std::pair<unsigned, int>> flagged(nflags);
    for (size_t k = 0; k < nflags; ++k)
      if (scanf("%u %d", &flagged[k].first, &flagged[k].second) != 2) return 2;
    if (rc != BGV_OK) {
      printf("%d\n", rc);
      continue;
    }
    SigPoolBitsPlan p;
    sigpool_plan_bits(jobs.data(), njobs, codes.data(), tags.data(), gen_of_set.data(), nsets, r.view(), fields, wave_max,
                      &p);
    const SigPoolPlan& q = p.plan;
    printf("0 %d %zu |", q.form, q.member.size());
    for (uint32_t v : q.ids) printf(" %u", v);
    printf(" |");
    for (uint32_t v : q.first) printf(" %u", v);
    printf(" |");
    for (uint32_t v : q.count) printf(" %u", v);
    printf(" |");
    for (uint32_t v : q.member) printf(" %u", v);
    std::vector<int32_t> flag(q.ids.size(), BGV_OK);
    for (size_t e = 0; e < q.ids.size(); ++e)
      for (const auto& fl : flagged)
        if (fl.first == q.ids[e]) flag[e] = fl.second;
    sigpool_commit_bits(&p, flag.data(), tags.data(), nsets, r.written.data(), r.count.data(), r.bits.data());
    printf(" |");
    for (uint8_t v : p.outcome) printf(" %u", v);
    printf(" |");
    for (uint32_t id = 0; id < BGV_MAX_SIGPOOL; ++id)
      if (r.live[id]) {
        printf(" %u:%u:%u:", id, r.count[id], r.nbits[id]);
        print_hex(r.bits.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * id, sigpool_bits_bytes(r.nbits[id]));
      }
    printf("\n");
  }
  return 0;
}
