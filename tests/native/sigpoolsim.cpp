// CPU driver of bgv_verify_accumulate's host plan (lodestar_amd/csrc/bgv_sigpool_plan.h): reads
// cases from stdin, prints each tag check and plan.  Test infrastructure only (tests/sigpoolsim.py).
//
//   stdin:  T, then per case:  njobs nsets nlive nchanged wave_max
//                              njobs x (first_set n_sets code)
//                              nsets x tag
//                              nlive x (id generation)       the registry at submit
//                              nchanged x (id live generation)  what changed before the step
//   stdout: per case one line: rc form n | ids[e] | first[e] | count[e] | member[n] | gen_of_set[nsets]
//           (rc: sigpool_check_tags'; when it is not 0 the line ends after it)
//   `consts` as the only argument prints BGV_NO_AGG, BGV_SIGAGG_WAVE_MAX and BGV_MAX_SIGPOOL.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../lodestar_amd/csrc/bgv_sigpool_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "consts")) {
    printf("%u %u %u\n", BGV_NO_AGG, (unsigned)BGV_SIGAGG_WAVE_MAX, (unsigned)BGV_MAX_SIGPOOL);
    return 0;
  }
  unsigned T = 0;
  if (scanf("%u", &T) != 1) return 2;
  for (unsigned t = 0; t < T; ++t) {
    unsigned long njobs, nsets, nlive, nchanged, wave_max;
    if (scanf("%lu %lu %lu %lu %lu", &njobs, &nsets, &nlive, &nchanged, &wave_max) != 5) return 2;
    std::vector<bgv_job> jobs(njobs);
    std::vector<int32_t> codes(njobs);
    for (size_t j = 0; j < njobs; ++j) {
      jobs[j].batchable = 1;
      if (scanf("%u %u %d", &jobs[j].first_set, &jobs[j].n_sets, &codes[j]) != 3) return 2;
      if ((size_t)jobs[j].first_set + jobs[j].n_sets > nsets) return 3;
    }
    // exactly nsets tags and BGV_MAX_SIGPOOL registry entries on the heap: the sanitized build
    // sees any read past them
    std::vector<uint32_t> tags(nsets);
    for (size_t i = 0; i < nsets; ++i)
      if (scanf("%u", &tags[i]) != 1) return 2;
    std::vector<uint8_t> live(BGV_MAX_SIGPOOL, 0);
    std::vector<uint32_t> gen(BGV_MAX_SIGPOOL, 0);
    for (size_t k = 0; k < nlive; ++k) {
      unsigned id, g;
      if (scanf("%u %u", &id, &g) != 2 || id >= BGV_MAX_SIGPOOL) return 2;
      live[id] = 1;
      gen[id] = g;
    }
    std::vector<uint32_t> gen_of_set;
    const int rc = sigpool_check_tags(tags.data(), nsets, SigPoolView{live.data(), gen.data()}, &gen_of_set);
    for (size_t k = 0; k < nchanged; ++k) {
      unsigned id, l, g;
      if (scanf("%u %u %u", &id, &l, &g) != 3 || id >= BGV_MAX_SIGPOOL) return 2;
      live[id] = l != 0;
      gen[id] = g;
    }
    if (rc != BGV_OK) {
      printf("%d\n", rc);
      continue;
    }
    SigPoolPlan p;
    sigpool_plan(jobs.data(), njobs, codes.data(), tags.data(), gen_of_set.data(), nsets,
                 SigPoolView{live.data(), gen.data()}, wave_max, &p);
    printf("0 %d %zu |", p.form, p.member.size());
    for (uint32_t v : p.ids) printf(" %u", v);
    printf(" |");
    for (uint32_t v : p.first) printf(" %u", v);
    printf(" |");
    for (uint32_t v : p.count) printf(" %u", v);
    printf(" |");
    for (uint32_t v : p.member) printf(" %u", v);
    printf(" |");
    for (uint32_t v : gen_of_set) printf(" %u", v);
    printf("\n");
  }
  return 0;
}
