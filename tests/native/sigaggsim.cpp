// CPU driver of bgv_verify_aggregate's host plan (lodestar_amd/csrc/bgv_sigagg_plan.h): reads
// cases from stdin, prints each plan.  Test infrastructure only (tests/sigaggsim.py).
//
//   stdin:  T, then per case:  njobs nsets naggs wave_max
//                              njobs x (first_set n_sets code)
//                              nsets x tag
//   stdout: per case one line: rc form n | first[naggs] | count[naggs] | member[n]
//           (rc: sigagg_check_tags'; when it is not 0 the line ends after it)
//   `consts` as the only argument prints BGV_NO_AGG, BGV_SIGAGG_WAVE_MAX and the largest naggs.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../lodestar_amd/csrc/bgv_sigagg_plan.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "consts")) {
    printf("%u %u %u\n", BGV_NO_AGG, (unsigned)BGV_SIGAGG_WAVE_MAX, (unsigned)BGV_SIGAGG_MAX_AGGS);
    return 0;
  }
  unsigned T = 0;
  if (scanf("%u", &T) != 1) return 2;
  for (unsigned t = 0; t < T; ++t) {
    unsigned long njobs, nsets, naggs, wave_max;
    if (scanf("%lu %lu %lu %lu", &njobs, &nsets, &naggs, &wave_max) != 4) return 2;
    std::vector<bgv_job> jobs(njobs);
    std::vector<int32_t> codes(njobs);
    for (size_t j = 0; j < njobs; ++j) {
      jobs[j].batchable = 1;
      if (scanf("%u %u %d", &jobs[j].first_set, &jobs[j].n_sets, &codes[j]) != 3) return 2;
      if ((size_t)jobs[j].first_set + jobs[j].n_sets > nsets) return 3;
    }
    // exactly nsets tags on the heap: the sanitized build sees any read past them
    std::vector<uint32_t> tags(nsets);
    for (size_t i = 0; i < nsets; ++i)
      if (scanf("%u", &tags[i]) != 1) return 2;
    const int rc = sigagg_check_tags(tags.data(), nsets, naggs);
    if (rc != BGV_OK) {
      printf("%d\n", rc);
      continue;
    }
    SigAggPlan p;
    sigagg_plan(jobs.data(), njobs, codes.data(), tags.data(), nsets, naggs, wave_max, &p);
    printf("0 %d %zu |", p.form, p.member.size());
    for (uint32_t v : p.first) printf(" %u", v);
    printf(" |");
    for (uint32_t v : p.count) printf(" %u", v);
    printf(" |");
    for (uint32_t v : p.member) printf(" %u", v);
    printf("\n");
  }
  return 0;
}
