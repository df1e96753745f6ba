// bgv_verify_accumulate's host plan: the tag check of a call against the pool's registry, the
// generations it records at submit, and, once the codes are final, which sets are added to which
// entry and in which decoding form.  Host-only, no HIP types: a stand-alone CPU program runs it
// (tests/native/sigpoolsim.cpp), as bgv_sigagg_plan.h is run.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bgv_sigagg_plan.h"  // sigagg_form and the forms: one threshold for both steps

// The registry as the plan reads it: BGV_MAX_SIGPOOL entries each.  An id's generation changes
// every time it is opened, so (live, generation) names one life of an entry.
struct SigPoolView {
  const uint8_t* live;
  const uint32_t* gen;
};

struct SigPoolPlan {
  // the touched entries in ascending id; entry ids[e]'s sets are member[first[e] .. first[e] +
  // count[e]), in set order
  std::vector<uint32_t> ids, first, count, member;
  int form = SIGAGG_FORM_NONE;
};

// The argument check of pool_of_set at submit.  -BGV_E_ARG when any tag is neither BGV_NO_AGG nor
// below BGV_MAX_SIGPOOL (whatever the verdict of its set will be); otherwise -BGV_E_BAD_INDEX when
// any tag names an entry that is not live.  On BGV_OK gen_of_set[i] is the generation of set i's
// entry as it stands now (0 for an untagged set).
static inline int sigpool_check_tags(const uint32_t* pool_of_set, size_t nsets, const SigPoolView& v,
                                     std::vector<uint32_t>* gen_of_set) {
  if (nsets && !pool_of_set) return -BGV_E_ARG;
  for (size_t i = 0; i < nsets; ++i)
    if (pool_of_set[i] != BGV_NO_AGG && pool_of_set[i] >= BGV_MAX_SIGPOOL) return -BGV_E_ARG;
  for (size_t i = 0; i < nsets; ++i)
    if (pool_of_set[i] != BGV_NO_AGG && !v.live[pool_of_set[i]]) return -BGV_E_BAD_INDEX;
  gen_of_set->assign(nsets, 0);
  for (size_t i = 0; i < nsets; ++i)
    if (pool_of_set[i] != BGV_NO_AGG) (*gen_of_set)[i] = v.gen[pool_of_set[i]];
  return BGV_OK;
}

// Set i is added iff the code of the job that holds it is 1 (sigagg_plan's rule: a set no job
// holds is not accepted, a set several jobs hold is accepted once), it is tagged, and its entry is
// live with the generation recorded at submit.  The tags have passed sigpool_check_tags; v is the
// registry as it stands at the step.  A counting sort by id keeps set order inside an entry.
static inline void sigpool_plan(const bgv_job* jobs, size_t njobs, const int32_t* codes, const uint32_t* pool_of_set,
                                const uint32_t* gen_of_set, size_t nsets, const SigPoolView& v, size_t wave_max,
                                SigPoolPlan* p) {
  p->ids.clear();
  p->first.clear();
  p->count.clear();
  p->member.clear();
  p->form = SIGAGG_FORM_NONE;
  std::vector<uint8_t> take(nsets, 0);
  for (size_t j = 0; j < njobs; ++j) {
    if (codes[j] != 1) continue;
    for (uint32_t k = 0; k < jobs[j].n_sets; ++k) take[(size_t)jobs[j].first_set + k] = 1;
  }
  std::vector<uint32_t> per_id(BGV_MAX_SIGPOOL, 0);
  size_t n = 0;
  for (size_t i = 0; i < nsets; ++i) {
    const uint32_t id = pool_of_set[i];
    take[i] = take[i] && id != BGV_NO_AGG && v.live[id] && v.gen[id] == gen_of_set[i];
    if (take[i]) {
      ++per_id[id];
      ++n;
    }
  }
  if (n == 0) return;
  std::vector<uint32_t> slot(BGV_MAX_SIGPOOL, 0);  // the entry's place among the touched ones
  uint32_t at = 0;
  for (uint32_t id = 0; id < BGV_MAX_SIGPOOL; ++id)
    if (per_id[id]) {
      slot[id] = (uint32_t)p->ids.size();
      p->ids.push_back(id);
      p->first.push_back(at);
      p->count.push_back(per_id[id]);
      at += per_id[id];
    }
  p->member.resize(n);
  std::vector<uint32_t> fill(p->first);
  for (size_t i = 0; i < nsets; ++i)
    if (take[i]) p->member[fill[slot[pool_of_set[i]]]++] = (uint32_t)i;
  p->form = sigagg_form(n, wave_max);
}
