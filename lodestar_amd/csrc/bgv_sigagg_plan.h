// bgv_verify_aggregate's host plan: which sets a call accepted, grouped by the aggregate each
// belongs to, and which decoding form the aggregation step takes.  Host-only, no HIP types: a
// stand-alone CPU program runs it (tests/native/sigaggsim.cpp), as bgv_retry_plan.h and
// bgv_pk_bits.h are run.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/blsgpu.h"

#define BGV_SIGAGG_MAX_AGGS (1u << 20)

// the decoding form of a call (bgv_k_sigagg.hip)
enum { SIGAGG_FORM_NONE = 0, SIGAGG_FORM_WAVE = 1, SIGAGG_FORM_BULK = 2 };

struct SigAggPlan {
  // aggregate a's accepted sets are member[first[a] .. first[a] + count[a]), in set order
  std::vector<uint32_t> first, count, member;
  int form = SIGAGG_FORM_NONE;
};

// The argument check of agg_of_set: every tag is BGV_NO_AGG or below naggs (naggs at most 2^20).
static inline int sigagg_check_tags(const uint32_t* agg_of_set, size_t nsets, size_t naggs) {
  if (naggs > BGV_SIGAGG_MAX_AGGS) return -BGV_E_ARG;
  if (naggs == 0) return BGV_OK;  // the tags are not read: bgv_verify_spans
  if (nsets && !agg_of_set) return -BGV_E_ARG;
  for (size_t i = 0; i < nsets; ++i)
    if (agg_of_set[i] != BGV_NO_AGG && agg_of_set[i] >= naggs) return -BGV_E_ARG;
  return BGV_OK;
}

// The decoding form for n accepted signatures: one per wavefront up to wave_max, one per lane above.
static inline int sigagg_form(size_t n, size_t wave_max) {
  return n == 0 ? SIGAGG_FORM_NONE : n <= wave_max ? SIGAGG_FORM_WAVE : SIGAGG_FORM_BULK;
}

// Set i is accepted iff the code of the job that holds it is 1 (a set no job holds is not; a set
// that several jobs hold is accepted once, if any of them is).  The jobs lie within nsets and the
// tags have passed sigagg_check_tags.  A counting sort by aggregate keeps set order inside one.
static inline void sigagg_plan(const bgv_job* jobs, size_t njobs, const int32_t* codes, const uint32_t* agg_of_set,
                               size_t nsets, size_t naggs, size_t wave_max, SigAggPlan* p) {
  p->first.assign(naggs, 0);
  p->count.assign(naggs, 0);
  p->member.clear();
  p->form = SIGAGG_FORM_NONE;
  if (naggs == 0) return;
  std::vector<uint8_t> accepted(nsets, 0);
  for (size_t j = 0; j < njobs; ++j) {
    if (codes[j] != 1) continue;
    for (uint32_t k = 0; k < jobs[j].n_sets; ++k) accepted[(size_t)jobs[j].first_set + k] = 1;
  }
  size_t n = 0;
  for (size_t i = 0; i < nsets; ++i)
    if (accepted[i] && agg_of_set[i] != BGV_NO_AGG) {
      ++p->count[agg_of_set[i]];
      ++n;
    }
  uint32_t at = 0;
  for (size_t a = 0; a < naggs; ++a) {
    p->first[a] = at;
    at += p->count[a];
  }
  p->member.resize(n);
  std::vector<uint32_t> fill(p->first);
  for (size_t i = 0; i < nsets; ++i)
    if (accepted[i] && agg_of_set[i] != BGV_NO_AGG) p->member[fill[agg_of_set[i]]++] = (uint32_t)i;
  p->form = sigagg_form(n, wave_max);
}
