// Pool entries that hold a participation bitfield: the argument check of bits_of_set at submit and
// the copy it takes, the step's plan (which members are added, known or overlapping, in set order),
// its commit once the device's flags are back, and the bit concatenation of bgv_sigpool_sum.
// Host-only, no HIP types: a stand-alone CPU program runs it (tests/native/sigpoolbitssim.cpp), as
// bgv_sigpool_plan.h is run.
#pragma once
#include <string.h>

#include "bgv_sigpool_plan.h"

// The registry as these functions read it: SigPoolView's arrays, per id the number of bit positions
// (0: a plain entry) and BGV_MAX_SIGPOOL x BGV_SIGPOOL_BITS_BYTES of fields in SSZ bit order (bit k
// is bit k % 8 of byte k / 8), clear at and past n_bits.  bits may be NULL while no entry has any.
struct SigPoolBitsView {
  const uint8_t* live;
  const uint32_t* gen;
  const uint32_t* nbits;
  const uint8_t* bits;
};

// What the submit keeps of bits_of_set, so the caller need not: per set the entry's n_bits (0 for an
// untagged set or a plain entry) and either the single position or where its field starts in bytes.
struct SigPoolFields {
  std::vector<uint32_t> nbits, at;
  std::vector<uint8_t> single;
  std::vector<uint8_t> bytes;
};

struct SigPoolBitsPlan {
  SigPoolPlan plan;              // the members to add, as sigpool_plan lays them out
  std::vector<uint8_t> outcome;  // BGV_POOL_* per set
  // per touched entry (plan.ids order): whether it has bits, and its field after this call's
  // additions (BGV_SIGPOOL_BITS_BYTES each, zero for a plain entry)
  std::vector<uint8_t> has_bits, bits;
};

static inline size_t sigpool_bits_bytes(uint32_t n_bits) { return ((size_t)n_bits + 7) / 8; }

// The check of bits_of_set, after sigpool_check_tags has passed.  For every tagged set whose entry
// has bits: -BGV_E_ARG when bits_of_set is NULL, n_bits is not the entry's, the single position is
// not below n_bits, or the field has a bit at or past n_bits or none at all.  On BGV_OK f holds the
// copy.  bits_of_set[i] of any other set is not read beyond the struct itself.
static inline int sigpool_check_bits(const uint32_t* pool_of_set, const bgv_poolbits* bits_of_set, size_t nsets,
                                     const SigPoolBitsView& v, SigPoolFields* f) {
  f->nbits.assign(nsets, 0);
  f->at.assign(nsets, 0);
  f->single.assign(nsets, 0);
  f->bytes.clear();
  for (size_t i = 0; i < nsets; ++i) {
    const uint32_t id = pool_of_set[i];
    if (id == BGV_NO_AGG || v.nbits[id] == 0) continue;
    const uint32_t n = v.nbits[id];
    if (!bits_of_set || bits_of_set[i].n_bits != n) return -BGV_E_ARG;
    const bgv_poolbits& b = bits_of_set[i];
    f->nbits[i] = n;
    if (!b.bits) {
      if (b.bit >= n) return -BGV_E_ARG;
      f->single[i] = 1;
      f->at[i] = b.bit;
      continue;
    }
    const size_t nb = sigpool_bits_bytes(n);
    if ((n & 7) && (b.bits[nb - 1] >> (n & 7))) return -BGV_E_ARG;
    uint8_t any = 0;
    for (size_t k = 0; k < nb; ++k) any |= b.bits[k];
    if (!any) return -BGV_E_ARG;
    f->at[i] = (uint32_t)f->bytes.size();
    f->bytes.insert(f->bytes.end(), b.bits, b.bits + nb);
  }
  return BGV_OK;
}

// The step's plan.  A set is a candidate by sigpool_plan's rule (the code of its job is 1, it is
// tagged, its entry is live in the generation recorded at submit).  Candidates of a plain entry are
// added.  Those of an entry with bits are taken in set order against B, the entry's field as v has
// it plus what earlier sets of this call added, with M the member's field: M & B == 0 adds the
// member and B |= M; otherwise M within B is BGV_POOL_KNOWN, anything else BGV_POOL_OVERLAP.  Only
// the added ones enter p->plan, and the decoding form follows their number.
static inline void sigpool_plan_bits(const bgv_job* jobs, size_t njobs, const int32_t* codes,
                                     const uint32_t* pool_of_set, const uint32_t* gen_of_set, size_t nsets,
                                     const SigPoolBitsView& v, const SigPoolFields& f, size_t wave_max,
                                     SigPoolBitsPlan* p) {
  SigPoolPlan& q = p->plan;
  q.ids.clear();
  q.first.clear();
  q.count.clear();
  q.member.clear();
  q.form = SIGAGG_FORM_NONE;
  p->outcome.assign(nsets, BGV_POOL_NOT_ADDED);
  p->has_bits.clear();
  p->bits.clear();
  std::vector<uint8_t> take(nsets, 0);
  for (size_t j = 0; j < njobs; ++j) {
    if (codes[j] != 1) continue;
    for (uint32_t k = 0; k < jobs[j].n_sets; ++k) take[(size_t)jobs[j].first_set + k] = 1;
  }
  const uint32_t none = 0xFFFFFFFFu;
  std::vector<uint32_t> work_of(BGV_MAX_SIGPOOL, none), per_id(BGV_MAX_SIGPOOL, 0);
  std::vector<uint8_t> work;  // BGV_SIGPOOL_BITS_BYTES per entry with bits that has a candidate
  size_t n = 0;
  for (size_t i = 0; i < nsets; ++i) {
    const uint32_t id = pool_of_set[i];
    if (!(take[i] && id != BGV_NO_AGG && v.live[id] && v.gen[id] == gen_of_set[i])) {
      take[i] = 0;
      continue;
    }
    uint8_t out = BGV_POOL_ADDED;
    if (f.nbits[i]) {
      if (work_of[id] == none) {
        work_of[id] = (uint32_t)(work.size() / BGV_SIGPOOL_BITS_BYTES);
        const uint8_t* src = v.bits + (size_t)BGV_SIGPOOL_BITS_BYTES * id;
        work.insert(work.end(), src, src + BGV_SIGPOOL_BITS_BYTES);
      }
      uint8_t* B = work.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * work_of[id];
      if (f.single[i]) {
        const uint32_t b = f.at[i];
        if (B[b >> 3] >> (b & 7) & 1)
          out = BGV_POOL_KNOWN;
        else
          B[b >> 3] |= (uint8_t)(1u << (b & 7));
      } else {
        const uint8_t* M = f.bytes.data() + f.at[i];
        const size_t nb = sigpool_bits_bytes(f.nbits[i]);
        uint8_t common = 0, beyond = 0;
        for (size_t k = 0; k < nb; ++k) {
          common |= M[k] & B[k];
          beyond |= M[k] & (uint8_t)~B[k];
        }
        if (!common)
          for (size_t k = 0; k < nb; ++k) B[k] |= M[k];
        else
          out = beyond ? BGV_POOL_OVERLAP : BGV_POOL_KNOWN;
      }
    }
    p->outcome[i] = out;
    take[i] = out == BGV_POOL_ADDED;
    if (take[i]) {
      ++per_id[id];
      ++n;
    }
  }
  if (n == 0) return;
  std::vector<uint32_t> slot(BGV_MAX_SIGPOOL, 0);
  uint32_t at = 0;
  for (uint32_t id = 0; id < BGV_MAX_SIGPOOL; ++id)
    if (per_id[id]) {
      slot[id] = (uint32_t)q.ids.size();
      q.ids.push_back(id);
      q.first.push_back(at);
      q.count.push_back(per_id[id]);
      at += per_id[id];
      p->has_bits.push_back(work_of[id] != none);
      const size_t o = p->bits.size();
      p->bits.resize(o + BGV_SIGPOOL_BITS_BYTES, 0);
      if (work_of[id] != none)
        memcpy(p->bits.data() + o, work.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * work_of[id], BGV_SIGPOOL_BITS_BYTES);
    }
  q.member.resize(n);
  std::vector<uint32_t> fill(q.first);
  for (size_t i = 0; i < nsets; ++i)
    if (take[i]) q.member[fill[slot[pool_of_set[i]]]++] = (uint32_t)i;
  q.form = sigagg_form(n, wave_max);
}

// The commit, once flag[e] of every touched entry is back from the device: an entry whose flag is 0
// is marked written, counts its added members and takes its new field; one whose flag is not 0 keeps
// everything and all of its sets of this call, known and overlapping ones too, become
// BGV_POOL_NOT_ADDED in p->outcome.  written / count / bits: the registry's arrays.
static inline void sigpool_commit_bits(SigPoolBitsPlan* p, const int32_t* flag, const uint32_t* pool_of_set,
                                       size_t nsets, uint8_t* written, uint32_t* count, uint8_t* bits) {
  std::vector<uint32_t> flagged;
  for (size_t e = 0; e < p->plan.ids.size(); ++e) {
    const uint32_t id = p->plan.ids[e];
    if (flag[e] != BGV_OK) {
      flagged.push_back(id);
      continue;
    }
    written[id] = 1;
    count[id] += p->plan.count[e];
    if (p->has_bits[e])
      memcpy(bits + (size_t)BGV_SIGPOOL_BITS_BYTES * id, p->bits.data() + (size_t)BGV_SIGPOOL_BITS_BYTES * e,
             BGV_SIGPOOL_BITS_BYTES);
  }
  for (uint32_t id : flagged)
    for (size_t i = 0; i < nsets; ++i)
      if (pool_of_set[i] == id) p->outcome[i] = BGV_POOL_NOT_ADDED;
}

// bgv_sigpool_sum's concatenation: ORs the n low positions of src into dst from bit position off
// on (both in SSZ bit order).  dst holds at least ceil((off + n) / 8) bytes and is clear from off on.
static inline void sigpool_append_bits(uint8_t* dst, size_t off, const uint8_t* src, uint32_t n) {
  const size_t nb = sigpool_bits_bytes(n);
  const unsigned sh = (unsigned)(off & 7);
  uint8_t* d = dst + off / 8;
  for (size_t k = 0; k < nb; ++k) {
    unsigned s = src[k];
    if (k == nb - 1 && (n & 7)) s &= (1u << (n & 7)) - 1;
    d[k] |= (uint8_t)(s << sh);
    const unsigned hi = s >> (8 - sh);  // sh == 0: s >> 8 == 0
    if (hi) d[k + 1] |= (uint8_t)hi;
  }
}
