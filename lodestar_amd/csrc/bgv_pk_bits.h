// Committee-bitfield pubkey sets: which members of a device-resident committee a set's
// bitfield selects, and which side of the committee gets summed.  Plain host/device functions
// (no HIP types): k_pk_agg_bits (bgv_k_prep.hip) runs them per lane, the host layout
// (bgv_host_layout.h) takes the mode decision, tests/native/committeesim.cpp runs both on a CPU.
// Below them the same for spans, one bitfield over several committees (k_pk_agg_span,
// tests/native/multicomsim.cpp).
//
// A committee of n members (validator indices kept on the device with their pubkey sum,
// bgv_committee_put) and an SSZ bitfield: member p takes part iff (bits[p >> 3] >> (p & 7)) & 1.
// The bitfield travels as ceil(n / 32) little-endian 32-bit words.  With k bits set the set's
// aggregate is either the sum of the k members whose bit is set (direct) or the committee's
// total minus the sum of the n - k members whose bit is clear (complement): the same group
// element, so the side with fewer point additions is taken.
#pragma once
#include <stdint.h>

#ifndef BGV_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BGV_HD __host__ __device__ __forceinline__
#else
#define BGV_HD inline __attribute__((always_inline))
#endif
#endif

// the chosen side has at most this many terms: a 16-lane team sums it, a whole wave above
// (the same threshold as k_pk_agg16 / k_pk_agg, bgv_device.h)
#ifndef BGV_PK_TEAM_MAX
#define BGV_PK_TEAM_MAX 256
#endif

// The direct sum gathers k keys (k - 1 additions on one lane, k with the start at infinity);
// the complement gathers n - k keys and adds once more, the subtraction from the total.
BGV_HD bool pkb_use_complement(uint32_t n, uint32_t k) { return n - k + 1 < k; }
// terms gathered on the chosen side
BGV_HD uint32_t pkb_terms(uint32_t n, uint32_t k, bool complement) { return complement ? n - k : k; }
BGV_HD uint32_t pkb_nwords(uint32_t n) { return (n + 31u) / 32u; }

BGV_HD uint32_t pkb_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}

// Word w of the selection: the bitfield's word (null words: every bit set, the committee's
// total), inverted in complement mode, without the positions at and past n.
BGV_HD uint32_t pkb_word(const uint32_t* words, uint32_t n, bool complement, uint32_t w) {
  uint32_t v = words ? words[w] : 0xFFFFFFFFu;
  if (complement) v = ~v;
  const uint32_t rem = n - 32u * w;  // members from this word on (w < pkb_nwords(n): rem >= 1)
  return rem >= 32u ? v : v & ((1u << rem) - 1u);
}

// position of the r-th set bit of v, r < popcount(v)
BGV_HD uint32_t pkb_select(uint32_t v, uint32_t r) {
  for (uint32_t i = 0; i < r; ++i) v &= v - 1u;
  return (uint32_t)__builtin_ctz(v);
}

// One lane's walk over the selection by RANK: lane l of a team of T lanes takes the selected
// members of rank l, l + T, l + 2T, ... (rank = number of selected members before it), so a
// lane's number of additions is ceil((m - l) / T) whatever the bit pattern.  The cursor keeps the
// next word to look at, the per-word popcount prefix before it and the rank wanted next.
struct pkb_cursor {
  uint32_t w;     // next word to scan
  uint32_t base;  // selected members in the words before w
  uint32_t want;  // rank of the lane's next member
};
BGV_HD pkb_cursor pkb_begin(uint32_t lane) { return pkb_cursor{0u, 0u, lane}; }
// true and *pos = the member position of rank c.want, then c.want += T; false when the
// selection has no member of that rank
BGV_HD bool pkb_next(pkb_cursor& c, const uint32_t* words, uint32_t n, bool complement, uint32_t T, uint32_t* pos) {
  const uint32_t W = pkb_nwords(n);
  while (c.w < W) {
    const uint32_t v = pkb_word(words, n, complement, c.w);
    const uint32_t cnt = pkb_popc(v);
    if (c.want < c.base + cnt) {
      *pos = 32u * c.w + pkb_select(v, c.want - c.base);
      c.want += T;
      return true;
    }
    c.base += cnt;
    ++c.w;
  }
  return false;
}

// ---------------------------------------------------------------------------------------------
// Spans: one bitfield laid over several committees (blsgpu.h bgv_pkspan).  Committee c owns the
// bits [off_c, off_c + n_c) of the bitfield, off_c the sum of the lengths before it, so its words
// start at any bit position.  The host cuts the bitfield at the committee edges: per committee
// the side pkb_use_complement(n_c, k_c) gives, its selection words as pkb_word forms them
// (inverted on the complement side, nothing at or past n_c), and of those only the words that
// select somebody.  The slot's run in the index array:
//
//   [0] R   selection records          [1] Q   committees on the complement side
//   [2] M   terms (below)
//   [3 .. 3 + Q)                       the complement committees' directory handles
//   then R records {selection word, pkb_span_meta(handle, word number in its committee, side)}
//
// The set's sum is  sum_direct(selected) + sum_complement(total_c - unselected): a term list of
// M = sum_c pkb_terms(n_c, k_c, side_c) + Q terms -- the selected members of every record in
// order, negated where the record's committee is on the complement side, then the Q totals --
// which a team walks by RANK over the whole list as pkb_next does over one committee.  A
// committee with k_c = 0 leaves no record; one with k_c = n_c (> 1) only its total.
BGV_HD uint32_t pkb_span_meta(uint32_t handle, uint32_t w, bool complement) {
  return handle | (w << 15) | (complement ? 0x80000000u : 0u);  // handle < 2^15 (kComHandles), w < 2^11
}
BGV_HD uint32_t pkb_meta_handle(uint32_t meta) { return meta & 0x7FFFu; }
BGV_HD uint32_t pkb_meta_word(uint32_t meta) { return (meta >> 15) & 0xFFFFu; }
BGV_HD bool pkb_meta_complement(uint32_t meta) { return (meta >> 31) != 0u; }

// 32 bits of an SSZ bitfield of nbytes bytes from bit position `at` on (zero past its end)
BGV_HD uint32_t pkb_bits_at(const uint8_t* bits, uint32_t nbytes, uint32_t at) {
  const uint32_t b = at >> 3;
  uint64_t v = 0;
  for (uint32_t q = 0; q < 5u; ++q)
    if (b + q < nbytes) v |= (uint64_t)bits[b + q] << (8u * q);
  return (uint32_t)(v >> (at & 7u));
}
// Word w of the selection of a committee of n members whose first bit is bit `off` of the
// bitfield: masked exactly as pkb_word masks a committee's own word
BGV_HD uint32_t pkb_span_word(const uint8_t* bits, uint32_t nbytes, uint32_t off, uint32_t n, bool complement,
                              uint32_t w) {
  const uint32_t v = pkb_bits_at(bits, nbytes, off + 32u * w);
  return pkb_word(&v, n - 32u * w, complement, 0u);
}
// members of that committee whose bit is set
BGV_HD uint32_t pkb_span_count(const uint8_t* bits, uint32_t nbytes, uint32_t off, uint32_t n) {
  uint32_t k = 0;
  for (uint32_t w = 0; w < pkb_nwords(n); ++w) k += pkb_popc(pkb_span_word(bits, nbytes, off, n, false, w));
  return k;
}

// One committee of a span as the host knows it: its directory handle, its length and how many of
// its members the bitfield selects.
#define PKB_SPAN_HEAD 3u  // R, Q, M
struct pkb_part {
  uint32_t handle, n, k;
};
// The run of a span (above) through push(word); returns M, its number of terms.
template <class Push>
inline uint32_t pkb_span_build(const pkb_part* parts, uint32_t nc, const uint8_t* bits, uint32_t nbytes, Push push) {
  uint32_t nrec = 0, ncomp = 0, m = 0, off = 0;
  for (uint32_t c = 0; c < nc; off += parts[c].n, ++c) {
    const bool comp = pkb_use_complement(parts[c].n, parts[c].k);
    ncomp += comp ? 1u : 0u;
    m += pkb_terms(parts[c].n, parts[c].k, comp) + (comp ? 1u : 0u);
    for (uint32_t w = 0; w < pkb_nwords(parts[c].n); ++w)
      nrec += pkb_span_word(bits, nbytes, off, parts[c].n, comp, w) != 0u ? 1u : 0u;
  }
  push(nrec);
  push(ncomp);
  push(m);
  for (uint32_t c = 0; c < nc; ++c)
    if (pkb_use_complement(parts[c].n, parts[c].k)) push(parts[c].handle);
  off = 0;
  for (uint32_t c = 0; c < nc; off += parts[c].n, ++c) {
    const bool comp = pkb_use_complement(parts[c].n, parts[c].k);
    for (uint32_t w = 0; w < pkb_nwords(parts[c].n); ++w) {
      const uint32_t v = pkb_span_word(bits, nbytes, off, parts[c].n, comp, w);
      if (v == 0u) continue;
      push(v);
      push(pkb_span_meta(parts[c].handle, w, comp));
    }
  }
  return m;
}

// One lane's walk over a span's member terms by rank, as pkb_next: true, *meta = the record's
// second word and *pos = the member's position in its committee for the term of rank c.want,
// then c.want += T.  false: no member term of that rank; c.base is then the number of member
// terms, and the lane's totals are those of rank c.want - c.base, + T, ... below Q.
struct pkb_span_cursor {
  uint32_t j;     // next record to look at
  uint32_t base;  // member terms in the records before j
  uint32_t want;  // rank of the lane's next term
};
BGV_HD pkb_span_cursor pkb_span_begin(uint32_t lane) { return pkb_span_cursor{0u, 0u, lane}; }
BGV_HD bool pkb_span_next(pkb_span_cursor& c, const uint32_t* recs, uint32_t nrec, uint32_t T, uint32_t* meta,
                          uint32_t* pos) {
  while (c.j < nrec) {
    const uint32_t v = recs[2u * c.j];
    const uint32_t cnt = pkb_popc(v);
    if (c.want < c.base + cnt) {
      *meta = recs[2u * c.j + 1u];
      *pos = 32u * pkb_meta_word(*meta) + pkb_select(v, c.want - c.base);
      c.want += T;
      return true;
    }
    c.base += cnt;
    ++c.j;
  }
  return false;
}
