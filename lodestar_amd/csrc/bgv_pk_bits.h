// Committee-bitfield pubkey sets: which members of a device-resident committee a set's
// bitfield selects, and which side of the committee gets summed.  Plain host/device functions
// (no HIP types): k_pk_agg_bits (bgv_k_prep.hip) runs them per lane, the host layout
// (bgv_host_layout.h) takes the mode decision, tests/native/committeesim.cpp runs both on a CPU.
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
