// Balance-weighted sampling (bgv_proposers, bgv_sync_committee_put): computeProposerIndex and
// getNextSyncCommitteeIndices (state-transition/src/util/seed.ts).  Plain host/device functions
// (no HIP types) over bgv_shuffle.h's swap-or-not arithmetic: k_sample_eval / k_sample_pick
// (bgv_k_sample.hip) run them per thread, the host (bgv_registry.cpp) runs the pass loop at the
// end of this file, and tests/native/samplesim.cpp (byte rule) and samplesim_electra.cpp (16-bit
// rule) run all of it on a CPU.
//
// Candidate i = 0, 1, 2, ... of a seed over n active indices:
//   v_i    = active[compute_shuffled_index(i mod n, n, seed)]
//   byte_i = sha256(seed | LE64(i div 32))[i mod 32]            (40 bytes, one block)
//   accepted iff eff[v_i] * 255 >= max_incr * byte_i
// and the first `want` accepted candidates, in order, are the seed's picks.  Candidates are
// examined a WINDOW at a time: every candidate of the window is evaluated (one thread each), then
// an ordered compaction appends the accepted ones to the picks.  A seed that is still short gets a
// further window; no candidate at or past `limit` is ever accepted, which bounds the work.
//
// That is the BYTE rule (phase0 .. Deneb).  The U16 rule (Electra, EIP-7251) draws 16 bits:
//   rand_i = LE16(sha256(seed | LE64(i div 16))[2 (i mod 16) ..])   (16 candidates per digest)
//   accepted iff eff[v_i] * 65535 >= max_incr * rand_i              (eff: uint16_t per validator)
// Only the draw, the table's element and the acceptance test differ (samp_rule8 / samp_rule16
// below); the walk, the pivots, the compaction, the pass loop, the cap and the limit are shared.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bgv_shuffle.h"

#define BGV_SAMPLE_BLOCK 256u       // candidates per block of k_sample_eval, threads per block of both kernels
#define BGV_SAMPLE_WAVE 64u         // lanes per ballot
#define BGV_SAMPLE_CAP 65536u       // BGV_SAMPLE_MAX_TRIES: candidates examined per seed, at most
#define BGV_SAMPLE_MAX_SEEDS 1024u
#define BGV_SAMPLE_MAX_WANT 65536u
#define BGV_SAMPLE_PASS_ITEMS (1u << 22)  // candidates of one pass over all its seeds, at most (20 MB of results)

// which acceptance rule a call samples by (bgv_sample_in::rule)
enum samp_rule_id : uint32_t { SAMP_RULE_BYTE = 0, SAMP_RULE_U16 = 1 };

// a seed's progress, kept on the device between passes
struct samp_state {
  uint32_t have;  // picks so far (<= want)
  uint32_t next;  // the next candidate number: a multiple of BGV_SAMPLE_BLOCK until the limit is reached
};

// ---------------------------------------------------------------------------
// per candidate
// ---------------------------------------------------------------------------
// sha256(seed | LE64(q)): the random bytes of candidates 32 q .. 32 q + 31 (byte rule), or of
// candidates 16 q .. 16 q + 15, two bytes each (16-bit rule)
BGV_HD void samp_hash_rand(uint32_t out[8], const shuf_seed& s, uint64_t q) {
  uint32_t blk[16];
  BGV_UNROLL for (int j = 0; j < 8; ++j) blk[j] = s.w[j];
  blk[8] = shuf_bswap((uint32_t)q);
  blk[9] = shuf_bswap((uint32_t)(q >> 32));
  blk[10] = 0x80u << 24;
  BGV_UNROLL for (int j = 11; j < 15; ++j) blk[j] = 0;
  blk[15] = 40u * 8u;
  sha256_init(out);
  sha256_compress(out, blk);
}
// byte k (< 32) of a digest held as SHA-256's 8 big-endian words
BGV_HD uint32_t samp_digest_byte(const uint32_t* d, uint32_t k) { return (d[k >> 2] >> (24u - 8u * (k & 3u))) & 0xffu; }

// compute_shuffled_index(i, n, seed) with every round's digest hashed on the spot: the pivots in
// piv[0 .. rounds), per round one shuf_hash_block and one bit test.  No table (bgv_shuffle.h's
// costs rounds * n / 256 digests per seed); the cost is rounds digests per candidate.
BGV_HD uint32_t samp_walk(uint32_t i, uint32_t n, uint32_t rounds, const shuf_seed& s, const uint32_t* piv) {
  if (n < 2) return i;
  BGV_NO_UNROLL for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t x = piv[r] + n - i;  // 1 .. 2n - 1
    const uint32_t flip = x >= n ? x - n : x;
    const uint32_t pos = i > flip ? i : flip;
    uint32_t d[8];
    shuf_hash_block(d, s, r, pos >> 8);
    const uint32_t k = (pos & 255u) >> 5;  // the word of the bit, picked without indexing registers
    uint32_t w = d[0];
    BGV_UNROLL for (uint32_t j = 1; j < 8; ++j) w = k == j ? d[j] : w;
    // bit (pos & 7) of byte (pos >> 3) & 3 of the big-endian word
    const uint32_t bit = (w >> (24u - 8u * ((pos >> 3) & 3u) + (pos & 7u))) & 1u;
    i = bit ? flip : i;
  }
  return i;
}

BGV_HD bool samp_accept(uint32_t eff, uint32_t max_incr, uint32_t byte) { return eff * 255u >= max_incr * byte; }

// 16-bit value k (< 16) of a digest held as SHA-256's 8 big-endian words: d[2k] | d[2k+1] << 8 of
// its bytes, which is one half-word of word k / 2 with its two bytes swapped.  The word is picked
// without indexing registers, as samp_walk picks its bit's word.
BGV_HD uint32_t samp_digest_u16(const uint32_t* d, uint32_t k) {
  const uint32_t j = k >> 1;
  uint32_t w = d[0];
  BGV_UNROLL for (uint32_t m = 1; m < 8; ++m) w = j == m ? d[m] : w;
  const uint32_t h = (w >> (16u - 16u * (k & 1u))) & 0xffffu;  // bytes 2k (high) and 2k+1 (low)
  return (h >> 8) | ((h & 0xffu) << 8);
}
// eff, max_incr and rand are all at most 65535, so both products fit 32 bits:
// 65535 * 65535 = 4294836225 < 2^32 = 4294967296.
BGV_HD bool samp_accept16(uint32_t eff, uint32_t max_incr, uint32_t rand) { return eff * 65535u >= max_incr * rand; }

// The two rules: what depends on the draw, and nothing else.
struct samp_rule8 {
  typedef uint8_t eff_t;
  static constexpr uint32_t SHIFT = 5;  // log2 of the candidates one digest serves
  static constexpr uint32_t MAX_INCR = 255;
  static BGV_HD uint32_t draw(const uint32_t* d, uint32_t k) { return samp_digest_byte(d, k); }
  static BGV_HD bool accept(uint32_t eff, uint32_t max_incr, uint32_t r) { return samp_accept(eff, max_incr, r); }
};
struct samp_rule16 {
  typedef uint16_t eff_t;
  static constexpr uint32_t SHIFT = 4;
  static constexpr uint32_t MAX_INCR = 65535;
  static BGV_HD uint32_t draw(const uint32_t* d, uint32_t k) { return samp_digest_u16(d, k); }
  static BGV_HD bool accept(uint32_t eff, uint32_t max_incr, uint32_t r) { return samp_accept16(eff, max_incr, r); }
};
// digests behind the draws of one block's BGV_SAMPLE_BLOCK candidates: 8 (byte rule), 16 (16-bit rule)
template <class R>
constexpr uint32_t samp_rand_digests() {
  return BGV_SAMPLE_BLOCK >> R::SHIFT;
}

// What one block of k_sample_eval shares: the seed's pivots and the digests of the draws of its
// BGV_SAMPLE_BLOCK candidates base .. base + 255 (base a multiple of 256, hence of 32 and of 16).
// Thread t's part.
template <class R>
BGV_HD void samp_setup_item_r(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t base, uint32_t* piv,
                              uint32_t* rnd /* samp_rand_digests<R>() x 8 words */) {
  constexpr uint32_t ND = samp_rand_digests<R>();
  if (t < rounds && n >= 2) piv[t] = shuf_pivot(s, t, n);
  // the last threads of the block: with the usual 90 rounds they hash no pivot
  if (t >= BGV_SAMPLE_BLOCK - ND && t < BGV_SAMPLE_BLOCK) {
    const uint32_t j = t - (BGV_SAMPLE_BLOCK - ND);
    uint32_t d[8];
    samp_hash_rand(d, s, (uint64_t)(base >> R::SHIFT) + j);
    BGV_UNROLL for (int w = 0; w < 8; ++w) rnd[8u * j + w] = d[w];
  }
}
// Candidate base + t: its validator index into *v, and whether it is accepted (never at or past limit).
template <class R>
BGV_HD bool samp_eval_item_r(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t base, uint32_t limit,
                             const uint32_t* piv, const uint32_t* rnd, const uint32_t* active,
                             const typename R::eff_t* eff, uint32_t max_incr, uint32_t* v) {
  const uint32_t i = base + t;
  *v = active[samp_walk(i % n, n, rounds, s, piv)];
  const uint32_t r = R::draw(rnd + 8u * ((i >> R::SHIFT) - (base >> R::SHIFT)), i & ((1u << R::SHIFT) - 1u));
  return i < limit && R::accept(eff[*v], max_incr, r);
}

// the byte rule under its own names
#define BGV_SAMPLE_RAND_DIGESTS (BGV_SAMPLE_BLOCK / 32u)
BGV_HD void samp_setup_item(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t base, uint32_t* piv,
                            uint32_t* rnd /* BGV_SAMPLE_RAND_DIGESTS x 8 words */) {
  samp_setup_item_r<samp_rule8>(t, s, n, rounds, base, piv, rnd);
}
BGV_HD bool samp_eval_item(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t base, uint32_t limit,
                           const uint32_t* piv, const uint32_t* rnd, const uint32_t* active, const uint8_t* eff,
                           uint32_t max_incr, uint32_t* v) {
  return samp_eval_item_r<samp_rule8>(t, s, n, rounds, base, limit, piv, rnd, active, eff, max_incr, v);
}
// ... and the 16-bit rule
#define BGV_SAMPLE_RAND_DIGESTS16 (BGV_SAMPLE_BLOCK / 16u)
BGV_HD void samp_setup_item16(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t base,
                              uint32_t* piv, uint32_t* rnd /* BGV_SAMPLE_RAND_DIGESTS16 x 8 words */) {
  samp_setup_item_r<samp_rule16>(t, s, n, rounds, base, piv, rnd);
}
BGV_HD bool samp_eval_item16(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t base,
                             uint32_t limit, const uint32_t* piv, const uint32_t* rnd, const uint32_t* active,
                             const uint16_t* eff, uint32_t max_incr, uint32_t* v) {
  return samp_eval_item_r<samp_rule16>(t, s, n, rounds, base, limit, piv, rnd, active, eff, max_incr, v);
}
static_assert(samp_rand_digests<samp_rule8>() == BGV_SAMPLE_RAND_DIGESTS &&
                  samp_rand_digests<samp_rule16>() == BGV_SAMPLE_RAND_DIGESTS16,
              "a block's digests follow from the candidates one digest serves");

// ---------------------------------------------------------------------------
// ordered compaction (k_sample_pick)
// ---------------------------------------------------------------------------
// Where the candidate of `lane` goes among its seed's picks, given the ballot of its wave's accept
// flags and how many were accepted before the wave (earlier passes, chunks and waves); `want`: nowhere.
BGV_HD uint32_t samp_pick_dst(uint64_t ballot, uint32_t lane, uint32_t before, uint32_t want) {
  if (!((ballot >> lane) & 1u)) return want;
  const uint64_t lower = ballot & ((uint64_t(1) << lane) - 1u);
  const uint64_t dst = (uint64_t)before + (uint32_t)__builtin_popcountll(lower);
  return dst < want ? (uint32_t)dst : want;
}

// ---------------------------------------------------------------------------
// pass planning (host only)
// ---------------------------------------------------------------------------
// candidates of one pass: `count` are examined, in a grid of `window` (count rounded up to whole blocks)
struct samp_pass {
  uint32_t window, count;
};
inline uint32_t samp_round_up(uint64_t v) {
  return (uint32_t)((v + BGV_SAMPLE_BLOCK - 1u) / BGV_SAMPLE_BLOCK * BGV_SAMPLE_BLOCK);
}
// no candidate at or past this number is examined: the cap, and for proposers (who never wrap
// past the list: seed.ts:76-78) the list's length
inline uint32_t samp_limit(uint64_t n_active, bool proposers) {
  return proposers && n_active < BGV_SAMPLE_CAP ? (uint32_t)n_active : BGV_SAMPLE_CAP;
}
inline uint32_t samp_first_window(uint32_t want) {
  return samp_round_up(2ull * want > BGV_SAMPLE_BLOCK ? 2ull * want : BGV_SAMPLE_BLOCK);
}
// The pass after one of prev_window candidates (0: the first) for n_todo seeds whose next candidate
// is base (< limit): twice the window, within BGV_SAMPLE_PASS_ITEMS over the seeds and within the limit.
inline samp_pass samp_plan_pass(uint32_t prev_window, uint32_t want, uint32_t base, uint32_t limit, uint32_t n_todo) {
  uint64_t w = prev_window ? 2ull * prev_window : samp_first_window(want);
  uint64_t most = BGV_SAMPLE_PASS_ITEMS / (n_todo ? n_todo : 1u) / BGV_SAMPLE_BLOCK * BGV_SAMPLE_BLOCK;
  if (most < BGV_SAMPLE_BLOCK) most = BGV_SAMPLE_BLOCK;
  if (w > most) w = most;
  if (w > limit - base) w = limit - base;
  return samp_pass{samp_round_up(w), (uint32_t)w};
}

// The pass loop.  dev.pass(todo, p, st) evaluates and picks p.count candidates for the seeds in
// todo (their next candidate is the same: they have been in every pass so far) and refreshes st,
// the states of all seeds.  Returns the first nonzero code of a pass, else 0; st[s].have < want
// afterwards says that seed s found fewer than want within limit candidates.
template <class Dev>
int samp_run(Dev& dev, uint32_t n_seeds, uint32_t want, uint32_t limit, std::vector<samp_state>& st) {
  st.assign(n_seeds, samp_state{0, 0});
  std::vector<uint32_t> todo(n_seeds);
  for (uint32_t s = 0; s < n_seeds; ++s) todo[s] = s;
  uint32_t base = 0, prev = 0;
  while (!todo.empty() && base < limit) {
    const samp_pass p = samp_plan_pass(prev, want, base, limit, (uint32_t)todo.size());
    if (int rc = dev.pass(todo, p, st)) return rc;
    base += p.count;
    prev = p.window;
    std::vector<uint32_t> rest;
    for (uint32_t s : todo)
      if (st[s].have < want) rest.push_back(s);
    todo.swap(rest);
  }
  return 0;
}
