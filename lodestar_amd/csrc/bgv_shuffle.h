// Epoch shuffling (bgv_shuffling_put): the swap-or-not arithmetic of compute_shuffled_index /
// unshuffleList (state-transition/src/util/shuffle.ts) and the committee bounds of
// computeEpochShuffling (util/epochShuffling.ts).  Plain host/device functions (no HIP types):
// k_shuffle_table / k_shuffle_walk / k_shuffle_dir (bgv_k_shuffle.hip) run them per thread, the
// host (bgv_registry.cpp) cuts its mirror with the bounds and tests/native/shufflesim.cpp runs all of
// it on a CPU.
//
// Round r (one byte) of a list of n positions has a pivot LE64(sha256(seed | r)[0:8]) mod n and
// one 256-bit digest sha256(seed | r | LE32(b)) per block b of 256 positions.  Position i meets
// flip = (pivot + n - i) mod n; the larger of the two, pos, names the deciding bit
// (digest_b[(pos & 255) >> 3] >> (pos & 7)) & 1 with b = pos >> 8, and i moves to flip when it is
// set.  Both messages (33 and 37 bytes) fit one SHA-256 block.  The digests of all rounds form the
// TABLE: rounds x ceil(n / 256) x 8 words, each digest stored as little-endian 32-bit words, so
// the bit of pos is (table[(r * nblk + (pos >> 8)) * 8 + ((pos >> 5) & 7)] >> (pos & 31)) & 1 --
// one 32-bit load, a shift and a mask.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bls_sha256.h"  // bls_hash.h's SHA-256: sha256_init / sha256_compress, BGV_HD

#define BGV_SHUFFLE_MAX_N (1u << 22)
#define BGV_SHUFFLE_MAX_ROUNDS 255u

// ---------------------------------------------------------------------------
// committees of a shuffling of n indices cut into count = slots * committees_per_slot pieces
// ---------------------------------------------------------------------------
// committee k is shuffling[shuf_bound(n, k, count), shuf_bound(n, k + 1, count))
BGV_HD uint32_t shuf_bound(uint32_t n, uint32_t k, uint32_t count) { return (uint32_t)((uint64_t)n * k / count); }
// how many of the count committees hold a member, and the longest one
BGV_HD uint32_t shuf_nonempty(uint32_t n, uint32_t count) { return n < count ? n : count; }
BGV_HD uint32_t shuf_longest(uint32_t n, uint32_t count) { return (uint32_t)(((uint64_t)n + count - 1) / count); }
// The j-th non-empty committee (j < shuf_nonempty): its number k and its range [*lo, *hi).
// With n >= count every committee holds a member; with n < count a committee holds one or none,
// and the j-th member is alone in the first committee whose upper bound reaches j + 1.
BGV_HD uint32_t shuf_nonempty_k(uint32_t n, uint32_t count, uint32_t j, uint32_t* lo, uint32_t* hi) {
  if (n >= count) {
    *lo = shuf_bound(n, j, count);
    *hi = shuf_bound(n, j + 1, count);
    return j;
  }
  *lo = j;
  *hi = j + 1;
  return (uint32_t)((((uint64_t)j + 1) * count + n - 1) / n) - 1u;
}

// ---------------------------------------------------------------------------
// the table's geometry
// ---------------------------------------------------------------------------
BGV_HD uint32_t shuf_nblk(uint32_t n) { return (n + 255u) >> 8; }
// words of the table proper; the rounds pivots follow it
BGV_HD uint64_t shuf_table_words(uint32_t n, uint32_t rounds) { return (uint64_t)rounds * shuf_nblk(n) * 8u; }

// One round's move of position i (< n) given the round's pivot (< n) and its digests
// (tab_r = table + r * nblk * 8): one dependent 32-bit load.
BGV_HD uint32_t shuf_step(uint32_t i, uint32_t n, uint32_t pivot, const uint32_t* tab_r) {
  const uint32_t x = pivot + n - i;  // 1 .. 2n - 1
  const uint32_t flip = x >= n ? x - n : x;
  const uint32_t pos = i > flip ? i : flip;
  const uint32_t w = tab_r[(pos >> 8) * 8u + ((pos >> 5) & 7u)];
  return ((w >> (pos & 31u)) & 1u) ? flip : i;
}

// compute_shuffled_index(i, n, seed) over the table's rounds, r = 0 .. rounds - 1
BGV_HD uint32_t shuf_walk(uint32_t i, uint32_t n, uint32_t rounds, const uint32_t* table, const uint32_t* pivots) {
  if (n < 2) return i;
  const uint32_t stride = shuf_nblk(n) * 8u;
  for (uint32_t r = 0; r < rounds; ++r) i = shuf_step(i, n, pivots[r], table + (size_t)r * stride);
  return i;
}

// ---------------------------------------------------------------------------
// the two hash inputs
// ---------------------------------------------------------------------------
// the seed as SHA-256 reads it: 8 big-endian words
struct shuf_seed {
  uint32_t w[8];
};
BGV_HD shuf_seed shuf_seed_load(const uint8_t seed[32]) {
  shuf_seed s;
  for (int j = 0; j < 8; ++j)
    s.w[j] = (uint32_t)seed[4 * j] << 24 | (uint32_t)seed[4 * j + 1] << 16 | (uint32_t)seed[4 * j + 2] << 8 |
             (uint32_t)seed[4 * j + 3];
  return s;
}
BGV_HD uint32_t shuf_bswap(uint32_t v) {
  return v << 24 | (v & 0xff00u) << 8 | (v >> 8 & 0xff00u) | v >> 24;
}

// sha256(seed | r): the pivot's digest (33 bytes, one block)
BGV_HD void shuf_hash_pivot(uint32_t out[8], const shuf_seed& s, uint32_t r) {
  uint32_t blk[16];
  BGV_UNROLL for (int j = 0; j < 8; ++j) blk[j] = s.w[j];
  blk[8] = r << 24 | 0x80u << 16;
  BGV_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0;
  blk[15] = 33u * 8u;
  sha256_init(out);
  sha256_compress(out, blk);
}
// sha256(seed | r | LE32(b)): the digest of block b (37 bytes, one block)
BGV_HD void shuf_hash_block(uint32_t out[8], const shuf_seed& s, uint32_t r, uint32_t b) {
  uint32_t blk[16];
  BGV_UNROLL for (int j = 0; j < 8; ++j) blk[j] = s.w[j];
  blk[8] = r << 24 | (b & 0xffu) << 16 | (b & 0xff00u) | (b >> 16 & 0xffu);
  blk[9] = (b >> 24) << 24 | 0x80u << 16;
  BGV_UNROLL for (int j = 10; j < 15; ++j) blk[j] = 0;
  blk[15] = 37u * 8u;
  sha256_init(out);
  sha256_compress(out, blk);
}

// the round's pivot: the digest's first 8 bytes as a little-endian number, mod n
BGV_HD uint32_t shuf_pivot(const shuf_seed& s, uint32_t r, uint32_t n) {
  uint32_t d[8];
  shuf_hash_pivot(d, s, r);
  const uint64_t v = (uint64_t)shuf_bswap(d[1]) << 32 | shuf_bswap(d[0]);
  return (uint32_t)(v % n);
}
// block b of round r as the table keeps it: 8 little-endian words
BGV_HD void shuf_table_block(uint32_t out[8], const shuf_seed& s, uint32_t r, uint32_t b) {
  uint32_t d[8];
  shuf_hash_block(d, s, r, b);
  BGV_UNROLL for (int j = 0; j < 8; ++j) out[j] = shuf_bswap(d[j]);
}

// Element t of the table's (rounds * nblk) digests and rounds pivots, as k_shuffle_table's
// thread t computes it.
BGV_HD void shuf_table_item(uint32_t t, const shuf_seed& s, uint32_t n, uint32_t rounds, uint32_t* table,
                            uint32_t* pivots) {
  const uint32_t nblk = shuf_nblk(n), nd = rounds * nblk;
  if (t < nd) {
    uint32_t d[8];
    shuf_table_block(d, s, t / nblk, t % nblk);
    BGV_UNROLL for (int j = 0; j < 8; ++j) table[(size_t)t * 8u + j] = d[j];
  } else if (t < nd + rounds) {
    pivots[t - nd] = shuf_pivot(s, t - nd, n);
  }
}
