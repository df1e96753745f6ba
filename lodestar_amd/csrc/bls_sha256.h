// SHA-256 for the device and the host: one compression function and a driver for messages
// given byte by byte (hash_to_G2's expand_message_xmd, bls_hash.h; the swap-or-not digests of
// the epoch shuffling, bgv_shuffle.h).  Stands alone (no field arithmetic), so host programs that
// need the hash only compile it in a moment.
#pragma once
#include <stdint.h>

// as bls_field.h defines them (token for token, whichever header comes first)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef BGV_HD
#if defined(__HIPCC__)
#define BGV_HD __host__ __device__ __forceinline__
#else
#define BGV_HD inline __attribute__((always_inline))
#endif
#endif
#ifndef BGV_NOINLINE
#if defined(__HIPCC__)
#define BGV_NOINLINE static __host__ __device__ __noinline__
#else
#define BGV_NOINLINE __attribute__((noinline))
#endif
#endif
#ifndef BGV_UNROLL
#define BGV_UNROLL _Pragma("unroll")
#define BGV_NO_UNROLL _Pragma("unroll 1")
#endif

// ---------------------------------------------------------------------------
// SHA-256
// ---------------------------------------------------------------------------
BGV_HD uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

BGV_NOINLINE void sha256_compress(uint32_t st[8], const uint32_t blk[16]) {
  const uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t w[16];
  BGV_UNROLL for (int i = 0; i < 16; ++i) w[i] = blk[i];
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  BGV_UNROLL for (int i = 0; i < 64; ++i) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      uint32_t s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3);
      uint32_t s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
      wi = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
      w[i & 15] = wi;
    }
    uint32_t S1 = sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25);
    uint32_t ch = (e & f) ^ (~e & g);
    uint32_t t1 = h + S1 + ch + K[i] + wi;
    uint32_t S0 = sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22);
    uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    uint32_t t2 = S0 + mj;
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
  st[4] += e;
  st[5] += f;
  st[6] += g;
  st[7] += h;
}

BGV_HD void sha256_init(uint32_t st[8]) {
  st[0] = 0x6a09e667u;
  st[1] = 0xbb67ae85u;
  st[2] = 0x3c6ef372u;
  st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu;
  st[5] = 0x9b05688cu;
  st[6] = 0x1f83d9abu;
  st[7] = 0x5be0cd19u;
}

// Hash a "virtual" message of total_len bytes whose byte at position i is
// get(i) (lane-uniform length, so every lane runs the same number of blocks).
template <class G>
BGV_HD void sha256_virtual(uint32_t out[8], const G& get, uint32_t total_len) {
  uint32_t st[8];
  sha256_init(st);
  const uint32_t padded = ((total_len + 9 + 63) / 64) * 64;
  const uint64_t bitlen = (uint64_t)total_len * 8;
  BGV_NO_UNROLL for (uint32_t base = 0; base < padded; base += 64) {
    uint32_t blk[16];
    BGV_UNROLL for (int wi = 0; wi < 16; ++wi) {
      uint32_t word = 0;
      BGV_UNROLL for (int k = 0; k < 4; ++k) {
        const uint32_t pos = base + (uint32_t)(wi * 4 + k);
        uint32_t byte;
        if (pos < total_len)
          byte = get(pos);
        else if (pos == total_len)
          byte = 0x80;
        else if (pos >= padded - 8)
          byte = (uint32_t)(bitlen >> (8 * (padded - 1 - pos))) & 0xff;
        else
          byte = 0;
        word = (word << 8) | byte;
      }
      blk[wi] = word;
    }
    sha256_compress(st, blk);
  }
  BGV_UNROLL for (int i = 0; i < 8; ++i) out[i] = st[i];
}
