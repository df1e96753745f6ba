// TEST-ONLY: the fed team Miller loop (k_lines_team -> k_miller_team_fed) emulated on the host,
// over the product's own headers: the writer walks a pair's twist point with miller_lines_walk
// and stores each step's line scaled by the pair's P (lz_pline_scaled) at
// miller_fed_rec_word(pair, k) of a buffer of cap pairs, exactly as a k_lines_team lane does
// (the kernel walks signature pairs, P = -G1; the general scaling of a Jacobian P is checked
// here too, it is what a pubkey-sum pair would take);
// the reader is a team as k_miller_team_fed runs it: its sixteen lanes bring the record into
// the team's staging words (quad c, and quad 16 + c on lanes 0..4), the accumulator goes
// through bls_team.h's tm_emu team operations (first step f = line, then per step a squaring
// and a line product, an addition step only the line product), conjugated at the end.
//
//   fedsim            runs every check; prints "ok <name>" per check, exits 1 on a failure
//
// Checks (exact equality of field elements):
//   sig      P = -G1, Q Jacobian with Z != 1: final_exp(fed) == final_exp(miller_loop1)
//   pk       P Jacobian with Z != 1 (a pubkey sum):  the same
//   dead     a pair that takes no part gives 1
//   offsets  writer and reader agree for pair 0, pair cap - 1 and a cap that is no multiple of
//            64, every record inside the buffer and no two records overlapping
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../lodestar_amd/csrc/bls_hash.h"
#include "../../lodestar_amd/csrc/bls_pairing.h"
#include "../../lodestar_amd/csrc/bls_team.h"
#include "../../lodestar_amd/csrc/bgv_tmiller.h"

static const uint32_t FILL = 0xDEADBEEFu;  // unwritten words

static bool fp12_same(const fp12_t& a, const fp12_t& b) {
  const fp2_t* x[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  const fp2_t* y[6] = {&b.c0.c0, &b.c0.c1, &b.c0.c2, &b.c1.c0, &b.c1.c1, &b.c1.c2};
  for (int i = 0; i < 6; ++i)
    if (!fp2_eq(*x[i], *y[i])) return false;
  return true;
}

// the writer: one k_lines_team lane.  Returns the number of records written.
static int write_pair(std::vector<uint32_t>& lines, uint32_t cap, uint32_t pair, const g1_jac& p, const g2_jac& q,
                      bool unit_z) {
  if (pair >= cap || jac_is_inf(p) || jac_is_inf(q)) return 0;
  const miller_p P0 = miller_p_make(p);
  const lz_mp P = {lz_in(P0.xn), lz_in(P0.yp), lz_in(P0.zp3)};
  int n = 0;
  miller_lines_walk(&q, [&](int k, const auto& rec) {
    const lz_sline s = lz_pline_scaled(rec, P, unit_z);
    static_assert(sizeof(s) == 4 * BGV_LINE_WORDS, "scaled record layout");
    const size_t w = miller_fed_rec_word(pair, k);
    if (w + BGV_LINE_WORDS > lines.size()) {
      fprintf(stderr, "writer: record %d of pair %u past the buffer\n", k, pair);
      exit(1);
    }
    memcpy(lines.data() + w, &s, sizeof(s));
    ++n;
  });
  return n;
}

// the reader: one team of k_miller_team_fed, lane by lane
static fp12_t read_pair(const std::vector<uint32_t>& lines, uint32_t pair, bool live) {
  uint32_t R[BGV_LINE_WORDS];
  int k = 0;
  auto stage = [&](fp2_t* l0, fp2_t* l1, fp2_t* l3) {
    for (int c = 0; c < BGV_TEAM; ++c) {  // lane c: quad c, lanes 0..4 also quad 16 + c
      for (int part = 0; part < 2; ++part) {
        const int quad = part * BGV_TEAM + c;
        if (quad >= BGV_LINE_QUADS) continue;
        for (int j = 0; j < 4; ++j) {
          const size_t w = miller_fed_rec_word(pair, k) + 4 * quad + j;
          if (live && w >= lines.size()) {
            fprintf(stderr, "reader: record %d of pair %u past the buffer\n", k, pair);
            exit(1);
          }
          R[4 * quad + j] = live ? lines[w] : 0u;
        }
      }
    }
    ++k;
    lz_sline_fp2(R, l0, l1, l3);
  };
  tm_emu_ops o;
  fp2_t l0, l1, l3;
  stage(&l0, &l1, &l3);
  tm_emu_t f = o.line(l0, l1, l3);
  for (int i = 61; i >= 0; --i) {
    if (tmp_add_at(i)) {
      stage(&l0, &l1, &l3);
      f = o.mul_line(f, l0, l1, l3);
    }
    f = o.sqr(f);
    stage(&l0, &l1, &l3);
    f = o.mul_line(f, l0, l1, l3);
  }
  if (k != BGV_MILLER_STEPS) {
    fprintf(stderr, "reader: %d records, not %d\n", k, BGV_MILLER_STEPS);
    exit(1);
  }
  return live ? tm_emu_to_fp12(o.conj(f)) : fp12_one();
}

static int fails = 0;
static void check(const char* name, bool ok) {
  printf("%s %s\n", ok ? "ok" : "FAIL", name);
  if (!ok) ++fails;
}

int main() {
  const uint8_t m0[32] = {1, 2, 3}, m1[32] = {9, 8, 7, 6};
  const g2_jac Q0 = hash_to_g2(m0, 32), Q1 = hash_to_g2(m1, 32);
  const g1_jac negG1 = jac_from_aff(g1_neg_generator());
  const g1_jac Pk = jac_mul_u64(jac_from_aff(g1_generator()), 0x1234567890ABCDEFull);
  check("inputs: Q has Z != 1", !fp2_eq(Q0.z, fp2_t{fp_one(), fp_zero()}) && !jac_is_inf(Q0));
  check("inputs: the pubkey sum has Z != 1", !fp_eq(Pk.z, fp_one()) && !jac_is_inf(Pk));

  const uint32_t cap = 100;  // no multiple of 64
  const size_t words = (size_t)cap * BGV_MILLER_STEPS * BGV_LINE_WORDS;  // bgv_line_record_bytes() * cap / 4
  std::vector<uint32_t> lines(words, FILL);

  // (a) a signature pair at pair 0, (b) a pubkey-sum pair at pair cap - 1
  check("sig: 68 records", write_pair(lines, cap, 0, negG1, Q0, true) == BGV_MILLER_STEPS);
  check("pk: 68 records", write_pair(lines, cap, cap - 1, Pk, Q1, false) == BGV_MILLER_STEPS);
  check("sig: final_exp(fed) == final_exp(miller_loop1)",
        fp12_same(final_exp(read_pair(lines, 0, true)), final_exp(miller_loop1(negG1, Q0))));
  check("pk: final_exp(fed) == final_exp(miller_loop1)",
        fp12_same(final_exp(read_pair(lines, cap - 1, true)), final_exp(miller_loop1(Pk, Q1))));
  // the signature pair with the general scaling (Z_P^3 = 1 as a product) is the same record
  {
    std::vector<uint32_t> other(words, FILL);
    write_pair(other, cap, 0, negG1, Q0, false);
    bool same = true;
    for (int k = 0; k < BGV_MILLER_STEPS && same; ++k) {
      fp2_t a0, a1, a3, b0, b1, b3;
      lz_sline_fp2(lines.data() + miller_fed_rec_word(0, k), &a0, &a1, &a3);
      lz_sline_fp2(other.data() + miller_fed_rec_word(0, k), &b0, &b1, &b3);
      same = fp2_eq(a0, b0) && fp2_eq(a1, b1) && fp2_eq(a3, b3);
    }
    check("sig: l0 without the product equals l0 * 1", same);
  }

  // (c) pairs that take no part: an infinite Q / an infinite P write nothing, the team gives 1
  {
    std::vector<uint32_t> snap = lines;
    check("dead: an infinite Q writes nothing", write_pair(lines, cap, 5, negG1, jac_infinity<fp2_t>(), true) == 0);
    check("dead: an infinite P writes nothing", write_pair(lines, cap, 6, jac_infinity<fp_t>(), Q0, false) == 0);
    check("dead: a pair past the capacity writes nothing", write_pair(lines, cap, cap, negG1, Q0, true) == 0);
    check("dead: the buffer is untouched", snap == lines);
    check("dead: the team's value is 1", fp12_is_one(read_pair(lines, 5, false)));
  }

  // (d) offsets: only the two pairs' words were written, each record whole and inside the buffer
  {
    bool ok = true;
    for (uint32_t p = 0; p < cap && ok; ++p)
      for (int k = 0; k < BGV_MILLER_STEPS && ok; ++k) {
        const size_t w = miller_fed_rec_word(p, k);
        ok = w % 4 == 0 && w + BGV_LINE_WORDS <= words &&
             (k + 1 == BGV_MILLER_STEPS || miller_fed_rec_word(p, k + 1) == w + BGV_LINE_WORDS) &&
             (p + 1 == cap || miller_fed_rec_word(p + 1, 0) == miller_fed_rec_word(p, 0) + words / cap);
      }
    check("offsets: records are whole, 16-byte aligned, contiguous per pair, inside the buffer", ok);
    check("offsets: the last record of pair cap - 1 ends the buffer",
          miller_fed_rec_word(cap - 1, BGV_MILLER_STEPS - 1) + BGV_LINE_WORDS == words);
    size_t written = 0;
    bool inside = true;
    for (size_t w = 0; w < words; ++w) {
      // a limb is at most 28 bits wide, so a written word never equals the fill
      if (lines[w] == FILL) continue;
      ++written;
      const size_t pair = w / (words / cap);
      inside = inside && (pair == 0 || pair == cap - 1);
    }
    check("offsets: exactly two pairs' words were written",
          inside && written == 2 * (size_t)BGV_MILLER_STEPS * BGV_LINE_WORDS);
    // 2^32-safe: the word index of a far pair does not wrap
    check("offsets: pair 1,000,000 is past 2^32 words and does not wrap",
          miller_fed_rec_word(1000000u, 0) == (size_t)1000000 * BGV_MILLER_STEPS * BGV_LINE_WORDS &&
              miller_fed_rec_word(1000000u, 0) > 0xFFFFFFFFull);
  }
  return fails ? 1 : 0;
}
