// TEST-ONLY host build of what the bulk k_prep's task_sig and task_hash run for one set
// (lodestar_amd/csrc/bgv_k_tasks.h): the complete mixed addition jac_madd, [|x|]P and r * P of an
// affine signature (jac_mul_x_abs_aff, jac_mul_glv_aff), and hash_to_g2_sum, the hash with one
// isogeny.  Three builds of this one source:
//   shared library               entries for tests/test_prep_arith.py (compared with the oracle)
//   -DPREPSIM_MAIN               a stand-alone program (built with ASan + UBSan by the test) that
//                                checks each new form against the one it replaces
//   shared, -DBGV_COUNT_OPS      counting bodies of task_sig / task_hash (tools/count_ops.py)
// Nothing in the product links it.
#include <stdio.h>
#include <string.h>

#include "../../lodestar_amd/csrc/bls_hash.h"

static fp_t in_fp(const uint8_t* be) { return fp_to_mont(fp_from_be48(be)); }
static void out_fp(uint8_t* be, const fp_t& a) { fp_to_be48(be, fp_from_mont(a)); }
static fp2_t in_fp2(const uint8_t* be) { return fp2_t{in_fp(be), in_fp(be + 48)}; }  // (c0, c1)
static void out_fp2(uint8_t* be, const fp2_t& a) {
  out_fp(be, a.c0);
  out_fp(be + 48, a.c1);
}
// affine points as in tests/hostsim.py: coordinates of 48 raw big-endian bytes each
static g2_aff in_g2(const uint8_t* be) { return g2_aff{in_fp2(be), in_fp2(be + 96)}; }
static int g2_out(uint8_t* out, const g2_jac& j) {
  g2_aff a;
  if (!jac_to_aff(&a, j)) return 0;
  out_fp2(out, a.x);
  out_fp2(out + 96, a.y);
  return 1;
}
// the point in Jacobian form with Z != 1: (l^2 x, l^3 y, l)
static g2_jac g2_scaled(const g2_aff& a) {
  const fp2_t l = {fp_to_mont(fp_t{{3}}), fp_to_mont(fp_t{{5}})};
  const fp2_t l2 = fp2_sqr(l);
  return g2_jac{fp2_mul(a.x, l2), fp2_mul(a.y, fp2_mul(l2, l)), l};
}

enum { FORM_JAC = 0, FORM_AFF = 1, FORM_INF = 2 };
static g2_jac g2_form(const g2_aff& a, int form) {
  return form == FORM_INF ? jac_infinity<fp2_t>() : (form == FORM_AFF ? jac_from_aff(a) : g2_scaled(a));
}
// iso(q0) + iso(q1) and iso(q0 + q1) of the SSWU points of u0, u1, cofactor cleared
static g2_jac map_two(const fp2_t& u0, const fp2_t& u1) {
  const fp_t sm5 = fp_sqrt_minus5();
  return g2_clear_cofactor(jac_add(iso_map_g2_jac(sswu_g2_jac(u0, sm5)), iso_map_g2_jac(sswu_g2_jac(u1, sm5))));
}
static g2_jac map_sum(const fp2_t& u0, const fp2_t& u1) {
  const fp_t sm5 = fp_sqrt_minus5();
  return g2_clear_cofactor(iso_map_g2_jac(e2p_add(sswu_g2_jac(u0, sm5), sswu_g2_jac(u1, sm5))));
}

extern "C" {
// acc (in the given form) + q by jac_madd, as an affine point; bit 0: finite, bit 1: jac_add of the
// same operands gives the same point
int ps_g2_madd(uint8_t* out, const uint8_t* acc_aff, int form, const uint8_t* q_aff) {
  const g2_jac acc = g2_form(in_g2(acc_aff), form);
  const g2_aff q = in_g2(q_aff);
  const g2_jac m = jac_madd(acc, q);
  return g2_out(out, m) | (jac_eq(m, jac_add(acc, jac_from_aff(q))) ? 2 : 0);
}
int ps_g2_in_subgroup_aff(const uint8_t* aff) { return g2_in_subgroup_aff(in_g2(aff)); }
int ps_g2_mul_glv_aff(uint8_t* out, const uint8_t* aff, uint64_t k) { return g2_out(out, jac_mul_glv_aff(in_g2(aff), k)); }
int ps_hash_to_g2_sum(uint8_t* out, const uint8_t* msg, uint32_t len) { return g2_out(out, hash_to_g2_sum(msg, len)); }
int ps_hash_to_g2(uint8_t* out, const uint8_t* msg, uint32_t len) { return g2_out(out, hash_to_g2(msg, len)); }
// the two forms from field elements u0, u1 (96 bytes each: c0, c1); 0 for infinity
int ps_map_sum(uint8_t* out, const uint8_t* u0, const uint8_t* u1) { return g2_out(out, map_sum(in_fp2(u0), in_fp2(u1))); }
int ps_map_two(uint8_t* out, const uint8_t* u0, const uint8_t* u1) { return g2_out(out, map_two(in_fp2(u0), in_fp2(u1))); }

#ifdef BGV_COUNT_OPS
unsigned long long bgv_count_mul = 0, bgv_count_sqr = 0;
void ps_count_reset() { bgv_count_mul = bgv_count_sqr = 0; }
unsigned long long ps_count_mul() { return bgv_count_mul; }
unsigned long long ps_count_sqr() { return bgv_count_sqr; }
// what bgv_k_tasks.h task_sig / task_hash compute per set, for counting only
int ps_k_sig_body(const uint8_t* sig96, uint64_t r) {
  g2_aff a;
  bool inf;
  if (g2_decompress(&a, &inf, sig96) || inf) return 0;
  if (!g2_in_subgroup_aff(a)) return 0;
  return !jac_is_inf(jac_mul_glv_aff(a, r));
}
int ps_k_hash_body(const uint8_t* msg32) { return !jac_is_inf(hash_to_g2_sum(msg32, 32)); }
#endif
}  // extern "C"

#ifdef PREPSIM_MAIN
static const uint32_t kWords[] = {0, 1, 7, 8, 9, 0x88888888u, 0x99999999u, 0x77777777u, 0x80000000u, 0xffffffffu};
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static int check_madd(const g2_jac& acc, const g2_aff& q, bool want_inf, const char* what) {
  const g2_jac m = jac_madd(acc, q);
  const int bad = !jac_eq(m, jac_add(acc, jac_from_aff(q))) || jac_is_inf(m) != want_inf;
  if (bad) fprintf(stderr, "prepsim: jac_madd wrong, %s\n", what);
  return bad;
}
int main() {
  int bad = 0;
  g2_aff p, q;
  const uint8_t m0[8] = {'p', 'r', 'e', 'p', 's', 'i', 'm', '0'}, m1[8] = {'p', 'r', 'e', 'p', 's', 'i', 'm', '1'};
  if (!jac_to_aff(&p, hash_to_g2(m0, 8)) || !jac_to_aff(&q, hash_to_g2(m1, 8))) return 2;
  // the mixed addition: generic, acc == Q, acc == -Q, acc at infinity; Z == 1 and Z != 1
  bad += check_madd(g2_scaled(p), q, false, "generic");
  bad += check_madd(jac_from_aff(p), q, false, "generic, Z == 1");
  bad += check_madd(g2_scaled(q), q, false, "acc == Q");
  bad += check_madd(jac_from_aff(q), q, false, "acc == Q, Z == 1");
  bad += check_madd(jac_neg(g2_scaled(q)), q, true, "acc == -Q");
  bad += check_madd(jac_neg(jac_from_aff(q)), q, true, "acc == -Q, Z == 1");
  {
    const g2_jac m = jac_madd(jac_infinity<fp2_t>(), q);
    if (!jac_eq(m, jac_from_aff(q))) {
      fprintf(stderr, "prepsim: jac_madd wrong, acc at infinity\n");
      ++bad;
    }
  }
  // [|x|]P and the subgroup check of an affine point
  bad += !jac_eq(jac_mul_x_abs_aff(p), jac_mul_x_abs(jac_from_aff(p)));
  bad += !g2_in_subgroup_aff(p) || !g2_in_subgroup_aff(q);
  // r * P: the edge words in either half and in both, and seeded scalars
  int n = 0;
  for (uint32_t lo : kWords)
    for (uint32_t hi : kWords) {
      if (lo != 0 && hi != 0 && lo != hi) continue;
      const uint64_t k = ((uint64_t)hi << 32) | lo;
      const int b = !jac_eq(jac_mul_glv_aff(p, k), jac_mul_glv(jac_from_aff(p), k));
      if (b) fprintf(stderr, "prepsim: jac_mul_glv_aff mismatch at k = %016llx\n", (unsigned long long)k);
      bad += b;
      ++n;
    }
  for (int i = 0; i < 8; ++i, ++n) {
    const uint64_t k = rng();
    bad += !jac_eq(jac_mul_glv_aff(q, k), jac_mul_glv(jac_from_aff(q), k));
  }
  // the hash with one isogeny: messages, equal field elements, opposite ones, u == 0
  for (int i = 0; i < 6; ++i) {
    uint8_t msg[32];
    for (int j = 0; j < 32; ++j) msg[j] = (uint8_t)(rng() >> 17);
    const int b = !jac_eq(hash_to_g2_sum(msg, 32), hash_to_g2(msg, 32));
    if (b) fprintf(stderr, "prepsim: hash_to_g2_sum mismatch, message %d\n", i);
    bad += b;
  }
  fp2_t u0, u1;
  hash_to_field_fp2(&u0, &u1, m0, 8);
  bad += !jac_eq(map_sum(u0, u0), map_two(u0, u0)) || jac_is_inf(map_sum(u0, u0));
  bad += !jac_is_inf(map_sum(u0, fp2_neg(u0))) || !jac_is_inf(map_two(u0, fp2_neg(u0)));
  bad += !jac_eq(map_sum(fp2_zero(), u1), map_two(fp2_zero(), u1));
  bad += !jac_eq(map_sum(fp2_zero(), fp2_zero()), map_two(fp2_zero(), fp2_zero()));
  printf("prepsim: %d scalars, %d failures\n", n, bad);
  return bad ? 1 : 0;
}
#endif
