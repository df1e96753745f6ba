// TEST-ONLY host build of the bulk k_prep's point arithmetic (lodestar_amd/csrc/bls_curve.h,
// bls_hash.h): the signed radix-16 recoding, jac_mul_glv for P with Z != 1, Z == 1 and P at
// infinity, the subgroup check and hash_to_g2.  Three builds of this one source:
//   shared library               entries for tests/test_curve_recode.py (compared with the oracle)
//   -DCURVESIM_MAIN              a stand-alone program (built with ASan + UBSan by the test) that
//                                checks the recoding and the multiplications against jac_mul_u64
//   shared, -DBGV_COUNT_OPS      counting bodies of task_sig / task_hash / task_pk (tools/count_ops.py)
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
static g1_aff in_g1(const uint8_t* be) { return g1_aff{in_fp(be), in_fp(be + 48)}; }
static int g2_out(uint8_t* out, const g2_jac& j) {
  g2_aff a;
  if (!jac_to_aff(&a, j)) return 0;
  out_fp2(out, a.x);
  out_fp2(out + 96, a.y);
  return 1;
}
static int g1_out(uint8_t* out, const g1_jac& j) {
  g1_aff a;
  if (!jac_to_aff(&a, j)) return 0;
  out_fp(out, a.x);
  out_fp(out + 48, a.y);
  return 1;
}
// the point handed over in Jacobian form with Z != 1: (l^2 x, l^3 y, l)
static g2_jac g2_scaled(const g2_aff& a) {
  const fp2_t l = {fp_to_mont(fp_t{{3}}), fp_to_mont(fp_t{{5}})};
  const fp2_t l2 = fp2_sqr(l);
  return g2_jac{fp2_mul(a.x, l2), fp2_mul(a.y, fp2_mul(l2, l)), l};
}
static g1_jac g1_scaled(const g1_aff& a) {
  const fp_t l = fp_to_mont(fp_t{{7}});
  const fp_t l2 = fp_sqr(l);
  return g1_jac{fp_mul(a.x, l2), fp_mul(a.y, fp_mul(l2, l)), l};
}

enum { FORM_JAC = 0, FORM_AFF = 1, FORM_INF = 2 };
static g1_jac mul_glv(const g1_aff& a, uint64_t k, int form) {
  if (form == FORM_AFF) return jac_mul_glv(jac_from_aff(a), k);
  return jac_mul_glv(form == FORM_INF ? jac_infinity<fp_t>() : g1_scaled(a), k);
}
static g2_jac mul_glv(const g2_aff& a, uint64_t k, int form) {
  if (form == FORM_AFF) return jac_mul_glv(jac_from_aff(a), k);
  return jac_mul_glv(form == FORM_INF ? jac_infinity<fp2_t>() : g2_scaled(a), k);
}

extern "C" {
// digits[0..7] = d_j, digits[8] = the final carry
void cs_recode16(uint32_t a, int32_t* digits) {
  const uint64_t c = bgv_recode16_carries(a);
  for (int j = 0; j < 8; ++j) digits[j] = bgv_recode16_digit(a, c, j);
  digits[8] = (int32_t)((c >> 32) & 1u);
}
// [lo32(k) + hi32(k) x^2] P as an affine point; 0 for infinity
int cs_g1_mul_glv(uint8_t* out, const uint8_t* aff, uint64_t k, int form) { return g1_out(out, mul_glv(in_g1(aff), k, form)); }
int cs_g2_mul_glv(uint8_t* out, const uint8_t* aff, uint64_t k, int form) { return g2_out(out, mul_glv(in_g2(aff), k, form)); }
int cs_g2_in_subgroup(const uint8_t* aff) { return g2_in_subgroup(jac_from_aff(in_g2(aff))); }
// 96-byte compressed signature -> affine (0), or the BGV_* code, or 100 for infinity
int cs_g2_decompress(uint8_t* out, const uint8_t* in96) {
  g2_aff a;
  bool inf;
  const int rc = g2_decompress(&a, &inf, in96);
  if (rc) return rc;
  if (inf) return 100;
  out_fp2(out, a.x);
  out_fp2(out + 96, a.y);
  return 0;
}
int cs_hash_to_g2(uint8_t* out, const uint8_t* msg, uint32_t len) { return g2_out(out, hash_to_g2(msg, len)); }

#ifdef BGV_COUNT_OPS
unsigned long long bgv_count_mul = 0, bgv_count_sqr = 0;
void cs_count_reset() { bgv_count_mul = bgv_count_sqr = 0; }
unsigned long long cs_count_mul() { return bgv_count_mul; }
unsigned long long cs_count_sqr() { return bgv_count_sqr; }
// what bgv_k_tasks.h task_sig / task_hash / task_pk compute per set, for counting only
int cs_k_sig_body(const uint8_t* sig96, uint64_t r) {
  g2_aff a;
  bool inf;
  if (g2_decompress(&a, &inf, sig96) || inf) return 0;
  if (!g2_in_subgroup(jac_from_aff(a))) return 0;
  return !jac_is_inf(jac_mul_glv(jac_from_aff(a), r));
}
int cs_k_hash_body(const uint8_t* msg32) { return !jac_is_inf(hash_to_g2(msg32, 32)); }
int cs_k_pk_body(const uint8_t* pk_aff, uint32_t n_pk, uint64_t r) {
  const g1_aff p = in_g1(pk_aff);
  g1_jac acc = jac_infinity<fp_t>();
  for (uint32_t k = 0; k < n_pk; ++k) acc = jac_add_aff(acc, p);
  return !jac_is_inf(jac_mul_glv(acc, r));
}
#endif
}  // extern "C"

#ifdef CURVESIM_MAIN
static const uint32_t kWords[] = {0, 1, 7, 8, 9, 0x88888888u, 0x99999999u, 0x77777777u, 0x80000000u, 0xffffffffu};
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static int check_recode(uint32_t a) {
  int32_t d[9];
  cs_recode16(a, d);
  int64_t sum = 0;
  for (int j = 8; j >= 0; --j) {
    if (j < 8 && (d[j] < -8 || d[j] > 8)) return 1;
    sum = sum * 16 + d[j];
  }
  return (d[8] != 0 && d[8] != 1) || sum != (int64_t)a;
}
// a P + b E(P) with the plain unsigned windows of jac_mul_u64
template <class F>
static jac_t<F> mul_ref(const jac_t<F>& p, uint64_t k) {
  return jac_add(jac_mul_u64(p, k & 0xffffffffull), jac_endo_x2(jac_mul_u64(p, k >> 32)));
}
template <class A>
static int check_mul(const A& a, uint64_t k) {
  const auto ref = mul_ref(jac_from_aff(a), k);
  int bad = 0;
  bad += !jac_eq(mul_glv(a, k, FORM_JAC), ref);
  bad += !jac_eq(mul_glv(a, k, FORM_AFF), ref);
  bad += !jac_is_inf(mul_glv(a, k, FORM_INF));
  if (bad) fprintf(stderr, "curvesim: jac_mul_glv mismatch at k = %016llx\n", (unsigned long long)k);
  return bad;
}
int main() {
  int bad = 0;
  for (uint32_t a : kWords) bad += check_recode(a);
  for (int i = 0; i < 100000; ++i) bad += check_recode((uint32_t)rng());
  if (bad) fprintf(stderr, "curvesim: %d recodings wrong\n", bad);
  const g1_aff g1 = g1_generator();
  g2_aff g2;
  const uint8_t msg[8] = {'c', 'u', 'r', 'v', 'e', 's', 'i', 'm'};
  if (!jac_to_aff(&g2, hash_to_g2(msg, 8))) return 2;
  if (!g2_in_subgroup(jac_from_aff(g2))) return 3;
  int n = 0;
  for (uint32_t lo : kWords)
    for (uint32_t hi : kWords) {
      if (lo != 0 && hi != 0 && lo != hi) continue;  // each word in either half, and in both
      const uint64_t k = ((uint64_t)hi << 32) | lo;
      bad += check_mul(g1, k) + check_mul(g2, k);
      ++n;
    }
  for (int i = 0; i < 8; ++i, ++n) {
    const uint64_t k = rng();
    bad += check_mul(g1, k) + check_mul(g2, k);
  }
  printf("curvesim: %d scalars, %d failures\n", n, bad);
  return bad ? 1 : 0;
}
#endif
