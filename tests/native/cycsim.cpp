// TEST-ONLY: the closing kernels' final exponentiation (bls_team.h: tm_cyc_sqr_lane, tm_easy_norm /
// tm_easy_finish, tm_final_exp_cyc, tm_batch_inv) on the host, over the product's own headers: a team
// is tm_emu_ops (every lane function run for each of the 12 lanes), the references are the one-lane
// tower functions of bls_field.h / bls_pairing.h.
//
//   cycsim            runs every check; prints "ok <name>" per check, exits 1 on a failure
//
// Built as a program under AddressSanitizer + UBSan and, at -O2, as a shared library (tests/cycsim.py):
// cs_selftest runs the same checks there, the other cs_* functions let pytest compare with
// oracle/bls12381.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../lodestar_amd/csrc/bls_hash.h"
#include "../../lodestar_amd/csrc/bls_pairing.h"
#include "../../lodestar_amd/csrc/bls_team.h"

static fp_t in_fp(const uint8_t* be) { return fp_to_mont(fp_from_be48(be)); }
static void out_fp(uint8_t* be, const fp_t& a) { fp_to_be48(be, fp_from_mont(a)); }
static const int kTower[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 0}, {1, 1}, {1, 2}};
static fp2_t* f12_at(fp12_t& f, int i) {
  fp6_t& h = kTower[i][0] ? f.c1 : f.c0;
  return kTower[i][1] == 0 ? &h.c0 : (kTower[i][1] == 1 ? &h.c1 : &h.c2);
}
static fp12_t in_fp12(const uint8_t* be) {
  fp12_t f;
  for (int i = 0; i < 6; ++i) *f12_at(f, i) = fp2_t{in_fp(be + 96 * i), in_fp(be + 96 * i + 48)};
  return f;
}
static void out_fp12(uint8_t* be, const fp12_t& f0) {
  fp12_t f = f0;
  for (int i = 0; i < 6; ++i) {
    out_fp(be + 96 * i, f12_at(f, i)->c0);
    out_fp(be + 96 * i + 48, f12_at(f, i)->c1);
  }
}

static bool fp12_same(const fp12_t& a0, const fp12_t& b0) {
  fp12_t a = a0, b = b0;
  for (int i = 0; i < 6; ++i)
    if (!fp2_eq(*f12_at(a, i), *f12_at(b, i))) return false;
  return true;
}

// The closing as a team runs it, with the inversion on one lane: U, and whether n was zero.
static tm_emu_t team_final_exp_cyc(const tm_emu_t& f, bool* zero) {
  tm_emu_ops o;
  tm_emu_t G;
  const tm_emu_t N = tm_easy_norm(o, f, &G);
  const fp_t n = o.norm2(N);
  fp_t ninv;
  *zero = tm_batch_inv<1>(&n, &ninv, [](const fp_t& x) { return fp_inv(x); }) != 0;
  return tm_final_exp_cyc(o, tm_easy_finish(o, f, G, N, ninv));
}

// what the closing kernels store: u = 1 + conj(U)
static tm_emu_t team_gu(const tm_emu_t& U) {
  tm_emu_ops o;
  tm_emu_t u = o.conj(U);
  u.c[0] = fp_add(u.c[0], fp_one());
  return u;
}

extern "C" {
// U of f (576 bytes, tower order, canonical big-endian); returns 1 when f has norm zero
int cs_final_exp_cyc(uint8_t* out, const uint8_t* f) {
  bool zero;
  out_fp12(out, tm_emu_to_fp12(team_final_exp_cyc(tm_emu_from_fp12(in_fp12(f)), &zero)));
  return zero ? 1 : 0;
}
// the power of the pairing value that U is
int cs_chain_factor() { return BGV_FINAL_EXP_CHAIN_FACTOR; }
// verdict bit 0 of the closing kernels: u = 1 + conj(U) lies in Fp6
int cs_verdict(const uint8_t* f) {
  bool zero;
  tm_emu_ops o;
  const tm_emu_t U = team_final_exp_cyc(tm_emu_from_fp12(in_fp12(f)), &zero);
  return !zero && o.is_fp6(team_gu(U));
}
}

// ---------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static fp_t rand_fp() {
  uint8_t b[48];
  for (int i = 0; i < 48; ++i) b[i] = (uint8_t)(rng() >> 32);
  b[0] &= 0x0f;  // < 2^380 < p
  return in_fp(b);
}
static fp12_t rand_fp12() {
  fp12_t f;
  for (int i = 0; i < 6; ++i) *f12_at(f, i) = fp2_t{rand_fp(), rand_fp()};
  return f;
}
// f^((p^6 - 1)(p^2 + 1)) on one lane, as bls_pairing.h final_exp starts
static fp12_t easy_one_lane(const fp12_t& f) {
  const fp12_t t = fp12_mul(fp12_conj(f), fp12_inv(f));
  return fp12_mul(fp12_frob2(t), t);
}

static int fails = 0;
static void check(const char* name, bool ok) {
  printf("%s %s\n", ok ? "ok" : "FAIL", name);
  if (!ok) ++fails;
}

// every check; the number of failed ones
extern "C" int cs_selftest() {
  fails = 0;
  tm_emu_ops o;
  // 1. squaring values
  {
    bool cyc = true, gen = true;
    for (int it = 0; it <= 20; ++it) {
      const fp12_t g = it == 20 ? fp12_one() : easy_one_lane(rand_fp12());
      const fp12_t h = tm_emu_to_fp12(o.cyc_sqr(tm_emu_from_fp12(g)));
      cyc = cyc && fp12_same(h, fp12_cyclotomic_sqr(g));
      gen = gen && fp12_same(h, fp12_sqr(g));
    }
    check("sqr: 20 cyclotomic elements and 1 equal fp12_cyclotomic_sqr", cyc);
    check("sqr: 20 cyclotomic elements and 1 equal fp12_sqr", gen);
    // extreme operands: every coefficient 2p (the largest value a team holds), every limb below the
    // top one at 2^28 - 1 under 2p's top limb less one, and the two alternating with 0.  Off the
    // cyclotomic subgroup the lane function is still the same polynomial map as the one-lane
    // formula, which takes the operands reduced.
    const fp_t two_p = {BGV_2P_LIMBS};
    fp_t full = two_p;
    for (int l = 0; l < NL - 1; ++l) full.v[l] = LMASK;
    full.v[NL - 1] -= 1;
    const fp_t pat[3] = {two_p, full, fp_zero()};
    bool ext = true;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        for (int ph = 0; ph < 2; ++ph) {
          tm_emu_t x, xr;
          for (int c = 0; c < BGV_TEAM_COMPS; ++c) {
            // ph 0: alternate over re / im; ph 1: over the two halves of an Fp4 pair
            const bool first = ph == 0 ? (c & 1) == 0 : (c >> 1) < 3;
            x.c[c] = first ? pat[a] : pat[b];
            xr.c[c] = fp_mul(x.c[c], fp_one());  // the same value, below 1.1 p
          }
          const fp12_t h = tm_emu_to_fp12(o.cyc_sqr(x));
          ext = ext && fp12_same(h, fp12_cyclotomic_sqr(tm_emu_to_fp12(xr)));
          for (int c = 0; c < BGV_TEAM_COMPS; ++c) {  // the result is a team value again
            const fp_t r = o.cyc_sqr(x).c[c];
            for (int l = 0; l < NL - 1; ++l) ext = ext && r.v[l] <= LMASK;
            ext = ext && r.v[NL - 1] <= two_p.v[NL - 1];
          }
        }
    check("sqr: operands with every limb at its bound", ext);
    const fp12_t nc = rand_fp12();
    check("sqr: off the cyclotomic subgroup it differs from fp12_sqr",
          !fp12_same(tm_emu_to_fp12(o.cyc_sqr(tm_emu_from_fp12(nc))), fp12_sqr(nc)));
  }
  // 2. easy part
  {
    bool d6 = true, n2 = true, inv = true, easy = true;
    for (int it = 0; it < 4; ++it) {
      const fp12_t f = rand_fp12();
      const tm_emu_t F = tm_emu_from_fp12(f);
      d6 = d6 && o.is_fp6(o.mul(F, o.conj(F)));
      tm_emu_t G;
      const tm_emu_t N = tm_easy_norm(o, F, &G);
      for (int c = 2; c < BGV_TEAM_COMPS; ++c) n2 = n2 && fp_is_zero(N.c[c]);
      const fp_t n = o.norm2(N);
      const fp_t ninv = fp_inv(n);
      inv = inv && fp12_same(tm_emu_to_fp12(o.mul(G, o.scale2(N, ninv))), fp12_inv(f));
      easy = easy && fp12_same(tm_emu_to_fp12(tm_easy_finish(o, F, G, N, ninv)), easy_one_lane(f));
    }
    check("easy: D = f conj(f) lies in Fp6", d6);
    check("easy: N = D E lies in Fp2", n2);
    check("easy: conj(f) E conj2(N) / n equals fp12_inv(f)", inv);
    check("easy: t equals the one-lane f^((p^6 - 1)(p^2 + 1))", easy);
  }
  // Miller values: e(P, Q) e(-P, Q) (pairing value 1) and e(P, Q) e(-P, Q2) (not 1)
  const uint8_t m0[32] = {1, 2, 3}, m1[32] = {9, 8, 7, 6};
  const g2_jac Q0 = hash_to_g2(m0, 32), Q1 = hash_to_g2(m1, 32);
  const g1_jac Pk = jac_mul_u64(jac_from_aff(g1_generator()), 0x1234567890ABCDEFull);
  const g1_jac Pn = jac_neg(Pk);
  const fp12_t valid = fp12_mul(miller_loop1(Pk, Q0), miller_loop1(Pn, Q0));
  const fp12_t perturbed = fp12_mul(miller_loop1(Pk, Q0), miller_loop1(Pn, Q1));
  const fp12_t f1 = rand_fp12(), f2 = rand_fp12();
  bool z;
  // 3. the final exponentiation's value
  {
    bool same = true;
    const fp12_t in[4] = {f1, f2, valid, perturbed};
    for (int i = 0; i < 4; ++i) {
      const fp12_t U = tm_emu_to_fp12(team_final_exp_cyc(tm_emu_from_fp12(in[i]), &z));
      same = same && !z && fp12_same(U, final_exp(in[i]));
    }
    check("final: U equals the one-lane final_exp", same);
  }
  // 4. the gu convention
  {
    const tm_emu_t F1 = tm_emu_from_fp12(f1), F2 = tm_emu_from_fp12(f2);
    const tm_emu_t old1 = tm_final_exp_u(o, F1);
    const tm_emu_t new1 = team_gu(team_final_exp_cyc(F1, &z)), new2 = team_gu(team_final_exp_cyc(F2, &z));
    check("gu: u_old conj(1 + conj(U)) lies in Fp6 for the same f", o.is_fp6(o.mul(old1, o.conj(new1))));
    check("gu: new against new lies in Fp6 for the same f", o.is_fp6(o.mul(new1, o.conj(new1))));
    check("gu: it does not for two different pairing values",
          !o.is_fp6(o.mul(old1, o.conj(new2))) && !o.is_fp6(o.mul(new1, o.conj(new2))));
    check("gu: U = 1 for e(P, Q) e(-P, Q)",
          fp12_is_one(tm_emu_to_fp12(team_final_exp_cyc(tm_emu_from_fp12(valid), &z))) && !z);
    bool agree = true;
    const fp12_t in[3] = {f1, valid, perturbed};
    const bool want[3] = {false, true, false};
    for (int i = 0; i < 3; ++i) {
      const tm_emu_t F = tm_emu_from_fp12(in[i]);
      const bool v = o.is_fp6(team_gu(team_final_exp_cyc(F, &z)));
      agree = agree && v == want[i] && v == tm_final_exp_is_one(o, F) && !z;
    }
    check("gu: verdicts agree with tm_final_exp_is_one (random, valid, perturbed)", agree);
  }
  // 5. batched inversion: five values, the third zero
  {
    fp_t v[5], out[5];
    for (int i = 0; i < 5; ++i) v[i] = i == 2 ? fp_zero() : rand_fp();
    int calls = 0;
    const uint32_t zero = tm_batch_inv<5>(v, out, [&](const fp_t& x) {
      ++calls;
      return fp_inv(x);
    });
    check("inv: the zero slot is flagged, no other", zero == 1u << 2);
    bool exact = calls == 1;
    for (int i = 0; i < 5; ++i)
      if (i != 2) exact = exact && fp_eq(out[i], fp_inv(v[i])) && fp_eq(fp_mul(out[i], v[i]), fp_one());
    check("inv: the other four inverses are exact, from one inversion", exact);
    // p is zero too (a team's n = N0^2 + N1^2 is reduced below 2p only)
    const fp_t p_ = {BGV_P_LIMBS};
    v[4] = p_;
    check("inv: a zero held as p is flagged",
          tm_batch_inv<5>(v, out, [](const fp_t& x) { return fp_inv(x); }) == (1u << 2 | 1u << 4));
  }
  fflush(stdout);
  return fails;
}

int main() { return cs_selftest() ? 1 : 0; }
