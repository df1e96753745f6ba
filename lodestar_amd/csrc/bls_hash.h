// hash_to_G2 on CDNA4: RFC 9380 suite BLS12381G2_XMD:SHA-256_SSWU_RO_, one
// message per lane.  SHA-256 (expand_message_xmd) -> hash_to_field (4 x Fp)
// -> 2 x simplified SWU on E2' -> 3-isogeny (Jacobian, no inversion) -> add
// -> clear_cofactor (psi method, RFC 9380 G.4).
#pragma once
#include "bls_curve.h"
#include "bls_sha256.h"

BGV_HD uint32_t dst_byte(uint32_t i) {
  // BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_ || I2OSP(43, 1)
  const char d[] = BGV_DST_POP;
  return i < BGV_DST_POP_LEN ? (uint32_t)(uint8_t)d[i] : (uint32_t)BGV_DST_POP_LEN;
}

struct xmd_b0_getter {
  const uint8_t* msg;
  uint32_t len;
  // Z_pad(64) || msg || I2OSP(256, 2) || 0x00 || DST_prime
  BGV_HD uint32_t operator()(uint32_t pos) const {
    if (pos < 64) return 0;
    pos -= 64;
    if (pos < len) return msg[pos];
    pos -= len;
    if (pos == 0) return 0x01;
    if (pos == 1) return 0x00;
    if (pos == 2) return 0x00;
    return dst_byte(pos - 3);
  }
};

struct xmd_bi_getter {
  const uint32_t* x;  // 8 words (b0 ^ b_{i-1})
  uint32_t idx;
  BGV_HD uint32_t operator()(uint32_t pos) const {
    if (pos < 32) return (x[pos >> 2] >> (24 - 8 * (pos & 3))) & 0xff;
    if (pos == 32) return idx;
    return dst_byte(pos - 33);
  }
};

// expand_message_xmd(msg, DST_POP, 256) -> 64 big-endian words
BGV_HD void expand_message_xmd_256(uint32_t ub[64], const uint8_t* msg, uint32_t len) {
  uint32_t b0[8], bi[8], x[8];
  xmd_b0_getter g0{msg, len};
  sha256_virtual(b0, g0, 64 + len + 3 + BGV_DST_POP_LEN + 1);
  BGV_UNROLL for (int k = 0; k < 8; ++k) x[k] = b0[k];
  BGV_NO_UNROLL for (uint32_t i = 1; i <= 8; ++i) {
    xmd_bi_getter gi{x, i};
    sha256_virtual(bi, gi, 32 + 1 + BGV_DST_POP_LEN + 1);
    BGV_UNROLL for (int k = 0; k < 8; ++k) {
      // store b_i: dynamic word index (i-1)*8+k; write via unrolled select to stay in registers
      x[k] = b0[k] ^ bi[k];
    }
    BGV_UNROLL for (int j = 1; j <= 8; ++j) {
      if (i == (uint32_t)j) {
        BGV_UNROLL for (int k = 0; k < 8; ++k) ub[(j - 1) * 8 + k] = bi[k];
      }
    }
  }
}

// bits [lo, lo+28) of a big-endian string of 16 u32 words (64 bytes)
BGV_HD uint32_t be_words_bits28(const uint32_t* w, int lo) {
  const int wi = lo >> 5, sh = lo & 31;  // word index from the little end
  uint64_t v = w[15 - wi];
  if (wi + 1 < 16) v |= (uint64_t)w[14 - wi] << 32;
  return (uint32_t)(v >> sh) & LMASK;
}

// 64 big-endian bytes (as 16 words) -> Fp (Montgomery), reduced mod p:
// value = hi * 2^392 + lo  ->  lo * R + hi * R^2 = mont(lo, R^2) + mont(hi, R^3)
BGV_HD fp_t fp_from_be64_words(const uint32_t* w) {
  fp_t lo, hi = fp_zero();
  BGV_UNROLL for (int i = 0; i < NL; ++i) lo.v[i] = be_words_bits28(w, LBITS * i);
  BGV_UNROLL for (int i = 0; i < 5; ++i) hi.v[i] = be_words_bits28(w, 392 + LBITS * i);
  hi.v[4] &= (1u << (512 - 392 - 4 * LBITS)) - 1;
  const fp_t r2 = {BGV_R2}, r3 = {BGV_R3};
  return fp_add(fp_mul(lo, r2), fp_mul(hi, r3));
}

BGV_HD void hash_to_field_fp2(fp2_t* u0, fp2_t* u1, const uint8_t* msg, uint32_t len) {
  uint32_t ub[64];
  expand_message_xmd_256(ub, msg, len);
  u0->c0 = fp_from_be64_words(ub + 0);
  u0->c1 = fp_from_be64_words(ub + 16);
  u1->c0 = fp_from_be64_words(ub + 32);
  u1->c1 = fp_from_be64_words(ub + 48);
}

// ---------------------------------------------------------------------------
// Simplified SWU on E2': y^2 = x^3 + A'x + B', A' = 240i, B' = 1012(1+i), Z = -(2+i)
// ---------------------------------------------------------------------------
// sqrt(-5) in Fp (Montgomery), used to turn sqrt(-n) into sqrt(N(Z) n), N(Z) = 5.
BGV_HD fp_t fp_sqrt_minus5() { return fp_t{BGV_SQRT_M5}; }

// If g is a square in Fp2: *y = sqrt(g), returns true.  Otherwise *y = sqrt(Z g).
// Two Fp exponentiations total (norm root + the Fp2 root).
BGV_NOINLINE bool fp2_sqrt_or_z(fp2_t* y, const fp2_t& g, const fp_t& sqrt_m5) {
  const fp2_t Z = BGV_SSWU_Z;
  const fp_t n = fp_add(fp_sqr(g.c0), fp_sqr(g.c1));
  const fp_t e = fp_pow_p_minus_3_div_4(n);
  const fp_t ne = fp_mul(n, e);
  const fp_t s = fp_mul(ne, e);
  const bool is_sq = fp_eq(s, fp_one()) || fp_is_zero(n);
  const fp2_t h = fp2_select(is_sq, fp2_mul(Z, g), g);
  const fp_t gam = fp_select(is_sq, fp_mul(sqrt_m5, fp_neg(ne)), ne);
  const bool h1z = fp_is_zero(h.c1);
  fp_t d = fp_select(h1z, fp_half(fp_add(h.c0, gam)), h.c0);
  fp_t t = fp_pow_p_minus_3_div_4(d);
  fp_t dt = fp_mul(d, t);
  fp_t s2 = fp_mul(dt, t);
  fp_t a1t2 = fp_half(fp_mul(h.c1, t));
  const bool qr = fp_eq(s2, fp_one());
  y->c0 = fp_select(qr, a1t2, dt);
  y->c1 = fp_select(qr, fp_neg(dt), a1t2);
  return is_sq;
}

// SWU on E2' in two halves so that two maps can share one inversion (Montgomery's trick):
// sswu_den gives den = Z^2 u^4 + Z u^2 (and Z u^2), sswu_finish takes 1/den (any value when
// den == 0: the exceptional case uses x1 = B / (Z A) and never reads it).
BGV_HD fp2_t sswu_den(const fp2_t& u, fp2_t* zu2) {
  const fp2_t Z = BGV_SSWU_Z;
  *zu2 = fp2_mul(Z, fp2_sqr(u));
  return fp2_add(fp2_sqr(*zu2), *zu2);
}

BGV_NOINLINE void sswu_finish(fp2_t* xo, fp2_t* yo, const fp2_t& u, const fp2_t& zu2, const fp2_t& den,
                              const fp2_t& den_inv, const fp_t& sqrt_m5) {
  const fp2_t A = BGV_SSWU_A, B = BGV_SSWU_B;
  const fp2_t bza = BGV_SSWU_B_OVER_ZA, mba = BGV_SSWU_MINUS_B_OVER_A;
  const bool den0 = fp2_is_zero(den);
  fp2_t x1 = fp2_mul(mba, fp2_add(fp2_one(), den_inv));
  x1 = fp2_select(den0, x1, bza);
  fp2_t gx1 = fp2_add(fp2_mul(fp2_add(fp2_sqr(x1), A), x1), B);
  fp2_t r;
  const bool sq = fp2_sqrt_or_z(&r, gx1, sqrt_m5);
  // non-square branch: x2 = Z u^2 x1, y = Z u^3 sqrt(Z gx1)
  fp2_t x2 = fp2_mul(zu2, x1);
  fp2_t y2 = fp2_mul(fp2_mul(zu2, u), r);
  fp2_t x = fp2_select(sq, x2, x1);
  fp2_t y = fp2_select(sq, y2, r);
  if (fp2_sgn0(u) != fp2_sgn0(y)) y = fp2_neg(y);
  *xo = x;
  *yo = y;
}

// returns the SWU point on E2' in affine coordinates
BGV_NOINLINE void sswu_g2(fp2_t* xo, fp2_t* yo, const fp2_t& u, const fp_t& sqrt_m5) {
  fp2_t zu2;
  const fp2_t den = sswu_den(u, &zu2);
  sswu_finish(xo, yo, u, zu2, den, fp2_inv(den), sqrt_m5);
}

// 3-isogeny E2' -> E2 (RFC 9380 E.3), output Jacobian without inversion.
BGV_NOINLINE g2_jac iso_map_g2(const fp2_t& x, const fp2_t& y) {
  const fp2_t xnum[4] = BGV_ISO_XNUM;
  const fp2_t xden[2] = BGV_ISO_XDEN;
  const fp2_t ynum[4] = BGV_ISO_YNUM;
  const fp2_t yden[3] = BGV_ISO_YDEN;
  fp2_t x2 = fp2_sqr(x);
  fp2_t x3 = fp2_mul(x2, x);
  fp2_t xn = fp2_add(fp2_add(fp2_mul(xnum[3], x3), fp2_mul(xnum[2], x2)), fp2_add(fp2_mul(xnum[1], x), xnum[0]));
  fp2_t xd = fp2_add(fp2_add(x2, fp2_mul(xden[1], x)), xden[0]);
  fp2_t yn = fp2_add(fp2_add(fp2_mul(ynum[3], x3), fp2_mul(ynum[2], x2)), fp2_add(fp2_mul(ynum[1], x), ynum[0]));
  fp2_t yd = fp2_add(fp2_add(x3, fp2_mul(yden[2], x2)), fp2_add(fp2_mul(yden[1], x), yden[0]));
  g2_jac r;
  r.z = fp2_mul(xd, yd);
  r.x = fp2_mul(fp2_mul(xn, yd), r.z);
  r.y = fp2_mul(fp2_mul(fp2_mul(y, yn), xd), fp2_sqr(r.z));
  return r;
}

// Simplified SWU on E2' straight to Jacobian coordinates, with no inversion (RFC 9380 6.6.2;
// x = X/Z^2, y = Y/Z^3).  x1 = x1n / x1d, so gx1 = U / V with V = x1d^3, and the square root
// of the ratio runs through the norm method of fp2_sqrt_or_z on U/V = w/n, w = U conj(V),
// n = N(V) in Fp: w/n is a square iff w is (n^2 is), sqrt(N(w/n)) = sqrt(N(w))/n, d = d'/n,
// and with T = n (d' n^3)^((p-3)/4)
//     d^((p+1)/4) = d' T,   h1 d^((p-3)/4) = h1' T,   d^((p-1)/2) = d' n T^2
// (n^(p-1) = 1), so the same two (p-3)/4 exponentiations as sqrt(g) give sqrt(U/V) and
// the inversion of the affine map is gone.  The same point as sswu_g2 (tests/test_hostsim_math.py).
template <class PW>
BGV_NOINLINE g2_jac sswu_g2_jac_t(const fp2_t& u, const fp_t& sqrt_m5) {
  const fp2_t Z = BGV_SSWU_Z, A = BGV_SSWU_A, B = BGV_SSWU_B;
  const fp2_t tv1 = fp2_mul(Z, fp2_sqr(u));
  const fp2_t tv2 = fp2_add(fp2_sqr(tv1), tv1);
  const bool exc = fp2_is_zero(tv2);  // x1 = B / (Z A)
  const fp2_t x1n = fp2_select(exc, fp2_neg(fp2_mul(B, fp2_add(tv2, fp2_one()))), B);
  const fp2_t x1d = fp2_select(exc, fp2_mul(A, tv2), fp2_mul(Z, A));
  const fp2_t d2 = fp2_sqr(x1d);
  const fp2_t V = fp2_mul(d2, x1d);
  const fp2_t U = fp2_add(fp2_mul(fp2_add(fp2_sqr(x1n), fp2_mul(A, d2)), x1n), fp2_mul(B, V));
  const fp2_t w = fp2_mul(U, fp2_conj(V));
  const fp_t n = fp_add(fp_sqr(V.c0), fp_sqr(V.c1));
  const fp_t nw = fp_add(fp_sqr(w.c0), fp_sqr(w.c1));
  const fp_t e = PW::p34(nw);
  const fp_t ne = fp_mul(nw, e);
  const bool sq = fp_eq(fp_mul(ne, e), fp_one()) || fp_is_zero(nw);
  const fp2_t h = fp2_select(sq, fp2_mul(Z, w), w);
  const fp_t gam = fp_select(sq, fp_mul(sqrt_m5, fp_neg(ne)), ne);
  const fp_t d = fp_select(fp_is_zero(h.c1), fp_half(fp_add(h.c0, gam)), h.c0);
  const fp_t T = fp_mul(n, PW::p34(fp_mul(d, fp_mul(fp_sqr(n), n))));
  const fp_t y0 = fp_mul(d, T), y1 = fp_half(fp_mul(h.c1, T));
  const bool qr = fp_eq(fp_mul(fp_mul(d, n), fp_sqr(T)), fp_one());
  fp2_t r;  // sqrt(gx1), or sqrt(Z gx1) when gx1 is not a square
  r.c0 = fp_select(qr, y1, y0);
  r.c1 = fp_select(qr, fp_neg(y0), y1);
  // x = x1 or x2 = tv1 x1; y = r or tv1 u r (= Z u^3 sqrt(Z gx1))
  const fp2_t xn = fp2_mul(x1n, x1d);
  fp2_t y = fp2_select(sq, fp2_mul(fp2_mul(tv1, u), r), r);
  if (fp2_sgn0(u) != fp2_sgn0(y)) y = fp2_neg(y);
  g2_jac o;
  o.x = fp2_select(sq, fp2_mul(tv1, xn), xn);
  o.y = fp2_mul(y, V);
  o.z = x1d;
  return o;
}
BGV_HD g2_jac sswu_g2_jac(const fp2_t& u, const fp_t& sqrt_m5) { return sswu_g2_jac_t<bgv_pow_lane>(u, sqrt_m5); }

// 3-isogeny E2' -> E2 (RFC 9380 E.3) of a Jacobian point: the rational maps in x = X/Z^2
// homogenized with z2 = Z^2 (XN = xnum z2^3, XD = xden z2^2, YN = ynum z2^3, YD = yden z2^3),
// x' = XN / (XD z2), y' = Y YN / (Z^3 YD); output (A D W, C B W^2, W) with A/B = x',
// C/D = y', W = B D.
BGV_NOINLINE g2_jac iso_map_g2_jac(const g2_jac& p) {
  const fp2_t xnum[4] = BGV_ISO_XNUM;
  const fp2_t xden[2] = BGV_ISO_XDEN;
  const fp2_t ynum[4] = BGV_ISO_YNUM;
  const fp2_t yden[3] = BGV_ISO_YDEN;
  const fp2_t X = p.x, z2 = fp2_sqr(p.z);
  const fp2_t z4 = fp2_sqr(z2), z6 = fp2_mul(z4, z2);
  const fp2_t X2 = fp2_sqr(X), X3 = fp2_mul(X2, X);
  const fp2_t X2z2 = fp2_mul(X2, z2), Xz4 = fp2_mul(X, z4);
  const fp2_t XN = fp2_add(fp2_add(fp2_mul(xnum[3], X3), fp2_mul(xnum[2], X2z2)),
                           fp2_add(fp2_mul(xnum[1], Xz4), fp2_mul(xnum[0], z6)));
  const fp2_t XD = fp2_add(fp2_add(X2, fp2_mul(xden[1], fp2_mul(X, z2))), fp2_mul(xden[0], z4));
  const fp2_t YN = fp2_add(fp2_add(fp2_mul(ynum[3], X3), fp2_mul(ynum[2], X2z2)),
                           fp2_add(fp2_mul(ynum[1], Xz4), fp2_mul(ynum[0], z6)));
  const fp2_t YD = fp2_add(fp2_add(X3, fp2_mul(yden[2], X2z2)), fp2_add(fp2_mul(yden[1], Xz4), fp2_mul(yden[0], z6)));
  const fp2_t Bq = fp2_mul(XD, z2);
  const fp2_t Dq = fp2_mul(fp2_mul(p.z, z2), YD);
  const fp2_t Cq = fp2_mul(p.y, YN);
  g2_jac r;
  r.z = fp2_mul(Bq, Dq);
  r.x = fp2_mul(fp2_mul(XN, Dq), r.z);
  r.y = fp2_mul(fp2_mul(Cq, Bq), fp2_sqr(r.z));
  return r;
}

// Doubling on E2' (dbl-2007-bl with a = A' = 240i; jac_dbl is the a = 0 form of E2).  Only the
// sum of two equal SSWU points takes it, so it is written with the eager products.
BGV_NOINLINE g2_jac e2p_dbl(const g2_jac& p) {
  const fp2_t A = BGV_SSWU_A;
  const fp2_t XX = fp2_sqr(p.x), YY = fp2_sqr(p.y), ZZ = fp2_sqr(p.z);
  const fp2_t YYYY = fp2_sqr(YY);
  const fp2_t S = fp2_dbl(fp2_sub(fp2_sub(fp2_sqr(fp2_add(p.x, YY)), XX), YYYY));
  const fp2_t M = fp2_add(fp2_add(fp2_dbl(XX), XX), fp2_mul(A, fp2_sqr(ZZ)));
  const fp2_t T = fp2_sub(fp2_sqr(M), fp2_dbl(S));
  const fp2_t Y8 = fp2_dbl(fp2_dbl(fp2_dbl(YYYY)));
  g2_jac r;
  r.x = T;
  r.y = fp2_sub(fp2_mul(M, fp2_sub(S, T)), Y8);
  r.z = fp2_sub(fp2_sub(fp2_sqr(fp2_add(p.y, p.z)), YY), ZZ);
  return r;
}

// Complete addition of two points of E2' (the SSWU outputs, never at infinity themselves): the
// addition formulas do not involve the curve's coefficients, the doubling does.  Opposite points
// give Z = 0, which iso_map_g2_jac maps to Z = 0.
BGV_HD g2_jac e2p_add(const g2_jac& p, const g2_jac& q) {
  bool hz, rz;
  g2_jac r = jac_add_raw(p, q, &hz, &rz);
  if (hz && rz) r = e2p_dbl(p);  // rare: equal SSWU points
  return r;
}

// hash_to_G2 with one isogeny: the 3-isogeny is a group homomorphism E2' -> E2, so
// iso(q0) + iso(q1) = iso(q0 + q1) with the sum taken on E2' (RFC 9380 6.6.3 notes the same for
// the affine map).  The same point of G2 as hash_to_g2, by another Jacobian representative.
BGV_NOINLINE g2_jac hash_to_g2_sum(const uint8_t* msg, uint32_t len) {
  fp2_t u0, u1;
  hash_to_field_fp2(&u0, &u1, msg, len);
  const fp_t sm5 = fp_sqrt_minus5();
  const g2_jac q0 = sswu_g2_jac(u0, sm5);
  const g2_jac q1 = sswu_g2_jac(u1, sm5);
  return g2_clear_cofactor(iso_map_g2_jac(e2p_add(q0, q1)));
}

// Full hash_to_G2 of one message: a Jacobian point in G2 (both maps in Jacobian form, no
// inversion anywhere).
BGV_NOINLINE g2_jac hash_to_g2(const uint8_t* msg, uint32_t len) {
  fp2_t u0, u1;
  hash_to_field_fp2(&u0, &u1, msg, len);
  const fp_t sm5 = fp_sqrt_minus5();
  const g2_jac q0 = iso_map_g2_jac(sswu_g2_jac(u0, sm5));
  const g2_jac q1 = iso_map_g2_jac(sswu_g2_jac(u1, sm5));
  return g2_clear_cofactor(jac_add(q0, q1));
}
