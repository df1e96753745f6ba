"""The closing kernels' final exponentiation on the host (tests/native/cycsim.cpp over bls_team.h):
Granger-Scott squarings lane by lane against fp12_cyclotomic_sqr and fp12_sqr (cyclotomic elements,
1, operands with every limb at its bound, and a non-cyclotomic element the two must disagree on);
the easy part's D in Fp6, N in Fp2, inverse and value; U against the one-lane final_exp; the gu
convention (u = 1 + conj(U) against tm_final_exp_u's u, verdicts against tm_final_exp_is_one); the
batched inversion with a zero among five values.  The program runs once under AddressSanitizer +
UBSan as a stand-alone program; the -O2 library runs the same checks and gives U to compare with the
oracle's final exponentiation raised to the chain's factor (BGV_FINAL_EXP_CHAIN_FACTOR)."""
import random

from oracle import bls12381 as o
from tests import cycsim
from tests import hostsim as hs

WANT = (
    "sqr: 20 cyclotomic elements and 1 equal fp12_cyclotomic_sqr",
    "sqr: 20 cyclotomic elements and 1 equal fp12_sqr",
    "sqr: operands with every limb at its bound",
    "sqr: off the cyclotomic subgroup it differs from fp12_sqr",
    "easy: D = f conj(f) lies in Fp6",
    "easy: N = D E lies in Fp2",
    "easy: conj(f) E conj2(N) / n equals fp12_inv(f)",
    "easy: t equals the one-lane f^((p^6 - 1)(p^2 + 1))",
    "final: U equals the one-lane final_exp",
    "gu: u_old conj(1 + conj(U)) lies in Fp6 for the same f",
    "gu: it does not for two different pairing values",
    "gu: U = 1 for e(P, Q) e(-P, Q)",
    "gu: verdicts agree with tm_final_exp_is_one (random, valid, perturbed)",
    "inv: the zero slot is flagged, no other",
    "inv: the other four inverses are exact, from one inversion",
)


def test_checks_under_sanitizers():
    code, lines, err = cycsim.run("san")
    print("\n".join(lines))
    assert code == 0, (lines, err[-2000:])
    assert lines and all(ln.startswith("ok ") for ln in lines), lines
    names = {ln[3:] for ln in lines}
    for w in WANT:
        assert w in names, w


def test_checks_at_O2():
    assert cycsim.lib().cs_selftest() == 0


def test_U_is_the_oracle_pairing_value_to_the_chain_factor():
    L = cycsim.lib()
    k = L.cs_chain_factor()
    assert k == 3  # 3 (p^4 - p^2 + 1) / r = (x-1)^2 (x+p) (x^2+p^2-1) + 3
    rnd = random.Random(0xC1C)
    f = tuple((rnd.randrange(o.P), rnd.randrange(o.P)) for _ in range(6))
    p = o.g1_mul(o.G1, rnd.randrange(1, o.R))
    q = o.g2_mul(o.G2, rnd.randrange(1, o.R))
    m = o.miller_loop(p, q)
    valid = o.f12_mul(m, o.miller_loop(o.g1_neg(p), q))
    for g, one in ((f, False), (m, False), (valid, True)):
        out = hs.buf(576)
        assert L.cs_final_exp_cyc(out, hs.fp12_b_tower(o.f12_to_tower_list(g))) == 0
        want = o.f12_pow(o.final_exp(g), k)
        assert hs.b_fp12_tower(out.raw) == o.f12_to_tower_list(want)
        assert (want == o.F12_ONE) == one
        assert L.cs_verdict(hs.fp12_b_tower(o.f12_to_tower_list(g))) == (1 if one else 0)
