"""CPU tests of what the bulk k_prep's task_sig and task_hash run per set (tests/native/prepsim.cpp,
the host build of bls_curve.h / bls_hash.h with the bulk unit's deferred-reduction products and every
lazy bound checked at run time), against the oracle, oracle/bls12381.py, as affine points:

  * jac_madd, the complete mixed addition: generic, acc == Q, acc == -Q, acc at infinity, each with
    the accumulator at Z == 1 and Z != 1, equal to jac_add of the same operands and to the oracle;
  * [|x|]P's subgroup check and r * P (jac_mul_glv_aff) of an affine point;
  * hash_to_g2_sum, the hash with one isogeny: the golden cases (the RFC 9380 vectors among them),
    the padding-boundary messages, and at the map level equal field elements (the E2' doubling),
    opposite ones (the sum at infinity) and u == 0 (the SSWU exceptional case).
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

from oracle import bls12381 as o
from tests import hostsim as hs
from tests import prepsim as ps
from tests.randomizer_edges import EDGE_WORDS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORDS = [1, 7, 8, 9, 0x88888888, 0x99999999, 0x77777777, 0x80000000, 0xFFFFFFFF]
X2 = (o.X * o.X) % o.R
PAD_EDGE_LENGTHS = [8, 9, 16, 17, 18, 72, 73, 137]  # len + 111 on and around a SHA-256 block boundary


@pytest.fixture(scope="module")
def L():
    return ps.lib()


@pytest.fixture(scope="module")
def points():
    return o.g2_mul(o.G2, 0x7654321), o.g2_mul(o.G2, 0x1234567)


@pytest.mark.parametrize("form", [ps.FORM_JAC, ps.FORM_AFF], ids=["jacobian", "z-one"])
def test_madd_cases(L, points, form):
    p, q = points
    out = hs.buf(192)
    for name, acc, want in (("generic", p, o.g2_add(p, q)), ("acc == Q", q, o.g2_add(q, q)),
                            ("acc == -Q", o.g2_neg(q), None)):
        rc = L.ps_g2_madd(out, hs.g2_b(acc), form, hs.g2_b(q))
        assert rc & 2, name  # the same point as jac_add
        assert bool(rc & 1) == (want is not None), name
        if want is not None:
            assert hs.b_g2(out.raw) == want, name


def test_madd_accumulator_at_infinity(L, points):
    _, q = points
    out = hs.buf(192)
    assert L.ps_g2_madd(out, hs.g2_b(q), ps.FORM_INF, hs.g2_b(q)) == 3
    assert hs.b_g2(out.raw) == q


def scalars():
    ks = WORDS + [w << 32 for w in WORDS] + [(w << 32) | w for w in WORDS]
    ks += [0xFFFFFFFFFFFFFFFF, (0x99999999 << 32) | 0x77777777, (1 << 32) | 0xFFFFFFFF]
    rnd = random.Random(0x17)
    ks += [rnd.getrandbits(64) for _ in range(48)]
    ks += EDGE_WORDS  # the list the device routes are run over (tests/test_gpu_randomizer_edges.py)
    return sorted(set(ks))


def test_mul_glv_aff(L, points):
    """[lo32(k)] P + [hi32(k)] E(P) with the oracle's arithmetic; E(P) = [x^2] P."""
    p, _ = points
    ep = o.g2_mul(p, X2)
    out = hs.buf(192)
    for k in scalars():
        assert L.ps_g2_mul_glv_aff(out, hs.g2_b(p), ctypes.c_uint64(k))
        assert hs.b_g2(out.raw) == o.g2_add(o.g2_mul(p, k & 0xFFFFFFFF), o.g2_mul(ep, k >> 32)), hex(k)
    assert L.ps_g2_mul_glv_aff(out, hs.g2_b(p), ctypes.c_uint64(0)) == 0


def test_subgroup_check_aff(L):
    """A valid signature is in G2, the not_in_g2 golden is on the curve and not in G2."""
    sig = o.sign(o.interop_secret_key(5), hashlib.sha256(b"prep-arith").digest())
    assert L.ps_g2_in_subgroup_aff(hs.g2_b(sig)) == 1
    gold = {j["name"]: j for j in json.load(open(os.path.join(GOLD, "verdicts.json")))["jobs"]}
    pt = o.g2_decompress(bytes.fromhex(gold["not_in_g2"]["sets"][0]["sig"]))
    assert o.g2_on_curve(pt) and not o.g2_in_group(pt)
    assert L.ps_g2_in_subgroup_aff(hs.g2_b(pt)) == 0


def _both_hashes(L, msg):
    one, two = hs.buf(192), hs.buf(192)
    assert L.ps_hash_to_g2_sum(one, msg, len(msg)) == 1
    assert L.ps_hash_to_g2(two, msg, len(msg)) == 1
    assert one.raw == two.raw, msg.hex()
    return hs.b_g2(one.raw)


def test_hash_sum_goldens(L):
    gold = json.load(open(os.path.join(GOLD, "hash_to_g2.json")))
    for c in gold["cases"]:
        got = _both_hashes(L, bytes.fromhex(c["msg"]))
        assert o.g2_serialize(got) == bytes.fromhex(c["uncompressed"]), c["msg"]


def test_hash_sum_padding_boundaries_and_roots(L):
    msgs = [bytes((37 * i + 11 * n + 1) & 0xFF for i in range(n)) for n in PAD_EDGE_LENGTHS]
    msgs += [hashlib.sha256(b"prep-arith-root-%d" % i).digest() for i in range(4)]
    for msg in msgs:
        assert _both_hashes(L, msg) == o.hash_to_g2(msg), len(msg)


def _map_oracle(u0, u1):
    q = o.g2_add(o.map_to_curve_g2(u0), o.map_to_curve_g2(u1))
    return None if q is None else o.clear_cofactor_g2(q)


def test_map_sum_exceptional_pairs(L):
    """Equal SSWU points (the sum is the E2' doubling), opposite ones (infinity), and u == 0, where
    the SSWU denominator vanishes, alone and twice."""
    u, v = o.hash_to_field_fp2(b"prep-arith-u", o.DST_POP, 2)
    zero = (0, 0)
    for name, u0, u1 in (("equal", u, u), ("opposite", u, o.f2_neg(u)), ("u0 == 0", zero, v), ("both 0", zero, zero),
                         ("generic", u, v)):
        want = _map_oracle(u0, u1)
        one, two = hs.buf(192), hs.buf(192)
        rc1 = L.ps_map_sum(one, hs.fp2_b(u0), hs.fp2_b(u1))
        rc2 = L.ps_map_two(two, hs.fp2_b(u0), hs.fp2_b(u1))
        assert rc1 == rc2 == (0 if want is None else 1), name
        if want is not None:
            assert one.raw == two.raw and hs.b_g2(one.raw) == want, name
    assert _map_oracle(u, o.f2_neg(u)) is None  # the opposite pair does reach infinity


def test_standalone_sanitizer_run():
    """Each new form against the one it replaces, in a program of its own built with ASan + UBSan."""
    p = subprocess.run([ps.build_san()], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-2000:]
    assert "0 failures" in p.stdout
