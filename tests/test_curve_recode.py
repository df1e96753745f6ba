"""CPU tests of the bulk k_prep's point arithmetic (tests/native/curvesim.cpp, the host build of
bls_curve.h / bls_hash.h) against the oracle, oracle/bls12381.py, as affine points: the signed
radix-16 recoding, jac_mul_glv for a Jacobian P (Z != 1) and for P handed over with Z == 1,
the subgroup check, and hash_to_g2 on its golden cases."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

from oracle import bls12381 as o
from tests import curvesim as cs
from tests import hostsim as hs
from tests.randomizer_edges import EDGE_WORDS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORDS = [0, 1, 7, 8, 9, 0x88888888, 0x99999999, 0x77777777, 0x80000000, 0xFFFFFFFF]
X2 = (o.X * o.X) % o.R


@pytest.fixture(scope="module")
def L():
    return cs.lib()


def scalars():
    ks = [w for w in WORDS if w] + [w << 32 for w in WORDS if w]  # each word in either half, the other 0
    ks += [(w << 32) | w for w in WORDS if w]  # and in both
    ks += [0xFFFFFFFFFFFFFFFF, (0x99999999 << 32) | 0x77777777, (1 << 32) | 0xFFFFFFFF]
    rnd = random.Random(0x16)
    ks += [rnd.getrandbits(64) for _ in range(64)]
    ks += EDGE_WORDS  # the list the device routes are run over (tests/test_gpu_randomizer_edges.py)
    return sorted(set(ks))


def test_recoding(L):
    """sum d_j 16^j + carry 16^8 == a with |d_j| <= 8, for the edge words and 1,000 seeded ones."""
    rnd = random.Random(0xC0DE)
    d = (ctypes.c_int32 * 9)()
    for a in WORDS + [rnd.getrandbits(32) for _ in range(1000)]:
        L.cs_recode16(ctypes.c_uint32(a), d)
        assert all(abs(d[j]) <= 8 for j in range(8)), hex(a)
        assert d[8] in (0, 1), hex(a)
        assert sum(d[j] * 16 ** j for j in range(9)) == a, hex(a)


def _expect(mul, add, p, ep, k):
    """[lo32(k)] P + [hi32(k)] E(P) with the oracle's arithmetic; E(P) = [x^2] P from the oracle."""
    return add(mul(p, k & 0xFFFFFFFF), mul(ep, k >> 32))


@pytest.mark.parametrize("form", [cs.FORM_JAC, cs.FORM_AFF], ids=["jacobian", "affine"])
def test_mul_glv_g1(L, form):
    p = o.g1_mul(o.G1, 0x1234567 + form)
    ep = o.g1_mul(p, X2)
    out = hs.buf(96)
    for k in scalars():
        assert L.cs_g1_mul_glv(out, hs.g1_b(p), ctypes.c_uint64(k), form)
        assert hs.b_g1(out.raw) == _expect(o.g1_mul, o.g1_add, p, ep, k), hex(k)


@pytest.mark.parametrize("form", [cs.FORM_JAC, cs.FORM_AFF], ids=["jacobian", "affine"])
def test_mul_glv_g2(L, form):
    p = o.g2_mul(o.G2, 0x7654321 + form)
    ep = o.g2_mul(p, X2)
    out = hs.buf(192)
    for k in scalars():
        assert L.cs_g2_mul_glv(out, hs.g2_b(p), ctypes.c_uint64(k), form)
        assert hs.b_g2(out.raw) == _expect(o.g2_mul, o.g2_add, p, ep, k), hex(k)


def test_mul_glv_zero_and_infinity(L):
    """k == 0 gives infinity; P == infinity gives infinity for every scalar."""
    o1, o2 = hs.buf(96), hs.buf(192)
    assert L.cs_g1_mul_glv(o1, hs.g1_b(o.G1), ctypes.c_uint64(0), cs.FORM_JAC) == 0
    assert L.cs_g2_mul_glv(o2, hs.g2_b(o.G2), ctypes.c_uint64(0), cs.FORM_AFF) == 0
    for k in (1, 0xFFFFFFFFFFFFFFFF, 0x99999999 << 32, 0x0123456789ABCDEF):
        assert L.cs_g1_mul_glv(o1, hs.g1_b(o.G1), ctypes.c_uint64(k), cs.FORM_INF) == 0
        assert L.cs_g2_mul_glv(o2, hs.g2_b(o.G2), ctypes.c_uint64(k), cs.FORM_INF) == 0


def test_subgroup_check(L):
    """A valid signature is in G2, the not_in_g2 golden is on the curve and not in G2."""
    sig = o.sign(o.interop_secret_key(5), hashlib.sha256(b"curve-recode").digest())
    assert L.cs_g2_in_subgroup(hs.g2_b(sig)) == 1
    gold = {j["name"]: j for j in json.load(open(os.path.join(GOLD, "verdicts.json")))["jobs"]}
    aff = hs.buf(192)
    assert L.cs_g2_decompress(aff, bytes.fromhex(gold["not_in_g2"]["sets"][0]["sig"])) == 0
    pt = hs.b_g2(aff.raw)
    assert o.g2_on_curve(pt) and not o.g2_in_group(pt)
    assert L.cs_g2_in_subgroup(aff.raw) == 0


def test_hash_to_g2_goldens(L):
    gold = json.load(open(os.path.join(GOLD, "hash_to_g2.json")))
    out = hs.buf(192)
    for c in gold["cases"]:
        msg = bytes.fromhex(c["msg"])
        assert L.cs_hash_to_g2(out, msg, len(msg)) == 1
        assert o.g2_serialize(hs.b_g2(out.raw)) == bytes.fromhex(c["uncompressed"]), c["msg"]


# Message lengths that put the hashed stream Z_pad(64) | msg | 3 bytes | DST'(44) of len + 111 bytes
# on and around a SHA-256 block boundary: len + 111 = 55, 56, 63, 0, 1 (mod 64), the same one
# block further (72, 73), and one unaligned long message.  The golden lengths (0, 3, 32, 100, 255)
# reach none of them.
PAD_EDGE_LENGTHS = [8, 9, 16, 17, 18, 72, 73, 137]


def pad_edge_messages():
    """One message per length, every byte depending on its position and on the length."""
    return [bytes((37 * i + 11 * n + 1) & 0xFF for i in range(n)) for n in PAD_EDGE_LENGTHS]


def test_hash_to_g2_padding_boundaries(L):
    assert sorted({(n + 111) % 64 for n in PAD_EDGE_LENGTHS[:5]}) == [0, 1, 55, 56, 63]
    out = hs.buf(192)
    for msg in pad_edge_messages():
        assert L.cs_hash_to_g2(out, msg, len(msg)) == 1
        assert o.g2_serialize(hs.b_g2(out.raw)) == o.g2_serialize(o.hash_to_g2(msg)), len(msg)


def test_standalone_sanitizer_run():
    """The recoding and scalar-multiplication cases once more in a program of their own built with
    ASan + UBSan (checked there against jac_mul_u64)."""
    p = subprocess.run([cs.build_san()], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-2000:]
    assert "0 failures" in p.stdout
