"""One-shot utility calls at one element and at one past a wavefront (n = 1, n = 65), bit-exact
against oracle/bls12381.py: bgv_sign, and bgv_pubkeys_validate called without the optional
uncompressed output (out96 = NULL), which lodestar_amd.native never does.  The other one-shot
calls are compared with the oracle's golden vectors in tests/test_gpu_parity.py (an empty
aggregate among non-empty ones included: tests/golden/next.json "aggregates")."""
import ctypes
import hashlib
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 65]


def load(name):
    return json.load(open(os.path.join(GOLD, name)))


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd import native
    c = native.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sign_reference():
    """65 (sk, msg, oracle signature): five roots; three full-size keys (the first one included,
    which is the n = 1 case) and small ones, which keep the oracle's 65 scalar products short."""
    from oracle import bls12381 as o  # checker only
    roots = [hashlib.sha256(b"oneshot-root-%d" % i).digest() for i in range(5)]
    hashed = [o.hash_to_g2(r) for r in roots]
    sks = [o.interop_secret_key(i) if i in (0, 31, 64) else 0x1001 + 257 * i for i in range(65)]
    return [(sk, roots[i % 5], o.g2_compress(o.g2_mul(hashed[i % 5], sk))) for i, sk in enumerate(sks)]


@pytest.mark.parametrize("n", SIZES)
def test_sign_matches_oracle(ctx, sign_reference, n):
    ref = sign_reference[:n]
    sigs = ctx.sign(b"".join(sk.to_bytes(32, "big") for sk, _, _ in ref), b"".join(m for _, m, _ in ref))
    assert len(sigs) == 96 * n
    for i, (_, _, want) in enumerate(ref):
        assert sigs[96 * i:96 * i + 96] == want, i


@pytest.fixture(scope="module")
def validate_reference():
    """65 (compressed key, oracle code): the golden edge cases, coded by the oracle here, in
    front of interop keys, which tests/test_oracle_kat.py pins as valid; the first is valid."""
    from oracle import bls12381 as o  # checker only
    edge = [bytes.fromhex(c["pk"]) for c in load("next.json")["pubkeys"]]
    ref = [(k, o.pubkey_validate(k)) for k in edge]
    ref += [(bytes.fromhex(k), 0) for k in load("keys.json")["pk_compressed"][20:20 + 65 - len(edge)]]
    assert len(ref) == 65 and ref[0][1] == 0 and any(code for _, code in ref)
    return ref


@pytest.mark.parametrize("n", SIZES)
def test_pubkeys_validate_without_uncompressed_output(ctx, validate_reference, n):
    from lodestar_amd import native
    ref = validate_reference[:n]
    st = (ctypes.c_int32 * n)(*([7] * n))
    rc = ctx.lib.bgv_pubkeys_validate(ctx._h, native._buf(b"".join(k for k, _ in ref)), n, st, None)
    assert rc == 0
    assert list(st) == [-code for _, code in ref]
    # and the same codes with the output
    codes, recs = ctx.pubkeys_validate([k for k, _ in ref])
    assert codes == list(st)
