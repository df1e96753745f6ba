"""GPU: both debug hooks at 2 sets and at 64 sets, pinned to oracle/bls12381.py.

The hooks lay their sets out with one slot builder (bgv_calls.cpp debug_slots): cached-key
slots padded to a wave, slot i's randomizer the i-th nonzero splitmix64 word of the seed.  2 sets
is the smallest call bgv_debug_uniform takes and the longest padding (62 slots); at 64 sets the
padding must add nothing and bgv_debug_prepare's one group is full.  The sets name 1, 2 or 3
cached keys in turn, so a slot's pk_off is not its index.

With sig_i = sk_i H(m) and pk_i = sk_i G1 (sk_i the sum of the set's keys), every expected value
is a power of gt_m = e(G1, H(m)):
  * bgv_debug_prepare returns set i's Miller value f_i with final_exp(f_i) = gt_m^(r_i sk_i).  Per
    root m, final_exp(prod_i f_i^(i + 1)) must equal gt_m^(sum (i + 1) r_i sk_i): one final
    exponentiation per root, and the distinct weights tell a value in the wrong slot from the
    right one.  H(m_i) is compared per slot, bit for bit.  Both paths.
  * bgv_debug_uniform's values are checked as tests/test_gpu_r06.py checks them at 40 sets.
Bit-exact integer work.  Reference: packages/beacon-node/src/chain/bls/maybeBatch.ts:18-25.
"""
import hashlib
import json
import os

import pytest

from tests.test_pairing_golden import f12_from_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [2, 64]
NMAX = 64
SEED = 0x5EED0009


@pytest.fixture(scope="module")
def world():
    """The context with the golden keys cached, and per set: its keys, its summed secret key."""
    from lodestar_amd import native
    from oracle import bls12381 as o  # checker only
    keys = json.load(open(os.path.join(HERE, "golden", "keys.json")))
    sks = [int(v, 16) for v in keys["sk"]]
    c = native.Context([0])
    c.pubkeys_put(0, b"".join(bytes.fromhex(k) for k in keys["pk_compressed"]), native.PK_COMPRESSED)
    members = [[(i + q) % len(sks) for q in range(1 + i % 3)] for i in range(NMAX)]
    agg = [sum(sks[k] for k in m) % o.R for m in members]
    roots = [hashlib.sha256(b"debug-hooks-root-%d" % q).digest() for q in range(2)]
    hashed = [o.hash_to_g2(r) for r in roots]
    gts = [o.pairing(o.G1, h) for h in hashed]
    yield {"ctx": c, "members": members, "agg": agg, "roots": roots, "h192": [o.g2_serialize(h) for h in hashed],
           "gt": gts}
    c.close()


def _sets(world, n, root_of):
    from lodestar_amd import native
    c = world["ctx"]
    msgs = [world["roots"][root_of(i)] for i in range(n)]
    sigs = c.sign(b"".join(world["agg"][i].to_bytes(32, "big") for i in range(n)), b"".join(msgs))
    return [native.SetSpec(msgs[i], sigs[96 * i:96 * i + 96], pk_indices=world["members"][i]) for i in range(n)]


@pytest.mark.parametrize("path", ["bulk", "latency"])
@pytest.mark.parametrize("n", SIZES)
def test_debug_prepare_values(world, n, path):
    from lodestar_amd import native
    from oracle import bls12381 as o  # checker only
    from tools.gen_golden_r04 import randomizers
    sets = _sets(world, n, lambda i: i & 1)
    out = world["ctx"].debug_prepare(sets, native.PATH_BULK if path == "bulk" else native.PATH_LATENCY, seed=SEED)
    assert len(out) == n
    rs = [r for _, r in randomizers(SEED, n)]
    for i, (h, _, ss, ps) in enumerate(out):
        assert (ss, ps) == (0, 0), i
        assert h == world["h192"][i & 1], i
    for q in range(2):
        prod, a = None, 0
        for i in range(q, n, 2):
            f = o.f12_pow(f12_from_bytes(out[i][1]), i + 1)
            prod = f if prod is None else o.f12_mul(prod, f)
            a += (i + 1) * rs[i] * world["agg"][i]
        assert o.final_exp(prod) == o.f12_pow(world["gt"][q], a % o.R), q


@pytest.mark.parametrize("n", SIZES)
def test_debug_uniform_values(world, n):
    from oracle import bls12381 as o  # checker only
    from tools.gen_golden_r04 import randomizers
    sets = _sets(world, n, lambda i: 0)
    rs = [r for _, r in randomizers(SEED, n)]
    full = (1 << n) - 1
    tests = [(sum(1 << k for k in range(n) if k & 1), False),  # a pattern test
             (full & ~(1 << (n - 1)), True)]                    # the weighted test, the last slot dead
    first, vals = world["ctx"].debug_uniform(sets, SEED, tests)

    def expect(mask, weighted):
        a = sum(((k + 1) if weighted else 1) * rs[k] * world["agg"][k] for k in range(n) if (mask >> k) & 1) % o.R
        return o.f12_pow(world["gt"][0], a)

    assert o.final_exp(f12_from_bytes(first)) == expect(full, False)
    assert len(vals) == len(tests)
    for (mask, weighted), (pk576, sig576) in zip(tests, vals):
        e = expect(mask, weighted)
        assert o.final_exp(f12_from_bytes(pk576)) == e, (hex(mask), weighted, "pubkey-sum pair")
        assert o.final_exp(f12_from_bytes(sig576)) == o.f12_inv(e), (hex(mask), weighted, "signature pair")
