"""GPU: the bulk k_prep with mixed additions for the affine signature and one isogeny per hash
(bgv_k_tasks.h task_sig / task_hash), at its smallest size: 130 one-set jobs of distinct roots, two
full 64-slot groups and a ragged third.

  * test_bulk_verdicts_under_edge_randomizers (a child process whose BGV_LATENCY_MAX=0 sends the
    call down the bulk path): per edge word k of tests/randomizer_edges.py placed in a slot through
    bgv_set_rng_seed, 130 valid jobs verify in one batch with no retry -- the batch equation
    prod e(r_i pk_i, H(m_i)) = e(G1, sum r_i sig_i) held, so H, r sig and r pk of every slot are
    consistent under that randomizer -- and the call with one wrong message, one wrong key and the
    three undecodable classes of tests/golden/verdicts.json (bad encoding, off the curve, not in
    G2) returns per-job mode's codes.
  * test_bulk_prepare_values: bgv_debug_prepare(PATH_BULK) of the 130 sets.  The hook returns H(m)
    and f = MillerLoop(r pk, H(m)) per set (r sig leaves the device only inside the uniform hook's
    signature pair, which tests/test_gpu_randomizer_edges.py route 4 runs over every edge word).
    H(m) equals the CPU restatement byte for byte for every set and oracle/bls12381.py for every
    13th; final_exp(f) of the edge slot equals e(G1, H(m))^(r sk) from the oracle, bit-exact.
  * test_latency_call_unchanged: one 64-set call of the latency path, the same checks, and the same
    pairing values as the bulk path for every set.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 130
WRONG_KEY, WRONG_MSG, BAD_FLAG, OFF_CURVE, NOT_IN_G2 = 3, 66, 129, 63, 64
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# all-ones halves, a zero half either side, digits at the table's ends (7, 8, 9 = -7 + carry), the
# full carry chain, both top carries
WORDS = [0xFFFFFFFF, 0xFFFFFFFF << 32, 0xFFFFFFFFFFFFFFFF, 8, 9 << 32, (0x88888889 << 32) | 7, (0x99999999 << 32) | 0x77777777]
SLOTS = [0, 63, 64, 127, 128, 129, 65]  # both sides of each group boundary and the ragged group


def _sks():
    return [int.from_bytes(hashlib.sha256(b"prep-arith-%d" % i).digest(), "little") % R for i in range(N)]


def _roots():
    return [hashlib.sha256(b"prep-arith-root-%d" % i).digest() for i in range(N)]


def _child():
    sys.path.insert(0, ROOT)
    from lodestar_amd import native
    from tests.randomizer_edges import seed_for
    skb = [sk.to_bytes(32, "big") for sk in _sks()]
    ctx = native.Context([0])
    ctx.keygen(b"".join(skb), cache_first=0, want_pubkeys=False)
    roots = _roots()
    sigs = ctx.sign(b"".join(skb), b"".join(roots))
    sigs = [sigs[96 * i:96 * i + 96] for i in range(N)]
    valid = [([native.SetSpec(roots[i], sigs[i], pk_indices=[i])], True) for i in range(N)]
    out = {"valid": [], "retries": []}
    try:
        for k, slot in zip(WORDS, SLOTS):
            ctx.set_rng_seed(seed_for(k, slot))
            st = native.BgvStats()
            out["valid"].append(ctx.verify_jobs(valid, native.MODE_WORKER, st))
            out["retries"].append(st.batch_retries)
        gold = {j["name"]: j for j in json.load(open(os.path.join(ROOT, "tests", "golden", "verdicts.json")))["jobs"]}
        keys = list(range(N))
        keys[WRONG_KEY] = WRONG_KEY + 1
        roots[WRONG_MSG] = hashlib.sha256(b"another root").digest()
        for i, name in ((BAD_FLAG, "bad_flag"), (OFF_CURVE, "off_curve"), (NOT_IN_G2, "not_in_g2")):
            sigs[i] = bytes.fromhex(gold[name]["sets"][0]["sig"])
        jobs = [([native.SetSpec(roots[i], sigs[i], pk_indices=[keys[i]])], True) for i in range(N)]
        ctx.set_rng_seed(seed_for(WORDS[2], WRONG_KEY))
        st = native.BgvStats()
        out["worker"] = ctx.verify_jobs(jobs, native.MODE_WORKER, st)
        out["mixed_retries"] = st.batch_retries
        out["alone"] = ctx.verify_jobs(jobs, native.MODE_PER_JOB)
    finally:
        ctx.set_rng_seed(0)
        ctx.close()
    print(json.dumps(out))


@pytest.mark.gpu
def test_bulk_verdicts_under_edge_randomizers():
    env = dict(os.environ, BGV_LATENCY_MAX="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for k, got, retries in zip(WORDS, res["valid"], res["retries"]):
        assert got == [1] * N, hex(k)
        assert retries == 0, hex(k)  # the one batch equation held
    want = [1] * N
    want[WRONG_KEY] = want[WRONG_MSG] = 0
    want[BAD_FLAG], want[OFF_CURVE], want[NOT_IN_G2] = -1, -2, -3
    assert res["alone"] == want
    assert res["worker"] == res["alone"]
    assert res["mixed_retries"] > 0  # the batch failed as a whole and was taken apart


@pytest.fixture(scope="module")
def world():
    from lodestar_amd import native
    from oracle.cpu import blscpu  # the CPU restatement: checker only
    sks = _sks()
    skb = [sk.to_bytes(32, "big") for sk in sks]
    c = native.Context([0])
    c.keygen(b"".join(skb), cache_first=0, want_pubkeys=False)
    roots = _roots()
    sigs = c.sign(b"".join(skb), b"".join(roots))
    sets = [native.SetSpec(roots[i], sigs[96 * i:96 * i + 96], pk_indices=[i]) for i in range(N)]
    yield {"ctx": c, "sks": sks, "roots": roots, "sets": sets, "h192": [blscpu.hash_to_g2(m) for m in roots]}
    c.close()


def _pairing(f576):
    """final_exp of a device Miller value on the host (tests/native/hostsim.cpp)"""
    from tests import hostsim as hs
    out = hs.buf(576)
    hs.lib().hs_final_exp(out, f576)
    return out.raw


def _check_prepare(world, path, n):
    from oracle import bls12381 as o  # checker only
    from tests.randomizer_edges import glv_scalar, seed_for
    from tests.test_pairing_golden import f12_from_bytes
    res_by_word = []
    for k, slot in zip(WORDS, SLOTS):
        slot %= n
        res = world["ctx"].debug_prepare(world["sets"][:n], path, seed=seed_for(k, slot))
        assert len(res) == n
        assert all((ss, ps) == (0, 0) for _, _, ss, ps in res), hex(k)
        assert [h for h, _, _, _ in res] == world["h192"][:n], hex(k)
        hm = o.hash_to_g2(world["roots"][slot])
        assert res[slot][0] == o.g2_serialize(hm), (hex(k), slot)
        want = o.f12_pow(o.pairing(o.G1, hm), glv_scalar(k) * world["sks"][slot] % o.R)
        assert o.final_exp(f12_from_bytes(res[slot][1])) == want, (hex(k), slot)
        res_by_word.append(res)
    return res_by_word


@pytest.mark.gpu
def test_bulk_prepare_values(world):
    from lodestar_amd import native
    from oracle import bls12381 as o  # checker only
    _check_prepare(world, native.PATH_BULK, N)
    for i in range(0, N, 13):
        assert world["h192"][i] == o.g2_serialize(o.hash_to_g2(world["roots"][i])), i


@pytest.mark.gpu
def test_latency_call_unchanged(world):
    from lodestar_amd import native
    from tests.randomizer_edges import seed_for
    lat = _check_prepare(world, native.PATH_LATENCY, 64)
    k, slot = WORDS[0], SLOTS[0]
    bulk = world["ctx"].debug_prepare(world["sets"][:64], native.PATH_BULK, seed=seed_for(k, slot))
    for i, (b, l) in enumerate(zip(bulk, lat[0])):
        assert (b[0], b[2], b[3]) == (l[0], l[2], l[3]), i
        # the latency path's G2 chains run in projective coordinates: f is another representative
        assert _pairing(b[1]) == _pairing(l[1]), i


if __name__ == "__main__":
    _child()
