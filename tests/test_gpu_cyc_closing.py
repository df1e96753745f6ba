"""The closing kernels' final exponentiation with cyclotomic squarings and one inversion per block
(k_final12: five 12-lane teams per block), end to end.  Every case runs in a child process whose
BGV_LATENCY_MAX=0 sends also a small call down the bulk path, so that it closes on k_final12 and
not on the fold, and compares every job's code in worker mode with the same job verified alone
(MODE_PER_JOB) and with the constructed truth.

distinct   1,100 batchable one-set jobs with distinct roots: 18 groups, i.e. three full blocks of
           five teams and a block of three, the last group short (12 slots).  Invalid: a wrong key at
           slot 0 of group 0, a wrong message at the last slot of the last group, two wrong keys in
           one group, an undecodable signature.  First pass, the pattern round with its complement
           bits over gu1, the pairs round, and padded teams inside the batched inversion.
small1 / small0   40 jobs, one live team and four idle ones in the block; one invalid job / none.
shared     the same 1,100 jobs with one root per 64 consecutive jobs (18 uniform groups, the last of
           12), a wrong key inside one of them (the weighted test finds it: k_final_wident over the
           new gu) and two inside another (pattern tests over the pubkey-sum pairs gpkp).
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N = 1100
# case -> (jobs, jobs per root, wrong keys, wrong messages, undecodable signatures)
CASES = {
    "distinct": (N, 1, (0, 64 * 7 + 3, 64 * 7 + 40), (N - 1,), (64 * 11 + 9,)),
    "small1": (40, 1, (17,), (), ()),
    "small0": (40, 1, (), (), ()),
    "shared": (N, 64, (64 * 2 + 31, 64 * 9, 64 * 9 + 63), (), ()),
}


def _child(case):
    sys.path.insert(0, ROOT)
    from lodestar_amd import native
    n, per_root, wrong_key, wrong_msg, undecodable = CASES[case]
    sks = [(int.from_bytes(hashlib.sha256(b"cyc-closing-%d" % i).digest(), "little") % R).to_bytes(32, "big")
           for i in range(n)]
    ctx = native.Context([0])
    ctx.keygen(b"".join(sks), cache_first=0, want_pubkeys=False)
    keys = [(7 * i) % n for i in range(n)]
    roots = [hashlib.sha256(b"cyc-closing-root-%d" % (i // per_root)).digest() for i in range(n)]
    sigs = ctx.sign(b"".join(sks[k] for k in keys), b"".join(roots))
    sigs = [sigs[96 * i:96 * i + 96] for i in range(n)]
    named = list(keys)
    for i in wrong_key:
        named[i] = (keys[i] + 1) % n  # signed by keys[i]
    for i in wrong_msg:
        roots[i] = hashlib.sha256(b"wrong" + roots[i]).digest()
    for i in undecodable:
        sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]  # the compression flag cleared
    jobs = [([native.SetSpec(roots[i], sigs[i], pk_indices=[named[i]])], True) for i in range(n)]
    st = native.BgvStats()
    worker = ctx.verify_jobs(jobs, native.MODE_WORKER, st)
    alone = ctx.verify_jobs(jobs, native.MODE_PER_JOB)
    ctx.close()
    print(json.dumps({"worker": worker, "alone": alone, "retries": st.batch_retries,
                      "bad_encoding": -native.BLST_BAD_ENCODING}))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_closing_on_final12(case):
    env = dict(os.environ, BGV_LATENCY_MAX="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    n, _, wrong_key, wrong_msg, undecodable = CASES[case]
    want = [1] * n
    for i in wrong_key + wrong_msg:
        want[i] = 0
    for i in undecodable:
        want[i] = res["bad_encoding"]
    assert res["worker"] == res["alone"]
    assert res["alone"] == want
    assert res["worker"] == want
    failing_groups = {i // 64 for i in wrong_key + wrong_msg}
    assert res["retries"] >= (1 if failing_groups else 0)
    if not failing_groups:
        assert res["retries"] == 0


if __name__ == "__main__":
    _child(sys.argv[1])
