"""The bulk k_prep (signed-window r * sig and r * pk) on the device at its smallest size: 130
one-set jobs of distinct roots -- two full 64-lane groups and a short one -- in a child process
whose BGV_LATENCY_MAX=0 sends even this call down the bulk path.  Every job's code in worker mode
(batched, randomized) equals the same job verified on its own (MODE_PER_JOB)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 130
WRONG_KEY, WRONG_MSG, OFF_CURVE, NOT_IN_G2, INF_SIG = 5, 70, 20, 100, 129


def _child():
    sys.path.insert(0, ROOT)
    from lodestar_amd import native
    R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    sks = [(int.from_bytes(hashlib.sha256(b"prep-bulk-%d" % i).digest(), "little") % R).to_bytes(32, "big")
           for i in range(N)]
    ctx = native.Context([0])
    ctx.keygen(b"".join(sks), cache_first=0, want_pubkeys=False)
    roots = [hashlib.sha256(b"prep-bulk-root-%d" % i).digest() for i in range(N)]
    sigs = ctx.sign(b"".join(sks), b"".join(roots))
    sigs = [sigs[96 * i:96 * i + 96] for i in range(N)]
    gold = {j["name"]: j for j in json.load(open(os.path.join(ROOT, "tests", "golden", "verdicts.json")))["jobs"]}
    keys = list(range(N))
    keys[WRONG_KEY] = WRONG_KEY + 1
    roots[WRONG_MSG] = hashlib.sha256(b"another root").digest()
    sigs[OFF_CURVE] = bytes.fromhex(gold["off_curve"]["sets"][0]["sig"])
    sigs[NOT_IN_G2] = bytes.fromhex(gold["not_in_g2"]["sets"][0]["sig"])
    sigs[INF_SIG] = bytes([0xC0]) + bytes(95)
    jobs = [([native.SetSpec(roots[i], sigs[i], pk_indices=[keys[i]])], True) for i in range(N)]
    st = native.BgvStats()
    worker = ctx.verify_jobs(jobs, native.MODE_WORKER, st)
    alone = ctx.verify_jobs(jobs, native.MODE_PER_JOB)
    ctx.close()
    print(json.dumps({"worker": worker, "alone": alone, "retries": st.batch_retries}))


@pytest.mark.gpu
def test_bulk_prep_small_call_matches_per_job():
    env = dict(os.environ, BGV_LATENCY_MAX="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    want = [1] * N
    want[WRONG_KEY] = want[WRONG_MSG] = 0
    want[OFF_CURVE], want[NOT_IN_G2] = -2, -3
    want[INF_SIG] = res["alone"][INF_SIG]
    assert res["alone"] == want
    assert res["alone"][INF_SIG] != 1
    assert res["worker"] == res["alone"]
    assert res["retries"] > 0  # the batch failed as a whole and was taken apart


if __name__ == "__main__":
    _child()
