"""Both closings of a uniform batch's retry round, at the smallest call the layout makes uniform
(BGV_UNIFORM_MIN_JOBS = 1,024): 1,152 batchable one-set jobs over nine signing roots of 128
consecutive jobs each, i.e. eighteen uniform 64-slot groups, in a child process whose
BGV_LATENCY_MAX=0 sends the call down the bulk path.  Five jobs name a wrong key: one in each of
three groups (the weighted test finds it) and two in a fourth (a second invalid slot defeats the
weighted test, so the pattern tests run too).  Every job's code in worker mode equals the same job
verified on its own (MODE_PER_JOB) and the constructed truth.

The retry rounds hold a few tests each.  By default they close on k_final_fold; with
BGV_RETRY_FOLD_MAX=0 they close on k_final12, which then multiplies the tests' pubkey-sum pairs
(gpkp) -- the route production takes for any round above the threshold.  The test cannot see which
kernel ran: that the second environment lands on k_final12 is read off bgv_launch_groups, where
`pairs && b.uniform && b.ngroups <= 0` is false for a non-empty round.  Both knobs are read once
per process, hence the fresh child per case."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PER_ROOT = 1152, 128
WRONG = (5, 200, 700, 1030, 1050)  # groups 0, 3, 10 and twice group 16


def _child():
    sys.path.insert(0, ROOT)
    from lodestar_amd import native
    R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    sks = [(int.from_bytes(hashlib.sha256(b"uniform-retry-%d" % i).digest(), "little") % R).to_bytes(32, "big")
           for i in range(N)]
    ctx = native.Context([0])
    ctx.keygen(b"".join(sks), cache_first=0, want_pubkeys=False)
    keys = [(7 * i) % N for i in range(N)]
    roots = [hashlib.sha256(b"uniform-retry-root-%d" % (i // PER_ROOT)).digest() for i in range(N)]
    sigs = ctx.sign(b"".join(sks[k] for k in keys), b"".join(roots))
    named = list(keys)
    for i in WRONG:
        named[i] = (keys[i] + 1) % N  # signed by keys[i]
    jobs = [([native.SetSpec(roots[i], sigs[96 * i:96 * i + 96], pk_indices=[named[i]])], True) for i in range(N)]
    st = native.BgvStats()
    worker = ctx.verify_jobs(jobs, native.MODE_WORKER, st)
    alone = ctx.verify_jobs(jobs, native.MODE_PER_JOB)
    ctx.close()
    print(json.dumps({"worker": worker, "alone": alone, "retries": st.batch_retries}))


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"BGV_LATENCY_MAX": "0"}, {"BGV_LATENCY_MAX": "0", "BGV_RETRY_FOLD_MAX": "0"}],
                         ids=["fold", "final12"])
def test_uniform_retry_round_closings(knobs):
    env = dict(os.environ, **knobs)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    want = [0 if i in WRONG else 1 for i in range(N)]
    assert res["worker"] == res["alone"]
    assert res["alone"] == want
    assert res["worker"] == want
    assert res["retries"] >= 1  # failing groups were taken apart in retry rounds


if __name__ == "__main__":
    _child()
