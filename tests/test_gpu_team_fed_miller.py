"""The fed team Miller loop on the device (k_lines_team -> k_miller_team_fed): the signature pairs
of a retry round after a bulk first pass without uniform groups read line records a k_lines_team
lane walked for them instead of walking their own twist point.  Verdicts must not move.

Each case runs in a fresh child process (the knobs are read once per process) with
BGV_LATENCY_MAX=0, which sends small calls down the bulk path, and BGV_RETRY_WIDE_MAX=0, which
keeps small retry rounds off k_miller_wide: bgv_launch_gpairs then feeds every such round's teams.

  * retry: 130 batchable one-set jobs of distinct roots and keys (groups of 64, 64 and 2).  Wrong
    keys at jobs 0 and 63 (the ends of a group), at 70 and 100 (two in one group) and at 129 (the
    two-slot group), one committed undecodable signature.  Worker codes equal per-job codes and
    the constructed truth, and the batch went through retry rounds.
  * full round: one call of exactly (compute units x 256) one-set jobs, i.e. one full k_facc
    round of one wave per SIMD, the geometry at which a first pass's group pairs open a second
    round.  (The first pass keeps its route: fed teams measured slower there)
    Three wrong keys in three groups; every code is the truth; the retry rounds over the three
    groups are fed.

Uniform rounds (and so bgv_debug_uniform's values) keep the walking teams and are covered by
tests/test_gpu_r06.py and tests/test_gpu_debug_hooks.py; the fed value against miller_loop1's is
compared on the host, tests/test_team_fed_miller.py.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KNOBS = {"BGV_LATENCY_MAX": "0", "BGV_RETRY_WIDE_MAX": "0"}

N_RETRY = 130
RETRY_WRONG = (0, 63, 70, 100, 129)
RETRY_OFF_CURVE = 20


def _world(native, tag, n):
    """n cached keys, n distinct roots, job i signed by key i."""
    sks = [(int.from_bytes(hashlib.sha256(b"%s-%d" % (tag, i)).digest(), "little") % R).to_bytes(32, "big")
           for i in range(n)]
    ctx = native.Context([0])
    ctx.keygen(b"".join(sks), cache_first=0, want_pubkeys=False)
    roots = [hashlib.sha256(b"%s-root-%d" % (tag, i)).digest() for i in range(n)]
    sigs = ctx.sign(b"".join(sks), b"".join(roots))
    return ctx, roots, [sigs[96 * i:96 * i + 96] for i in range(n)]


def _child_retry():
    sys.path.insert(0, ROOT)
    from lodestar_amd import native
    ctx, roots, sigs = _world(native, b"fed-retry", N_RETRY)
    gold = {j["name"]: j for j in json.load(open(os.path.join(ROOT, "tests", "golden", "verdicts.json")))["jobs"]}
    sigs[RETRY_OFF_CURVE] = bytes.fromhex(gold["off_curve"]["sets"][0]["sig"])
    named = list(range(N_RETRY))
    for i in RETRY_WRONG:
        named[i] = (i + 1) % N_RETRY  # signed by key i
    jobs = [([native.SetSpec(roots[i], sigs[i], pk_indices=[named[i]])], True) for i in range(N_RETRY)]
    st = native.BgvStats()
    worker = ctx.verify_jobs(jobs, native.MODE_WORKER, st)
    alone = ctx.verify_jobs(jobs, native.MODE_PER_JOB)
    ctx.close()
    print(json.dumps({"worker": worker, "alone": alone, "retries": st.batch_retries}))


def _child_first_pass():
    sys.path.insert(0, ROOT)
    import torch
    from lodestar_amd import native
    n = torch.cuda.get_device_properties(0).multi_processor_count * 256
    wrong = (1, n // 2 + 7, n - 1)
    ctx, roots, sigs = _world(native, b"fed-first", n)
    named = list(range(n))
    for i in wrong:
        named[i] = (i + 1) % n
    jobs = [([native.SetSpec(roots[i], sigs[i], pk_indices=[named[i]])], True) for i in range(n)]
    st = native.BgvStats()
    worker = ctx.verify_jobs(jobs, native.MODE_WORKER, st)
    ctx.close()
    bad = [i for i in range(n) if worker[i] != (0 if i in wrong else 1)]
    print(json.dumps({"n": n, "wrong": wrong, "bad": bad[:20], "nbad": len(bad), "retries": st.batch_retries}))


def _run_child(which):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), which], cwd=ROOT, env=dict(os.environ, **KNOBS),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_retry_rounds_feed_their_teams():
    res = _run_child("retry")
    want = [0 if i in RETRY_WRONG else 1 for i in range(N_RETRY)]
    want[RETRY_OFF_CURVE] = -2
    assert res["alone"] == want
    assert res["worker"] == res["alone"]
    assert res["worker"] == want
    assert res["retries"] >= 1


@pytest.mark.gpu
def test_full_round_call_with_fed_retry_rounds():
    res = _run_child("first_pass")
    assert res["n"] % 256 == 0 and res["n"] > 0
    assert res["nbad"] == 0, res
    assert res["retries"] >= 1


if __name__ == "__main__":
    {"retry": _child_retry, "first_pass": _child_first_pass}[sys.argv[1]]()
