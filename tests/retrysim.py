"""Builds and runs tests/native/retrysim.cpp, the CPU simulation of a call's layout and retry
rounds (bgv_host_layout.h, bgv_retry_plan.h), and makes its scenarios.  Test infrastructure only."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "retrysim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include", "blsgpu.h")
BUILDS = {
    "O2": ["-O2"],
    "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
# set kinds of a scenario (retrysim.cpp)
VALID, WRONG, UNDECODABLE, INF_SIG, INF_PK = range(5)
BLST_BAD_ENCODING, BLST_POINT_NOT_IN_GROUP, BLST_PK_IS_INFINITY = 1, 3, 6


def build(kind="O2"):
    out = os.path.join(HERE, "native", "retrysim_" + kind)
    deps = [SRC, INCLUDE] + [os.path.join(CSRC, f) for f in ("bgv_layout.h", "bgv_host_layout.h", "bgv_retry_plan.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(scenarios, kind="O2"):
    """The simulator's result records, one per scenario and in their order."""
    p = subprocess.run([build(kind)], input=json.dumps(scenarios), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "retrysim (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    out = [json.loads(line) for line in p.stdout.splitlines()]
    assert [o["name"] for o in out] == [s["name"] for s in scenarios]
    return out


def scenario(name, jobs, sets, mode=0, seed=1, uniform=False, layout=False):
    """jobs: (n_sets, batchable) each; sets: (root, kind, blst_code) each, in job order."""
    assert sum(n for n, _ in jobs) == len(sets)
    return {"name": name, "mode": mode, "seed": seed, "uniform": uniform, "layout": layout,
            "jobs": [[n, int(b)] for n, b in jobs], "sets": [list(s) for s in sets]}


def one_set_jobs(name, n, bad, **kw):
    """n batchable one-set jobs of distinct roots, the jobs in bad with a wrong signature."""
    bad = set(bad)
    return scenario(name, [(1, True)] * n, [(i, WRONG if i in bad else VALID, 0) for i in range(n)], **kw)


def truth(sc):
    """Per-job codes the reference gives (maybeBatch.ts + blst): the error of the first undecodable
    signature; else an infinity pubkey rejects (false for a one-set job, PK_IS_INFINITY for more);
    else 1 when every set verifies, 0 otherwise."""
    out, at = [], 0
    for n, _ in sc["jobs"]:
        sets = sc["sets"][at:at + n]
        at += n
        und = [s for s in sets if s[1] == UNDECODABLE]
        if und:
            out.append(-und[0][2])
        elif any(s[1] == INF_PK for s in sets):
            out.append(0 if n == 1 else -BLST_PK_IS_INFINITY)
        else:
            out.append(1 if all(s[1] == VALID for s in sets) else 0)
    return out


def plan_record(res):
    """What tests/golden/retry_plans.json keeps of a result: the groups of each round, and the
    rounds' record digests folded to 32 bits."""
    fold = 0
    for d in res["digest"]:
        v = int(d, 16)
        fold = ((fold * 0x01000193) ^ v ^ (v >> 32)) & 0xFFFFFFFF
    return "%s;%08x" % (",".join(str(g) for g in res["groups"]), fold)
