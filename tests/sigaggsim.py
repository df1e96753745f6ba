"""Builds and runs tests/native/sigaggsim.cpp, the CPU driver of bgv_verify_aggregate's host plan
(bgv_sigagg_plan.h), and holds the Python model the plan is checked against.
Test infrastructure only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sigaggsim.cpp")
PLAN = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc", "bgv_sigagg_plan.h")
INCLUDE = os.path.join(os.path.dirname(HERE), "include", "blsgpu.h")
BUILDS = {
    "O2": ["-O2"],
    "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
NO_AGG = 0xFFFFFFFF
E_ARG = 23
FORM_NONE, FORM_WAVE, FORM_BULK = 0, 1, 2


def build(kind="O2"):
    out = os.path.join(HERE, "native", "sigaggsim_" + kind)
    deps = [SRC, PLAN, INCLUDE]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def consts(kind="O2"):
    """(BGV_NO_AGG, BGV_SIGAGG_WAVE_MAX, the largest naggs) as the headers define them."""
    return tuple(int(v) for v in subprocess.check_output([build(kind), "consts"], text=True).split())


def run(cases, kind="O2"):
    """cases: [(jobs, tags, naggs, wave_max)] with jobs = [(first_set, n_sets, code)].  Returns per
    case -E_ARG, or (form, first, count, member)."""
    text = ["%d" % len(cases)]
    for jobs, tags, naggs, wave_max in cases:
        text.append("%d %d %d %d" % (len(jobs), len(tags), naggs, wave_max))
        text += ["%d %d %d" % j for j in jobs]
        text.append(" ".join("%d" % t for t in tags))
    p = subprocess.run([build(kind)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "sigaggsim (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        parts = [[int(v) for v in f.split()] for f in line.split("|")]
        if parts[0][0] != 0:
            out.append(parts[0][0])
            continue
        (_, form, n), first, count, member = parts
        assert len(member) == n
        out.append((form, first, count, member))
    assert len(out) == len(cases)
    return out


def model(jobs, tags, naggs, wave_max):
    """The contract in include/blsgpu.h, written down directly: set i is accepted iff the code of a
    job that holds it is 1; aggregate a lists its accepted sets in set order."""
    if naggs > 1 << 20 or (naggs and any(t != NO_AGG and t >= naggs for t in tags)):
        return -E_ARG
    accepted = set()
    for first, n, code in jobs:
        if code == 1:
            accepted.update(range(first, first + n))
    groups = [[i for i in sorted(accepted) if tags[i] == a] for a in range(naggs)] if naggs else []
    member = [i for g in groups for i in g]
    first, at = [], 0
    for g in groups:
        first.append(at)
        at += len(g)
    form = FORM_NONE if not member else FORM_WAVE if len(member) <= wave_max else FORM_BULK
    return form, first, [len(g) for g in groups], member
