"""Builds and runs tests/native/sigpoolsim.cpp, the CPU driver of bgv_verify_accumulate's host plan
(bgv_sigpool_plan.h), and holds the Python model the tag check and the plan are checked against.
Test infrastructure only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sigpoolsim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bgv_sigpool_plan.h"), os.path.join(CSRC, "bgv_sigagg_plan.h"),
        os.path.join(os.path.dirname(HERE), "include", "blsgpu.h")]
BUILDS = {
    "O2": ["-O2"],
    "san": ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
NO_AGG = 0xFFFFFFFF
E_BAD_INDEX, E_ARG = 22, 23
FORM_NONE, FORM_WAVE, FORM_BULK = 0, 1, 2


def build(kind="O2"):
    out = os.path.join(HERE, "native", "sigpoolsim_" + kind)
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def consts(kind="O2"):
    """(BGV_NO_AGG, BGV_SIGAGG_WAVE_MAX, BGV_MAX_SIGPOOL) as the headers define them."""
    return tuple(int(v) for v in subprocess.check_output([build(kind), "consts"], text=True).split())


def run(cases, kind="O2"):
    """cases: [(jobs, tags, live, changed, wave_max)] with jobs = [(first_set, n_sets, code)], live =
    {id: generation} at submit and changed = {id: (live, generation)} before the step.  Returns per
    case -code, or (form, ids, first, count, member, gen_of_set)."""
    text = ["%d" % len(cases)]
    for jobs, tags, live, changed, wave_max in cases:
        text.append("%d %d %d %d %d" % (len(jobs), len(tags), len(live), len(changed), wave_max))
        text += ["%d %d %d" % j for j in jobs]
        text.append(" ".join("%d" % t for t in tags))
        text += ["%d %d" % kv for kv in live.items()]
        text += ["%d %d %d" % (i, lv, g) for i, (lv, g) in changed.items()]
    p = subprocess.run([build(kind)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "sigpoolsim (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        parts = [[int(v) for v in f.split()] for f in line.split("|")]
        if parts[0][0] != 0:
            out.append(parts[0][0])
            continue
        (_, form, n), ids, first, count, member, gens = parts
        assert len(member) == n
        out.append((form, ids, first, count, member, gens))
    assert len(out) == len(cases)
    return out


def model(jobs, tags, live, changed, wave_max, max_pool=16384):
    """The contract in include/blsgpu.h, written down directly.  Submit: any tag that is neither
    NO_AGG nor below BGV_MAX_SIGPOOL is -E_ARG, otherwise any tag on an id that is not live is
    -E_BAD_INDEX.  Step: set i is added iff the code of a job that holds it is 1, it is tagged and
    its entry is still live in the generation seen at submit; the touched entries ascend by id and
    list their sets in set order."""
    if any(t != NO_AGG and t >= max_pool for t in tags):
        return -E_ARG
    if any(t != NO_AGG and t not in live for t in tags):
        return -E_BAD_INDEX
    gens = [0 if t == NO_AGG else live[t] for t in tags]
    now = {i: (1, g) for i, g in live.items()}
    now.update(changed)
    accepted = set()
    for first, n, code in jobs:
        if code == 1:
            accepted.update(range(first, first + n))
    by_id = {}
    for i in sorted(accepted):
        t = tags[i]
        if t != NO_AGG and now[t] == (1, gens[i]):
            by_id.setdefault(t, []).append(i)
    ids = sorted(by_id)
    member = [i for e in ids for i in by_id[e]]
    first, at = [], 0
    for e in ids:
        first.append(at)
        at += len(by_id[e])
    form = FORM_NONE if not member else FORM_WAVE if len(member) <= wave_max else FORM_BULK
    return form, ids, first, [len(by_id[e]) for e in ids], member, gens
