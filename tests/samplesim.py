"""Builds and runs tests/native/samplesim.cpp, the CPU simulation of the device-side
balance-weighted sampling (bgv_sample.h), and holds the model the tests compare with: the consensus
spec's compute_proposer_index and get_next_sync_committee_indices written out with hashlib over
tests/shufflesim.py's compute_shuffled_index.  Test infrastructure only."""
import hashlib
import os
import subprocess

from tests import shufflesim as S

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "samplesim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = S.BUILDS

NO_PROPOSER = 0xFFFFFFFF
MAX_TRIES = 65536
BLOCK = 256
PASS_ITEMS = 1 << 22

# --- the fixed inputs of the CPU and GPU tests -------------------------------------------------
SEED = hashlib.sha256(b"lodestar-amd gpu sampling").digest()
ROUNDS = 90
MAX_INCR = 32
TABLES = {
    "full": lambda v: 32,
    "mixed": lambda v: 32 if v % 3 else 1 + v % 7,
    "low": lambda v: 1 + v % 4,
    "one": lambda v: 1,
}


def slot_seeds(seed=SEED, slots=32):
    return [hashlib.sha256(seed + s.to_bytes(8, "little")).digest() for s in range(slots)]


def active(n):
    return [i + i // 6 for i in range(n)]


def table(name, n_eff):
    return bytes(TABLES[name](v) for v in range(n_eff))


# --- the model -----------------------------------------------------------------------------------

def candidates(seed, act, eff, max_incr, rounds):
    """(i, validator index, accepted) for i = 0, 1, 2, ...: the loop both spec functions share."""
    n = len(act)
    i = 0
    while True:
        v = act[S.compute_shuffled_index(i % n, n, seed, rounds)]
        byte = hashlib.sha256(seed + (i // 32).to_bytes(8, "little")).digest()[i % 32]
        yield i, v, eff[v] * 255 >= max_incr * byte
        i += 1


def proposer(seed, act, eff, max_incr=MAX_INCR, rounds=ROUNDS):
    """compute_proposer_index as seed.ts:22-80 bounds it: (index or None after len(act) rejected
    candidates, candidates examined)."""
    for i, v, ok in candidates(seed, act, eff, max_incr, rounds):
        if ok:
            return v, i + 1
        if i + 1 == len(act):
            return None, i + 1


def sync_committee(seed, act, eff, size, max_incr=MAX_INCR, rounds=ROUNDS, cap=MAX_TRIES):
    """get_next_sync_committee_indices: (indices or None when the cap is hit, candidates examined)."""
    out = []
    for i, v, ok in candidates(seed, act, eff, max_incr, rounds):
        if i == cap:
            return None, i
        if ok:
            out.append(v)
            if len(out) == size:
                return out, i + 1


def model_passes(want, limit, tries, n_todo=1):
    """The (window, count) passes a seed that needs `tries` candidates goes through: the first
    window is max(256, 2 want) rounded up to 256, each further one twice the last, within
    PASS_ITEMS candidates over the pass's seeds and within the limit."""
    out, base, w = [], 0, -(-max(BLOCK, 2 * want) // BLOCK) * BLOCK
    while base < min(tries, limit):
        w = min(w, max(BLOCK, PASS_ITEMS // n_todo // BLOCK * BLOCK))
        count = min(w, limit - base)
        out.append((-(-count // BLOCK) * BLOCK, count))
        base += count
        w = 2 * out[-1][0]
    return out


# --- the simulator ---------------------------------------------------------------------------------

def build(kind="O2"):
    out = os.path.join(HERE, "native", "samplesim_" + kind)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(text, kind="O2"):
    p = subprocess.run([build(kind)], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "samplesim (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def sim_sample(seeds, act, eff, want, proposers, max_incr=MAX_INCR, rounds=ROUNDS, kind="O2"):
    """One call of the simulator's pass loop -> {"passes": [(window, count, seeds in the pass)],
    "seeds": [(have, candidates examined, picks)], "us": its own time for the loop}."""
    text = "sample %d %d %d %d %d %d %d %s %s %s\n" % (
        len(seeds), want, 1 if proposers else 0, max_incr, rounds, len(act), len(eff),
        " ".join(s.hex() for s in seeds), " ".join(map(str, act)), bytes(eff).hex())
    res = {"passes": [], "seeds": [], "us": None}
    for ln in run(text, kind):
        f = ln.split()
        if f[0] == "pass":
            res["passes"].append((int(f[1]), int(f[2]), int(f[3])))
        elif f[0] == "seed":
            res["seeds"].append((int(f[1]), int(f[2]), [int(x) for x in f[3:]]))
        elif f[0] == "us":
            res["us"] = int(f[1])
    assert len(res["seeds"]) == len(seeds)
    return res


def sim_plan(want, limit, n_todo, kind="O2"):
    """The passes samp_plan_pass gives a seed that never finishes: [(window, count)]."""
    return [tuple(int(x) for x in ln.split()[1:]) for ln in run("plan %d %d %d\n" % (want, limit, n_todo), kind)]
