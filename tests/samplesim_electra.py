"""Builds and runs tests/native/samplesim_electra.cpp, the CPU simulation of the device-side
balance-weighted sampling under Electra's rule (bgv_sample.h's 16-bit rule), and holds the model
the tests compare with: the consensus spec's compute_proposer_index and
get_next_sync_committee_indices as EIP-7251 left them, written out with hashlib over
tests/shufflesim.py's compute_shuffled_index.  The fixed seed, active lists, slot seeds and rounds
are tests/samplesim.py's.  Test infrastructure only."""
import hashlib
import os
import struct
import subprocess

from tests import samplesim as M
from tests import shufflesim as S

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "samplesim_electra.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = S.BUILDS

MAX_RANDOM_VALUE = 2 ** 16 - 1
MAX_TRIES = M.MAX_TRIES
SEED, ROUNDS = M.SEED, M.ROUNDS
active, slot_seeds = M.active, M.slot_seeds

# --- the fixed inputs of the CPU and GPU tests -------------------------------------------------
MAX_INCR = 2048  # MAX_EFFECTIVE_BALANCE_ELECTRA / EFFECTIVE_BALANCE_INCREMENT
TABLES = {
    "full": lambda v: 2048,
    "mixed": lambda v: 2048 if v % 3 else 32 + 300 * (v % 7),  # values on both sides of 255
    "min": lambda v: 32,  # the mainnet shape: acceptance about 1 / 64
    "high": lambda v: 256 * (1 + v % 8),  # low byte 0: a table cut to bytes accepts almost nothing
}


def table(name, n_eff):
    return [TABLES[name](v) for v in range(n_eff)]


def edge_seed(k):
    return hashlib.sha256(b"edge16" + k.to_bytes(4, "little")).digest()


EDGE_FFFF, EDGE_0000 = edge_seed(15322), edge_seed(52444)  # candidate 0 draws 0xFFFF / 0x0000


# --- the model -----------------------------------------------------------------------------------

def rand16(seed, i):
    """random_value of candidate i: 16 candidates per digest, two little-endian bytes each"""
    random_bytes = hashlib.sha256(seed + (i // 16).to_bytes(8, "little")).digest()
    offset = i % 16 * 2
    return int.from_bytes(random_bytes[offset:offset + 2], "little")


def accepted(eff, max_incr, value):
    return eff * MAX_RANDOM_VALUE >= max_incr * value


def candidates(seed, act, eff, max_incr, rounds):
    """(i, validator index, accepted) for i = 0, 1, 2, ...: the loop both spec functions share."""
    n = len(act)
    i = 0
    while True:
        v = act[S.compute_shuffled_index(i % n, n, seed, rounds)]
        yield i, v, accepted(eff[v], max_incr, rand16(seed, i))
        i += 1


def proposer(seed, act, eff, max_incr=MAX_INCR, rounds=ROUNDS):
    """compute_proposer_index, bounded as tests/samplesim.py bounds the byte rule's: (index or None
    after len(act) rejected candidates, candidates examined)."""
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


# The passes do not depend on the rule: samp_plan_pass is the byte rule's, unchanged.
model_passes = M.model_passes

# The passes of a mainnet-shaped sync committee (2^20 active indices, every balance 32 of 2048,
# 512 members, SEED) as the simulator ran them: the 512th acceptance is candidate number 33,301,
# which lies in the sixth window (candidates 31,744 .. 64,511), so 64,512 candidates are evaluated.
# (window, count, seeds in the pass); DESIGN.md quotes this.
MAINNET_SYNC_TRIES = 33302
MAINNET_SYNC_PASSES = [(1024 << k, 1024 << k, 1) for k in range(6)]
assert [(w, c) for w, c, _ in MAINNET_SYNC_PASSES] == model_passes(512, MAX_TRIES, MAINNET_SYNC_TRIES)


# --- the simulator ---------------------------------------------------------------------------------

def build(kind="O2"):
    out = os.path.join(HERE, "native", "samplesim_electra_" + kind)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(text, kind="O2"):
    p = subprocess.run([build(kind)], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "samplesim_electra (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def sim_sample(seeds, act, eff, want, proposers, max_incr=MAX_INCR, rounds=ROUNDS, kind="O2"):
    """One call of the simulator's pass loop -> {"passes": [(window, count, seeds in the pass)],
    "seeds": [(have, candidates examined, picks)], "us": its own time for the loop}.  The table
    goes over as four hex digits per validator index, little-endian as the device reads it."""
    text = "sample %d %d %d %d %d %d %d %s %s %s\n" % (
        len(seeds), want, 1 if proposers else 0, max_incr, rounds, len(act), len(eff),
        " ".join(s.hex() for s in seeds), " ".join(map(str, act)), struct.pack("<%dH" % len(eff), *eff).hex())
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
