"""Builds and runs tests/native/multicomsim.cpp, the CPU simulation of the span sets (one bitfield
over several committees: bgv_pk_bits.h run and walk, bgv_host_layout.h checks and layout), and
loads their golden fixture.  Test infrastructure only."""
import json
import os
import subprocess

from tests import committeesim as cs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "multicomsim.cpp")
GOLDEN = os.path.join(HERE, "golden", "multi_committee.json")
BUILDS = {
    "O2": ["-O2"],
    # the layout driver alone (no G1 arithmetic: its headers take minutes to compile under the sanitizers)
    "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMULTICOMSIM_LAYOUT_ONLY"],
}
PK_SPAN = 32  # bgv_layout.h BGV_SLOT_PK_SPAN
SPAN_HEAD = 3  # bgv_pk_bits.h PKB_SPAN_HEAD: records, complement committees, terms
MAX_SET_COMMITTEES, MAX_SPAN_BITS = 64, 131072  # blsgpu.h

_fixture = None


def fixture():
    """multi_committee.json over the keys and committees of committee_bits.json"""
    global _fixture
    if _fixture is None:
        with open(GOLDEN) as f:
            _fixture = json.load(f)
        base = cs.fixture()
        _fixture["keys"], _fixture["committees"] = base["keys"], base["committees"]
    return _fixture


def expand(case, committees=None):
    """The index list the span stands for (get_attesting_indices' order; repeats kept)."""
    committees = committees or fixture()["committees"]
    bits, out, off = bytes.fromhex(case["bits"]), [], 0
    for name in case["committees"]:
        members = committees[name]
        out += [m for p, m in enumerate(members) if (bits[(off + p) >> 3] >> ((off + p) & 7)) & 1]
        off += len(members)
    assert off == case["n_bits"]
    return out


def build(kind="O2"):
    out = os.path.join(HERE, "native", "multicomsim_" + kind)
    deps = [SRC, cs.INCLUDE] + [os.path.join(cs.CSRC, f) for f in os.listdir(cs.CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-o", out + ".tmp", SRC]
                          + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(mode, text, kind="O2"):
    p = subprocess.run([build(kind), mode], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "multicomsim %s (%s) exit %d: %s" % (mode, kind, p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()
