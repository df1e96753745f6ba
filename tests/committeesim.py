"""Builds and runs tests/native/committeesim.cpp, the CPU simulation of the committee-bitfield
sets (bgv_pk_bits.h selection and mode, bgv_host_layout.h layout), and loads their golden fixture.
Test infrastructure only."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "committeesim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include", "blsgpu.h")
GOLDEN = os.path.join(HERE, "golden", "committee_bits.json")
BUILDS = {
    "O2": ["-O2"],
    # the layout driver alone (no G1 arithmetic: its headers take minutes to compile under the sanitizers)
    "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCOMMITTEESIM_LAYOUT_ONLY"],
}
# slot flags (bgv_layout.h) and codes (blsgpu.h)
PK_CACHED, PK_COMMITTEE, PK_COMPLEMENT = 2, 8, 16
E_EMPTY_AGGREGATE, E_BAD_INDEX, E_ARG = 20, 22, 23
PK_TEAM_MAX = 256

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with open(GOLDEN) as f:
            _fixture = json.load(f)
    return _fixture


def build(kind="O2"):
    out = os.path.join(HERE, "native", "committeesim_" + kind)
    deps = [SRC, INCLUDE] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-o", out + ".tmp", SRC]
                          + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(mode, text, kind="O2"):
    p = subprocess.run([build(kind), mode], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "committeesim %s (%s) exit %d: %s" % (mode, kind, p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


def words_of(bits: bytes, n: int):
    """The bitfield as the layout ships it: ceil(n / 32) little-endian 32-bit words."""
    padded = bits + bytes(-len(bits) % 4)
    return [int.from_bytes(padded[4 * w:4 * w + 4], "little") for w in range((n + 31) // 32)]


def pack(positions, n):
    b = bytearray((n + 7) // 8)
    for p in positions:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)
