"""Builds and runs tests/native/devscopesim.cpp, the CPU simulation of the one-shot calls'
device-memory owner (bgv_devscope.h) over a recording policy.  Test infrastructure only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "devscopesim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {
    "O2": ["-O2"],
    "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
BGV_E_DEVICE = 30  # include/blsgpu.h
NALLOC = 7  # the scripted call's allocations (bgv_aggregate_signatures')
NOPS = 7    # and its enqueued operations; operation NOPS is the explicit synchronize


def build(kind="O2"):
    out = os.path.join(HERE, "native", "devscopesim_" + kind)
    deps = [SRC, os.path.join(CSRC, "bgv_devscope.h"), os.path.join(CSRC, "..", "..", "include", "blsgpu.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(lines, kind="O2"):
    """lines: protocol lines -> [(rc, [events])], one per line."""
    p = subprocess.run([build(kind)], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0, "devscopesim (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        head, _, log = line.partition("|")
        out.append((int(head.split()[1]), log.split()))
    assert len(out) == len(lines)
    return out
