"""Builds and runs tests/native/fedsim.cpp, the host emulation of the fed team Miller loop
(k_lines_team's scaled line records read by k_miller_team_fed).  Test infrastructure only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fedsim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {
    "O2": ["-O2"],
    # -O0 as tests/curvesim.py: the unrolled field arithmetic takes minutes to instrument at -O1 -g
    "san": ["-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


def build(kind="O2"):
    out = os.path.join(HERE, "native", "fedsim_" + kind)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def run(kind="O2"):
    """The simulator's own program -> (exit code, its "ok <check>" / "FAIL <check>" lines, stderr)."""
    p = subprocess.run([build(kind)], capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout.splitlines(), p.stderr
