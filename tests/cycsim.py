"""Builds tests/native/cycsim.cpp, the host emulation of the closing kernels' final exponentiation
(cyclotomic squarings after an easy part with a batched inversion): as its own program under
AddressSanitizer + UBSan, and at -O2 as a shared library: cs_selftest runs the program's checks,
the other cs_* functions let the tests compare with the oracle.  Test infrastructure only."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "cycsim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
BUILDS = {
    # -O0 as tests/fedsim.py: the unrolled field arithmetic takes minutes to instrument at -O1 -g
    "san": ("cycsim_san", ["-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
    "lib": ("libcycsim.so", ["-O2", "-shared", "-fPIC"]),
}


def build(kind="san"):
    name, flags = BUILDS[kind]
    out = os.path.join(HERE, "native", name)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-o", out + ".tmp", SRC] + flags)
    os.replace(out + ".tmp", out)
    return out


def run(kind="san"):
    """The simulator's own program -> (exit code, its "ok <check>" / "FAIL <check>" lines, stderr)."""
    p = subprocess.run([build(kind)], capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout.splitlines(), p.stderr


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build("lib"))
    return _lib
