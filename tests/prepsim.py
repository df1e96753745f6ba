"""Builds tests/native/prepsim.cpp, the host build of what the bulk k_prep's task_sig and task_hash
run per set (mixed additions for the affine signature, the hash with one isogeny): a shared
library for ctypes and a stand-alone ASan + UBSan program.  Test infrastructure only."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "prepsim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
# the bulk unit's Fp2 products (bls_wide.h), every lazy bound checked at run time
LIB_FLAGS = ["-O2", "-DBGV_LZ2_WIDE", "-DBGV_LAZY_CHECK", "-shared", "-fPIC"]
# -O0 and no debug info: the force-inlined point formulas take many minutes to optimize under the sanitizers
SAN_FLAGS = ["-O0", "-DBGV_LZ2_WIDE", "-DBGV_LAZY_CHECK", "-DPREPSIM_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
FORM_JAC, FORM_AFF, FORM_INF = 0, 1, 2


def _build(out, flags):
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-o", out + ".tmp", SRC] + flags)
    os.replace(out + ".tmp", out)
    return out


def build_lib():
    return _build(os.path.join(HERE, "native", "libprepsim.so"), LIB_FLAGS)


def build_san():
    return _build(os.path.join(HERE, "native", "prepsim_san"), SAN_FLAGS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_lib())
    return _lib
