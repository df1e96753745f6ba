"""Generates tests/golden/sig_aggregate.json: the expected aggregates of the larger cases of
tests/test_gpu_verify_aggregate.py, computed by the oracle alone.

Signature k is interop secret key k over root(k); BLS signatures are deterministic, so the device's
bgv_sign gives the same bytes (the test compares their digest with `sigs_sha256`).  Every case is a
list of aggregates, each a list of signature numbers; its expected bytes are
oracle.bls12381.signatures_aggregate of exactly those signatures (the Python oracle decodes and
subgroup-checks each one: ~0.1 s per signature, which is why the large cases are recorded here
and the small ones are computed in the test).

    python tools/gen_golden_sig_aggregate.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bls12381 as o  # noqa: E402

from lodestar_amd.native import SIGAGG_WAVE_MAX  # noqa: E402

SIZES = [1, 2, 63, 64, 65, 129]  # the strided loop and the tree of the sum
NROOTS = 3


def root(k):
    return hashlib.sha256(b"sig-aggregate root %d" % (k % NROOTS)).digest()


def runs(sizes):
    out, at = [], 0
    for n in sizes:
        out.append(list(range(at, at + n)))
        at += n
    return out


def cases(wave_max):
    return {
        "sizes": runs(SIZES),
        "wave_max": [list(range(wave_max))],
        "wave_max_plus_1": [list(range(wave_max + 1))],
    }


def main():
    cs = cases(SIGAGG_WAVE_MAX)
    n = 1 + max(k for c in cs.values() for a in c for k in a)
    sigs = [o.g2_compress(o.sign(o.interop_secret_key(k), root(k))) for k in range(n)]
    out = {"wave_max": SIGAGG_WAVE_MAX, "n": n, "nroots": NROOTS,
           "sigs_sha256": hashlib.sha256(b"".join(sigs)).hexdigest(), "cases": {}}
    for name, aggs in cs.items():
        want = []
        for a in aggs:
            code, b = o.signatures_aggregate([sigs[k] for k in a])
            assert code == 0
            want.append(b.hex())
        # every aggregate is a run of consecutive signatures: [first, count]
        out["cases"][name] = {"runs": [[a[0], len(a)] for a in aggs], "aggregates": want}
    with open(os.path.join(ROOT, "tests", "golden", "sig_aggregate.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
