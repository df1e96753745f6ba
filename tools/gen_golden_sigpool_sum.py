"""Generates tests/golden/sigpool_sum.json: the expected bytes of bgv_sigpool_sum over many entries
(tests/test_gpu_sigpool_bits.py), computed by the oracle alone.

Signature k is interop secret key k over root(k), as in tools/gen_golden_sig_aggregate.py (the
same deterministic signatures; the test compares the digest of bgv_sign's output over the first n
with `sigs_sha256`).  Each recorded aggregate is oracle.bls12381.signatures_aggregate of the run
[0, count): 63 and 64 (groups of 63 and 64 one-signature entries) and 324 (the six "sizes" entries
of 1, 2, 63, 64, 65 and 129 signatures together).

    python tools/gen_golden_sigpool_sum.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bls12381 as o  # noqa: E402

from tools.gen_golden_sig_aggregate import SIZES, root  # noqa: E402

COUNTS = [63, 64, sum(SIZES)]


def main():
    n = max(COUNTS)
    sigs = [o.g2_compress(o.sign(o.interop_secret_key(k), root(k))) for k in range(n)]
    out = {"n": n, "sigs_sha256": hashlib.sha256(b"".join(sigs)).hexdigest(), "runs": {}}
    for count in COUNTS:
        code, b = o.signatures_aggregate(sigs[:count])
        assert code == 0
        out["runs"]["%d" % count] = b.hex()
    with open(os.path.join(ROOT, "tests", "golden", "sigpool_sum.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
