"""Golden fixture of the committee-bitfield sets (tests/golden/committee_bits.json).

    python tools/gen_golden_committee.py

A set may name its pubkeys as (committee, participation bitfield) instead of a list of validator
indices (include/blsgpu.h bgv_verify_bits).  The fixture pins, for committees of the sizes at
which the device code takes another path (word boundaries of the bitfield, the 16-lane team
against the whole wave, more terms than BGV_PK_TEAM_MAX) and the bit patterns on either side of
the direct / complement switch, the aggregate pubkey the oracle gives:

  keys[i]        compressed pubkey of sk_i = interop_secret_key(i), i < 520; keys[520] = -pk_0
                 (secret key r - sk_0), as tests/golden/keys.json's entry 128 is
  committees     name -> validator indices (the cache layout is index i = keys[i])
  cases[j]       committee (name), n, bits (hex, SSZ bit order: member k takes part iff
                 (bits[k >> 3] >> (k & 7)) & 1), k (bits set), agg (96-byte uncompressed
                 aggregate, 0x40 for infinity)

The aggregate is ONE scalar multiplication of G1 by the sum of the participants' secret keys
mod r, so the file is generated in a minute or two and never by the code under test.  Data only.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bls12381 as o  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "committee_bits.json")
NKEYS = 520
NEG0 = NKEYS  # index of -pk_0
SIZES = [1, 15, 16, 17, 31, 32, 33, 64, 65, 128, 257, 512, 513]


def secret_keys():
    sks = [o.interop_secret_key(i) for i in range(NKEYS)]
    return sks + [(o.R - sks[0]) % o.R]


def pack(positions, n):
    b = bytearray((n + 7) // 8)
    for p in positions:
        assert 0 <= p < n
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


def scattered(n, k, seed):
    """k distinct positions below n from a fixed linear congruential stream."""
    order, st = list(range(n)), seed
    for i in range(n - 1, 0, -1):
        st = (st * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        j = (st >> 33) % (i + 1)
        order[i], order[j] = order[j], order[i]
    return sorted(order[:k])


def patterns(n):
    half = (n + 1) // 2
    return [
        ("first", [0]),
        ("last", [n - 1]),
        ("all", list(range(n))),
        ("all_but_one", [p for p in range(n) if p != n // 2]),
        ("half", scattered(n, half, 1000 + n)),
        ("half_plus_one", scattered(n, min(n, half + 1), 2000 + n)),
        ("alternating", list(range(0, n, 2))),
    ]


def main():
    sks = secret_keys()
    keys = [o.g1_compress(o.sk_to_pk(sk)).hex() for sk in sks]
    committees, cases = {}, []

    def add_case(cname, pname, positions):
        members = committees[cname]
        n = len(members)
        bits = pack(positions, n)
        if not positions or any(c["committee"] == cname and c["bits"] == bits.hex() for c in cases):
            return  # an empty selection is an argument error, not an aggregate; no duplicates
        s = sum(sks[members[p]] for p in positions) % o.R
        cases.append({"name": "%s/%s" % (cname, pname), "committee": cname, "n": n, "bits": bits.hex(),
                      "k": len(positions), "agg": o.g1_serialize(o.g1_mul(o.G1, s)).hex()})

    for n in SIZES:
        cname = "n%d" % n
        committees[cname] = [(7 * i + 3 * n) % NKEYS for i in range(n)]  # 7 is a unit mod 520: distinct
        for pname, positions in patterns(n):
            add_case(cname, pname, positions)
    # pk_0 and -pk_0 among other members: both selected alone (infinity), both absent from a
    # majority (the complement side sums to infinity), both among a majority
    committees["cancel"] = [5, 0, 9, 11, NEG0, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71]
    add_case("cancel", "both_only", [1, 4])
    add_case("cancel", "both_absent", [p for p in range(20) if p not in (1, 4)])
    add_case("cancel", "both_in_majority", [p for p in range(20) if p not in (0, 7)])
    # committees whose total is infinity
    committees["inf_total2"] = [0, NEG0]
    add_case("inf_total2", "all", [0, 1])
    add_case("inf_total2", "first", [0])
    committees["inf_total4"] = [0, NEG0, 0, NEG0]
    add_case("inf_total4", "three", [0, 1, 2])  # complement mode over an infinity total
    add_case("inf_total4", "all", [0, 1, 2, 3])
    with open(OUT, "w") as f:
        json.dump({"keys": keys, "committees": committees, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d keys, %d committees, %d cases, %d bytes" %
          (OUT, len(keys), len(committees), len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
