"""Golden fixture of the span sets: one bitfield over several committees
(tests/golden/multi_committee.json).

    python tools/gen_golden_multi_committee.py

A set may lay ONE participation bitfield over a list of device-resident committees, concatenated
in list order (include/blsgpu.h bgv_pkspan; an attestation since EIP-7549).  The fixture uses the
521 keys and the committees of tests/golden/committee_bits.json (tools/gen_golden_committee.py) and
pins the aggregate pubkey of the expanded index list at the smallest shapes at which the walk
over the committees can go wrong:

  cases[j]   name, committees (names, in bitfield order; repeats allowed), n_bits (the sum of
             their lengths), bits (hex, SSZ bit order over the concatenation), k (bits set),
             terms (M: per committee the shorter side, plus one per complement committee),
             agg (96-byte uncompressed aggregate, 0x40 for infinity)

The aggregate is ONE scalar multiplication of G1 by the sum of the participants' secret keys mod
r (a repeated member counted again), never the code under test.  Data only.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bls12381 as o  # noqa: E402
from tools.gen_golden_committee import pack, scattered, secret_keys  # noqa: E402

BASE = os.path.join(ROOT, "tests", "golden", "committee_bits.json")
OUT = os.path.join(ROOT, "tests", "golden", "multi_committee.json")


def terms(n, k):
    """bgv_pk_bits.h: the complement side iff n - k + 1 < k; its total is one more term"""
    return n - k + 1 if n - k + 1 < k else k


def main():
    with open(BASE) as f:
        base = json.load(f)
    committees = base["committees"]
    sks = secret_keys()
    assert [o.g1_compress(o.sk_to_pk(sk)).hex() for sk in (sks[0], sks[-1])] == [base["keys"][0], base["keys"][-1]]
    cases = []

    def add(name, parts):
        """parts: [(committee name, selected positions in it)]"""
        positions, off, s, m = [], 0, 0, 0
        for cname, sel in parts:
            members = committees[cname]
            assert len(set(sel)) == len(sel) and all(0 <= p < len(members) for p in sel)
            positions += [off + p for p in sel]
            s += sum(sks[members[p]] for p in sel)
            m += terms(len(members), len(sel))
            off += len(members)
        cases.append({"name": name, "committees": [c for c, _ in parts], "n_bits": off,
                      "bits": pack(positions, off).hex(), "k": len(positions), "terms": m,
                      "agg": o.g1_serialize(o.g1_mul(o.G1, s % o.R)).hex()})

    def some(cname, k, seed):
        return scattered(len(committees[cname]), k, seed)

    def full(cname):
        return list(range(len(committees[cname])))

    # unaligned offsets (17, then 33), a one-member committee, a repeated id
    add("n17_n33", [("n17", some("n17", 9, 1)), ("n33", some("n33", 30, 2))])
    add("n1_n31_n1_n65", [("n1", [0]), ("n31", some("n31", 12, 3)), ("n1", [0]), ("n65", some("n65", 60, 4))])
    # direct, complement, empty and full committees in one set
    add("sides", [("n64", some("n64", 10, 5)), ("n128", some("n128", 120, 6)), ("n32", []), ("n33", full("n33")),
                  ("n1", [0]), ("n16", some("n16", 8, 7))])
    # 64 committees, most members present; every eighth committee empty
    ring = ["n1", "n15", "n16", "n17", "n31", "n32", "n33", "n64"]
    add("sixty_four", [(ring[c % 8], [] if c % 8 == 5 and c > 8 else
                        some(ring[c % 8], max(1, len(committees[ring[c % 8]]) * 9 // 10), 100 + c)) for c in range(64)])
    # M on both sides of the team (16 lanes), latency-path (49) and wave (256) switches
    add("m16", [("n31", some("n31", 8, 8)), ("n33", some("n33", 8, 9))])
    add("m17", [("n31", some("n31", 8, 10)), ("n33", some("n33", 9, 11))])
    add("m48", [("n64", some("n64", 24, 12)), ("n65", some("n65", 24, 13))])
    add("m49", [("n64", some("n64", 24, 14)), ("n65", some("n65", 23, 15)), ("n17", some("n17", 16, 16))])
    add("m256", [("n257", some("n257", 128, 17)), ("n513", some("n513", 128, 18))])
    add("m257", [("n257", some("n257", 128, 19)), ("n513", some("n513", 127, 20)), ("n15", some("n15", 15, 21)),
                 ("n16", some("n16", 16, 22))])
    # the only set bits sit in the bitfield's last word
    add("last_word", [("n33", []), ("n65", [63, 64])])
    # an infinity total on the complement side, alone and beside others
    add("inf_total2_complement", [("n17", some("n17", 5, 23)), ("inf_total2", [0, 1])])
    add("inf_total4_complement", [("inf_total4", [0, 1, 2]), ("n15", some("n15", 14, 24))])
    # pk_0 in one committee, -pk_0 in the next: the result is infinity
    add("cancel_across", [("cancel", [1]), ("inf_total2", [1])])
    add("cancel_totals", [("inf_total2", [0, 1]), ("inf_total4", [0, 1, 2, 3])])
    for c, want in (("m16", 16), ("m17", 17), ("m48", 48), ("m49", 49), ("m256", 256), ("m257", 257)):
        assert next(x for x in cases if x["name"] == c)["terms"] == want, c
    assert cases[-1]["agg"] == cases[-2]["agg"] == "40" + "00" * 95
    with open(OUT, "w") as f:
        json.dump({"base": "committee_bits.json", "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
