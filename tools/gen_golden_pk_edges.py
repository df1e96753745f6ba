"""Crafted G1 wire encodings (48-byte compressed keys, 96-byte records) for every pubkey-decoding
route of the device, with the oracle's answer for each: tests/golden/pk_edges.json (data only).

    python tools/gen_golden_pk_edges.py

Everything here comes from oracle/bls12381.py (g1_decompress, g1_deserialize, pubkey_validate,
core_verify, verify_signature_sets_maybe_batch, deposit_valid) and integer arithmetic; nothing
from the device code.  Secret keys and valid keys are those of tests/golden/keys.json.

An entry has `name`, `kind`, `pk48` and / or `pk96` (hex), and per wire form `expect48` /
`expect96` (0 or the BLST code of the decoding) with `infinity48` / `infinity96` where the bytes
are an infinity encoding.  `validate` is o.pubkey_validate(pk48), `deposit` o.deposit_valid(pk48,
root, sig).  Where a form decodes to a finite point, `x` / `y` hold it (both forms of an entry
decode to the same point) and `verdict` is o.core_verify(point, root, sig): what a one-set job
gives whose key is this point taken on trust (a cache entry or a 96-byte record).  `root` and
`sig` are the entry's own: the signature is by `key` (an index of keys.json) where the entry is
built on that key, else by key 0, which then has nothing to do with the point.

kinds
  flags      the eight values of the three flag bits over the bytes of a valid key, in both forms
  infinity   the infinity encodings, with the sort bit, with a stray bit at byte 1, 47 and 95
  field      x = p - 1, p, p + 1, 2^381 - 1; x = 0 with either sort bit and (0, +-2); y = p; x + p and
             y + p below 2^381 (the flag bits stay clear); x with x^3 + 4 a non-residue; a right
             x with another key's y; compressed bytes in the first 48 of a record, zero and junk tail
  flip       a valid key with the sort bit toggled / y -> p - y: decodes (code 0) to -pk, verdict 0
  limb       on-curve points whose x has an all-ones 28-bit limb (limbs 0, 6 and 12; the top limb
             of a value below p cannot be all ones) or a zero low limb, the first on-curve x
             upward from the pattern.  On the curve, not in G1: validate 3, verdict 0.
  valid      two plain valid keys: the positive control
  torsion    T_q = [h r / q^2] Q of exact order q, Q the curve point of x = 5, h the cofactor
             3 * 11^2 * 10177^2 * 859267^2 * 52437899^2 of E(Fp): each prime q, and 11 * 10177
  mixed      pk + T: on the curve, outside G1 (validate 3, deposit 0), yet e(pk + T, H) = e(pk, H)
             after the final exponentiation, so the signature of the underlying secret key
             verifies (verdict 1): one per order, one with a torsion part of composite order, pk -
             T_11 (whose torsion part cancels that of pk' + T_11) and the sort-flipped twin of one

`sets` are multi-record signature sets.  A record reference is k<j> (key j uncompressed), c<j>
(key j compressed in the first 48 bytes, zero tail), n<j> (-pk_j uncompressed), `inf` (0x40 and
zeros), `cinf` (0xC0 and zeros) or an entry's name (its pk96).  `expect` is the code of a one-set
job (1 / 0, or -code of the first record that does not decode; an infinity sum gives 0) and
`pair_expect` that of a non-batchable job of `pair_partner` (a valid one-record set) and this set
through o.verify_signature_sets_maybe_batch (an infinity sum raises BLST_PK_IS_INFINITY: -6).
`agg_keys` and an entry's `agg_sig`: for every mixed entry of verdict 1 the signature of its key
and the agg_keys together over its root, and `agg_verdict` the oracle's answer for the 16-key sum.
The table of names and codes is printed; the run takes a few minutes.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bls12381 as o  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "pk_edges.json")
P = o.P
H1 = 0x396C8C005555E1568C00AAAB0000AAAB  # the cofactor of E(Fp)
TORSION_PRIMES = (11, 10177, 859267, 52437899)
LIM = (1 << 381) - P  # a coordinate below this still fits under the flag bits with p added
LBITS, LMASK = 28, (1 << 28) - 1
AGG_KEYS = list(range(100, 115))
PAIR_SCALARS = [0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9]


def hx(v):
    return "%096x" % v


def be48(v, flags=0):
    assert 0 <= v < 1 << 384
    b = bytearray(v.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def with_flags(b, bits):
    return bytes([(b[0] & 0x1F) | (bits << 5)]) + bytes(b[1:])


def curve_y(x):
    return o.fp_sqrt((x * x * x + o.B1) % P)


def first_on_curve(x, step):
    while curve_y(x) is None:
        x += step
    return x


def torsion_points():
    assert H1 == 3 * 11**2 * 10177**2 * 859267**2 * 52437899**2
    q5 = (5, curve_y(5))
    assert q5[1] is not None and o.g1_on_curve(q5)
    out = {}
    for q in TORSION_PRIMES:
        t = o.g1_mul(q5, H1 * o.R // (q * q))
        assert t is not None and o.g1_on_curve(t) and o.g1_mul(t, q) is None and not o.g1_in_group(t)
        assert o.g1_mul(q5, H1 * o.R // q) is None  # the q-torsion is fully rational
        out[q] = t
    return out


_hash = o.hash_to_g2
_hashes = {}


def hash_once(msg, dst=o.DST_POP):
    if (msg, dst) not in _hashes:
        _hashes[(msg, dst)] = _hash(msg, dst)
    return _hashes[(msg, dst)]


def decode(fn, b):
    """(code, infinity, point) of one wire form."""
    try:
        pt = fn(b)
    except o.BlstError as err:
        return err.code, False, None
    return 0, pt is None, pt


class Corpus:
    def __init__(self, sks, pks):
        self.sks, self.pks, self.entries = sks, pks, []

    def add(self, name, kind, pk48=None, pk96=None, key=None, **extra):
        e = {"name": name, "kind": kind}
        root = hashlib.sha256(b"pk-edges:" + name.encode()).digest()
        sig_pt = o.g2_mul(hash_once(root), self.sks[key if key is not None else 0])
        sig = o.g2_compress(sig_pt)
        point = None
        for form, b, fn in (("48", pk48, o.g1_decompress), ("96", pk96, o.g1_deserialize)):
            if b is None:
                continue
            e["pk" + form] = bytes(b).hex()
            code, inf, pt = decode(fn, bytes(b))
            e["expect" + form] = code
            if inf:
                e["infinity" + form] = True
            if pt is not None:
                assert point is None or point == pt, name
                point = pt
        if pk48 is not None:
            e["validate"] = o.pubkey_validate(bytes(pk48))
            e["deposit"] = int(o.deposit_valid(bytes(pk48), root, sig))
        if point is not None:
            e["x"], e["y"] = hx(point[0]), hx(point[1])
            e["verdict"] = int(o.core_verify(point, root, sig_pt))
        e["root"], e["sig"] = root.hex(), sig.hex()
        if key is not None:
            e["key"] = key
        e.update(extra)
        self.entries.append(e)
        return e

    def both(self, name, kind, pt, key=None, **extra):
        return self.add(name, kind, o.g1_compress(pt), o.g1_serialize(pt), key, **extra)


def build_entries(c, torsion):
    sks, pks = c.sks, c.pks
    c48, u96 = o.g1_compress(pks[0]), o.g1_serialize(pks[0])

    # ---- flags --------------------------------------------------------------------------------
    for bits in range(8):
        c.add("flags48_%d%d%d" % (bits >> 2, bits >> 1 & 1, bits & 1), "flags", pk48=with_flags(c48, bits), key=0)
        c.add("flags96_%d%d%d" % (bits >> 2, bits >> 1 & 1, bits & 1), "flags", pk96=with_flags(u96, bits), key=0)

    # ---- infinity -----------------------------------------------------------------------------
    def stray(n, flag, at, v=1):
        b = bytearray([flag]) + bytearray(n - 1)
        b[at] |= v
        return bytes(b)

    c.add("infinity", "infinity", pk48=stray(48, 0xC0, 0, 0), pk96=stray(96, 0x40, 0, 0))
    c.add("infinity_sort_bit", "infinity", pk48=stray(48, 0xE0, 0, 0), pk96=stray(96, 0x60, 0, 0))
    c.add("infinity_stray_1", "infinity", pk48=stray(48, 0xC0, 1, 0x80), pk96=stray(96, 0x40, 1, 0x80))
    c.add("infinity_stray_47", "infinity", pk48=stray(48, 0xC0, 47), pk96=stray(96, 0x40, 47))
    c.add("infinity_stray_95", "infinity", pk96=stray(96, 0x40, 95))
    c.add("infinity_stray_flag_low", "infinity", pk48=stray(48, 0xC1, 0, 0), pk96=stray(96, 0x41, 0, 0))
    # a compressed infinity in a record: the decoding reads 48 bytes and never looks at the tail
    c.add("rec_compressed_infinity", "infinity", pk96=stray(96, 0xC0, 0, 0))
    c.add("rec_compressed_infinity_junk_tail", "infinity", pk96=stray(96, 0xC0, 95))
    c.add("rec_compressed_infinity_stray_47", "infinity", pk96=stray(96, 0xC0, 47))

    # ---- field edges --------------------------------------------------------------------------
    y_any = be48(pks[0][1])
    for name, x in (("p_minus_1", P - 1), ("p", P), ("p_plus_1", P + 1), ("all_ones_381", (1 << 381) - 1)):
        y = curve_y(x) if x < P else None
        c.add("x_" + name, "field", pk48=be48(x, 0x80), pk96=be48(x) + (be48(y) if y is not None else y_any))
    for sort in (0, 1):
        c.add("x0_sort%d" % sort, "field", pk48=be48(0, 0x80 | (0x20 if sort else 0)))
    c.add("x0_y2", "field", pk96=be48(0) + be48(2))
    c.add("x0_y_minus_2", "field", pk96=be48(0) + be48(P - 2))
    c.add("y_p", "field", pk96=be48(pks[0][0]) + be48(P))
    c.add("y_all_ones_384", "field", pk96=be48(pks[0][0]) + be48((1 << 384) - 1))
    jx = next(j for j in range(len(pks)) if pks[j][0] < LIM)
    jy = next(j for j in range(len(pks)) if min(pks[j][1], P - pks[j][1]) < LIM)
    py = pks[jy] if pks[jy][1] < LIM else o.g1_neg(pks[jy])
    sort = 0x20 if o.fp_lex_largest(pks[jx][1]) else 0
    assert (pks[jx][0] + P) >> 381 == 0 and (py[1] + P) >> 381 == 0
    c.add("noncanonical_x", "field", pk48=be48(pks[jx][0] + P, 0x80 | sort),
          pk96=be48(pks[jx][0] + P) + be48(pks[jx][1]), key=jx)
    c.add("noncanonical_y", "field", pk96=be48(py[0]) + be48(py[1] + P), key=jy)
    c.add("noncanonical_x_in_record_head", "field", pk96=be48(pks[jx][0] + P, 0x80 | sort) + bytes(48), key=jx)
    xn = 1
    while curve_y(xn) is not None:
        xn += 1
    c.add("x_nonresidue", "field", pk48=be48(xn, 0x80), pk96=be48(xn) + y_any)
    c.add("x_nonresidue_sort", "field", pk48=be48(xn, 0xA0))
    c.add("right_x_wrong_y", "field", pk96=be48(pks[1][0]) + be48(pks[2][1]), key=1)
    c.add("y_off_by_one", "field", pk96=be48(pks[1][0]) + be48(pks[1][1] ^ 1), key=1)
    c.add("rec_compressed_zero_tail", "field", pk96=o.g1_compress(pks[3]) + bytes(48), key=3)
    c.add("rec_compressed_junk_tail", "field", pk96=o.g1_compress(pks[4]) + bytes([0xAB]) * 48, key=4)
    c.add("rec_compressed_y_tail", "field", pk96=o.g1_compress(pks[4]) + be48(pks[4][1]), key=4)

    # ---- sort flips ---------------------------------------------------------------------------
    for j in (6, 7):
        e = c.both("flip_key%d" % j, "flip", o.g1_neg(pks[j]), key=j)
        assert e["pk48"] == with_flags(o.g1_compress(pks[j]), o.g1_compress(pks[j])[0] >> 5 ^ 1).hex()
        assert e["expect48"] == 0 and e["expect96"] == 0 and e["verdict"] == 0 and e["validate"] == 0

    # ---- limb patterns ------------------------------------------------------------------------
    base = pks[0][0]
    for limb in (0, 6, 12):
        x0 = base | (LMASK << (LBITS * limb))
        if limb == 0:
            x = first_on_curve(x0, 1 << LBITS)
        else:
            x = first_on_curve(x0 & ~LMASK, 1)
        assert x < P and (x >> (LBITS * limb)) & LMASK == LMASK
        c.both("limb_x_ones_%d" % limb, "limb", (x, curve_y(x)), limb=limb)
    x = first_on_curve(base & ~LMASK, 1 << LBITS)
    assert x < P and x & LMASK == 0
    c.both("limb_x_low_zero", "limb", (x, curve_y(x)), limb=0)

    # ---- valid --------------------------------------------------------------------------------
    for j in (8, 9):
        e = c.both("valid_key%d" % j, "valid", pks[j], key=j)
        assert e["verdict"] == 1 and e["deposit"] == 1 and e["validate"] == 0

    # ---- torsion and mixed order ----------------------------------------------------------------
    t_comp = o.g1_add(torsion[11], torsion[10177])
    assert o.g1_mul(t_comp, 11 * 10177) is None and o.g1_mul(t_comp, 11) is not None \
        and o.g1_mul(t_comp, 10177) is not None
    tors = [(q, torsion[q]) for q in TORSION_PRIMES] + [(11 * 10177, t_comp)]
    for q, t in tors:
        e = c.both("torsion_%d" % q, "torsion", t, order=q)
        assert e["validate"] == 3 and e["verdict"] == 0 and e["expect48"] == 0 and e["expect96"] == 0
    mixed = []
    for k, (q, t) in enumerate(tors):
        mixed.append(("mixed_%d" % q, o.g1_add(pks[10 + k], t), 10 + k, q))
    mixed.append(("mixed_11_minus", o.g1_add(pks[16], o.g1_neg(torsion[11])), 16, 11))
    for name, pt, key, q in mixed:
        assert o.g1_on_curve(pt) and not o.g1_in_group(pt)
        e = c.both(name, "mixed", pt, key=key, order=q)
        assert e["validate"] == 3 and e["verdict"] == 1 and e["deposit"] == 0, name
        # with the fifteen agg_keys: the 16-key sum and their joint signature
        sk = (sks[key] + sum(sks[j] for j in AGG_KEYS)) % o.R
        agg = pt
        for j in AGG_KEYS:
            agg = o.g1_add(agg, pks[j])
        root = bytes.fromhex(e["root"])
        s = o.g2_mul(hash_once(root), sk)
        e["agg_sig"] = o.g2_compress(s).hex()
        e["agg_verdict"] = int(o.core_verify(agg, root, s))
        assert e["agg_verdict"] == 1
    e = c.both("mixed_11_flip", "mixed", o.g1_neg(mixed[0][1]), key=10, order=11)
    assert e["validate"] == 3 and e["verdict"] == 0


def record(ref, c, by_name):
    if ref == "inf":
        return bytes([0x40]) + bytes(95)
    if ref == "cinf":
        return bytes([0xC0]) + bytes(95)
    if ref in by_name:
        return bytes.fromhex(by_name[ref]["pk96"])
    j = int(ref[1:])
    if ref[0] == "k":
        return o.g1_serialize(c.pks[j])
    if ref[0] == "n":
        return o.g1_serialize(o.g1_neg(c.pks[j]))
    assert ref[0] == "c"
    return o.g1_compress(c.pks[j]) + bytes(48)


def build_sets(c):
    by_name = {e["name"]: e for e in c.entries}
    k = lambda *js: ["k%d" % j for j in js]  # noqa: E731
    # (name, records, the keys whose secret keys sign, with multiplicity; [] signs with key 0)
    cases = [
        ("bad_first", ["x_p"] + k(20, 21), [20, 21]),
        ("bad_middle", k(20) + ["x_nonresidue"] + k(21), [20, 21]),
        ("bad_last", k(20, 21) + ["x0_y2"], [20, 21]),
        ("two_bad_codes", k(20) + ["right_x_wrong_y", "x_p"] + k(21), [20, 21]),
        ("two_bad_codes_reversed", k(20) + ["flags96_001", "y_off_by_one"] + k(21), [20, 21]),
        ("bad_after_infinity", ["inf", "noncanonical_y"] + k(20), [20]),
        ("infinity_among_valid", k(22) + ["inf"] + k(23), [22, 23]),
        ("compressed_infinity_among_valid", k(22) + ["cinf"] + k(23), [22, 23]),
        ("infinity_first", ["inf"] + k(22), [22]),
        ("all_infinity", ["inf", "inf", "cinf"], []),
        ("cancel", ["k24", "n24"], []),
        ("cancel_then_key", ["k24", "n24", "k25"], [25]),
        ("cancel_in_the_middle", ["k25", "k24", "n24"], [25]),
        ("twice", k(26, 26), [26, 26]),
        ("thrice", k(26, 26, 26), [26, 26, 26]),
        ("compressed_among_uncompressed", ["c27", "k28", "c29", "rec_compressed_junk_tail"], [27, 28, 29, 4]),
        ("records_17", k(*range(30, 47)), list(range(30, 47))),
        ("records_65", k(*range(47, 112)), list(range(47, 112))),
        ("all_mixed", ["mixed_11", "mixed_10177", "mixed_859267", "mixed_52437899", "mixed_111947"],
         [10, 11, 12, 13, 14]),
        ("mixed_among_valid", k(20) + ["mixed_859267"] + k(21), [20, 12, 21]),
        ("torsion_parts_cancel", ["mixed_11", "mixed_11_minus"], [10, 16]),
        ("mixed_and_its_negative", ["mixed_11", "mixed_11_flip"], []),
        ("torsion_and_key", ["torsion_11", "k22"], [22]),
        ("wrong_signer", k(20, 21), [20]),
        ("flipped_record", k(20) + ["flip_key6"], [20, 6]),
    ]
    partner_root = hashlib.sha256(b"pk-edges-set:partner").digest()
    partner_sig = o.g2_compress(o.g2_mul(hash_once(partner_root), c.sks[120]))
    partner = {"records": ["k120"], "root": partner_root.hex(), "sig": partner_sig.hex()}
    out = []
    for name, refs, signers in cases:
        root = hashlib.sha256(b"pk-edges-set:" + name.encode()).digest()
        sk = sum(c.sks[j] for j in signers) % o.R if signers else c.sks[0]
        sig = o.g2_compress(o.g2_mul(hash_once(root), sk))
        code, acc = 0, None
        for ref in refs:
            try:
                acc = o.g1_add(acc, o.g1_deserialize(record(ref, c, by_name)))
            except o.BlstError as err:
                code = err.code
                break
        if code:
            expect = pair = -code
        else:
            expect = int(o.verify_signature_sets_maybe_batch([(acc, root, sig)]))
            try:
                pair = int(o.verify_signature_sets_maybe_batch(
                    [(c.pks[120], partner_root, partner_sig), (acc, root, sig)], PAIR_SCALARS))
            except o.BlstError as err:
                pair = -err.code
        out.append({"name": name, "records": refs, "root": root.hex(), "sig": sig.hex(), "expect": expect,
                    "pair_expect": pair})
    got = {s["name"]: (s["expect"], s["pair_expect"]) for s in out}
    assert got["bad_first"] == (-1, -1) and got["bad_middle"] == (-2, -2) and got["bad_last"] == (-3, -3)
    assert got["two_bad_codes"] == (-2, -2) and got["two_bad_codes_reversed"] == (-1, -1)
    assert got["all_infinity"] == (0, -6) and got["cancel"] == (0, -6) and got["mixed_and_its_negative"] == (0, -6)
    for name in ("infinity_among_valid", "cancel_then_key", "twice", "thrice", "compressed_among_uncompressed",
                 "records_17", "records_65", "all_mixed", "torsion_parts_cancel", "torsion_and_key"):
        assert got[name] == (1, 1), (name, got[name])
    assert got["wrong_signer"] == (0, 0) and got["flipped_record"] == (0, 0)
    assert max(len(s["records"]) for s in out) == 65
    return partner, out


def main():
    keys = json.load(open(os.path.join(GOLD, "keys.json")))
    sks = [int(s, 16) for s in keys["sk"]]
    pks = [o.g1_decompress(bytes.fromhex(k)) for k in keys["pk_compressed"][:len(sks)]]
    for j in (0, 16, 120):
        assert o.sk_to_pk(sks[j]) == pks[j]
    o.hash_to_g2 = hash_once
    try:
        c = Corpus(sks, pks)
        build_entries(c, torsion_points())
        assert len({e["name"] for e in c.entries}) == len(c.entries)
        partner, sets = build_sets(c)
    finally:
        o.hash_to_g2 = _hash
    with open(OUT, "w") as f:
        json.dump({"note": "tools/gen_golden_pk_edges.py: crafted G1 wire bytes (pk48 compressed, pk96 records) and "
                           "the answers of oracle/bls12381.py: expect48 / expect96 the BLST code of g1_decompress / "
                           "g1_deserialize, validate of pubkey_validate, deposit of deposit_valid, verdict of "
                           "core_verify(point, root, sig) for the decoded point taken on trust; keys and secret "
                           "keys are those of keys.json.  sets: multi-record sets, a reference being k<j> / c<j> / "
                           "n<j> (key j uncompressed / compressed with a zero tail / negated), inf, cinf or an "
                           "entry's name; expect the one-set job's code, pair_expect that of the non-batchable "
                           "job [pair_partner, set]",
                   "agg_keys": AGG_KEYS, "entries": c.entries, "pair_partner": partner, "sets": sets},
                  f, indent=0, sort_keys=True)
        f.write("\n")
    for e in c.entries:
        print("%-36s 48:%-4s 96:%-4s validate %-2s verdict %-2s deposit %s" % (
            e["name"], "inf" if e.get("infinity48") else e.get("expect48", "-"),
            "inf" if e.get("infinity96") else e.get("expect96", "-"), e.get("validate", "-"),
            e.get("verdict", "-"), e.get("deposit", "-")))
    for s in sets:
        print("%-36s %2d records: %2d, paired %2d" % (s["name"], len(s["records"]), s["expect"], s["pair_expect"]))
    print("%d entries, %d sets, %d bytes" % (len(c.entries), len(sets), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
