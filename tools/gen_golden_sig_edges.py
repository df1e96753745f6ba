"""Crafted 96-byte G2 wire encodings for every signature-decoding route of the device, with the
oracle's answer for each: tests/golden/sig_edges.json (data only).

    python tools/gen_golden_sig_edges.py

Everything here comes from oracle/bls12381.py and integer arithmetic; nothing from the device
code.  Each entry has `name`, `kind`, `sig` (hex), `expect` (0 or the BLST code of
o.signature_from_bytes) and, where the bytes decode to a finite point, `x` / `y` as [c0, c1] hex.

kinds
  small      points of small order q on the twist E'(Fp2): T = [n / q^2] P (n / q where q divides
             the order once) of a random P, n = h2 r the order of E'(Fp2),
             h2 = (x^8 - 4x^7 + 5x^6 - 4x^4 + 6x^3 - 4x^2 - 4x + 13) / 9
                = 13^2 23^2 2713 11953 262069 (a 448-bit factor).
             `hits_exceptional`: whether the chain of tc_mul_x_abs (accumulator P; from bit 62 of
             |x| down: double, then add P at a set bit) meets an addition whose accumulator is
             0, P or -P, i.e. is 0, 1 or q - 1 mod q: computed from the integers alone.  Only
             order 13 does (acc = -P at bit 60, then infinity at bit 57), whatever the multiple,
             so the corpus holds three distinct points of order 13.
  mixed      S + T, S a golden signature (in G2): the small-subgroup shape
  sqrt       x = a + b i with 3 a^2 b - b^3 = -4, so that x^3 + 4 (1 + i) lies in Fp: y has
             c1 = 0 (y^2 a square of Fp) or c0 = 0 (a non-square); both sort bits.  Every element
             of Fp is a square in Fp2, so no such x is off the curve.  And two generic points,
             one per quadratic character of delta = (a0 + g) / 2, g = n^((p + 1) / 4) the root
             of the norm n of y^2 that the device's square root takes.
  x0         x = 0
  boundary   field-boundary and flag encodings
  flip       a golden signature with the sort bit toggled: decodes (status 0) to -sig, and must
             verify false; `key` and `msg` say whose it was
  length     0, 95, 97 and 192 bytes

`sum_sigs` are 130 distinct valid signatures (interop keys over one root) and `aggregates` the
lists of one Signature.aggregate call with the answer of o.signatures_aggregate for each: every
entry alone and between two valid signatures, valid lists among them, and the sums that take a
64-lane strided sum past its first turn (65 and 130 signatures, equal signatures in a lane and
at the tree levels, a signature and its sort-flipped twin, infinity mid-stride, an empty list
between full ones).  The table of names and codes is printed; the run takes about a minute.
"""
import hashlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bls12381 as o  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "sig_edges.json")
P = o.P
X = o.X
H2_NUM = X**8 - 4 * X**7 + 5 * X**6 - 4 * X**4 + 6 * X**3 - 4 * X**2 - 4 * X + 13
assert H2_NUM % 9 == 0
H2 = H2_NUM // 9
N_TWIST = H2 * o.R  # the order of E'(Fp2)
SMALL_PRIMES = (13, 23, 2713, 11953, 262069)  # trial division of H2


def check_cofactor():
    t = H2
    exps = {}
    for q in SMALL_PRIMES:
        while t % q == 0:
            t //= q
            exps[q] = exps.get(q, 0) + 1
    assert exps == {13: 2, 23: 2, 2713: 1, 11953: 1, 262069: 1}, exps
    assert t.bit_length() == 448
    return exps


def hits_exceptional(q):
    """The |x| chain on the integers mod the point's order q."""
    acc = 1
    for i in range(62, -1, -1):
        acc = 2 * acc % q
        if (o.X_ABS >> i) & 1:
            if acc in (0, 1, q - 1):
                return True
            acc = (acc + 1) % q
    return False


def curve_y(x):
    return o.f2_sqrt(o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B2))


def random_twist_point(rng):
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = curve_y(x)
        if y is not None:
            return (x, y)


def small_order_point(rng, q, exps):
    """A point of exact order q (a prime), from a random point of E'(Fp2)."""
    m = N_TWIST // q ** exps[q]
    while True:
        t = o.g2_mul(random_twist_point(rng), m)
        if t is None:
            continue
        while o.g2_mul(t, q) is not None:  # a cyclic q^2 part would need this; never taken so far
            t = o.g2_mul(t, q)
        return t


def check_small(t, order):
    assert o.g2_on_curve(t) and t is not None
    assert o.g2_mul(t, order) is None
    for q in SMALL_PRIMES:
        if order % q == 0:
            assert o.g2_mul(t, order // q) is not None  # exact order
    assert not o.g2_in_group(t)


def hx(v):
    return "%096x" % v


def entry(name, kind, sig, **extra):
    e = {"name": name, "kind": kind, "sig": bytes(sig).hex()}
    try:
        pt = o.g2_decompress(bytes(sig))
        decoded = True
    except o.BlstError:
        pt, decoded = None, False
    try:
        o.signature_from_bytes(bytes(sig))
        e["expect"] = 0
    except o.BlstError as err:
        e["expect"] = err.code
    if decoded and pt is None:
        e["infinity"] = True
    if pt is not None:
        e["x"] = [hx(pt[0][0]), hx(pt[0][1])]
        e["y"] = [hx(pt[1][0]), hx(pt[1][1])]
    e.update(extra)
    return e


def raw_x(c0, c1, flags=0x80):
    """The wire bytes of x = c0 + c1 i as given (no reduction): c1 below 2^381, c0 below 2^384."""
    assert 0 <= c1 < 1 << 381 and 0 <= c0 < 1 << 384
    b = bytearray(c1.to_bytes(48, "big") + c0.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def toggled(sig, bit=0x20):
    return bytes([sig[0] ^ bit]) + bytes(sig[1:])


def sqrt_branch_points():
    """x = a + b i on 3 a^2 b - b^3 = -4 for small b: y^2 = a^3 - 3 a b^2 + 4 in Fp."""
    found = {}
    for b in range(1, 200):
        a2 = (b**3 - 4) * o.inv(3 * b) % P
        a = o.fp_sqrt(a2)
        if a is None:
            continue
        for aa in (a, (-a) % P):
            x = (aa, b)
            y2 = o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B2)
            assert y2[1] == 0
            kind = "y2_fp_square" if o.fp_is_square(y2[0]) else "y2_fp_nonsquare"
            if kind not in found:
                y = curve_y(x)
                assert y is not None and (y[1] == 0 if kind == "y2_fp_square" else y[0] == 0)
                found[kind] = (x, y, b)
        if len(found) == 2:
            return found
    raise AssertionError("no small b gives both branches")


def delta_is_square(y2):
    """The quadratic character of delta as fp2_sqrt_t computes it (a1 != 0)."""
    n = (y2[0] * y2[0] + y2[1] * y2[1]) % P
    g = pow(n, (P + 1) // 4, P)
    assert g * g % P == n
    d = (y2[0] + g) * o.inv(2) % P
    return o.fp_is_square(d)


def generic_delta_points():
    found = {}
    k = 2
    while len(found) < 2:
        x = (k, 3)
        y2 = o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B2)
        y = o.f2_sqrt(y2)
        if y is not None and y2[1] != 0:
            kind = "delta_square" if delta_is_square(y2) else "delta_nonsquare"
            found.setdefault(kind, (x, y))
        k += 1
    return found


N_SUM = 130  # distinct valid signatures for the sums: two full strides of a 64-lane sum and a short one
INF_SIG = bytes([0xC0]) + bytes(95)


def resolve(ref, sum_sigs, by_name):
    if ref == "inf":
        return INF_SIG
    if ref in by_name:
        return bytes.fromhex(by_name[ref]["sig"])
    s = sum_sigs[int(ref[1:])]
    return toggled(s) if ref[0] == "f" else s


def aggregate_cases(entries):
    """One aggregation call: every entry alone and between two valid signatures, a valid aggregate
    after each second entry, then the sums that take a 64-lane strided sum past its first turn."""
    root = hashlib.sha256(b"sig-edges-sums").digest()
    h = o.hash_to_g2(root)
    sum_sigs = [o.g2_compress(o.g2_mul(h, o.interop_secret_key(j))) for j in range(N_SUM)]
    assert len(set(sum_sigs)) == N_SUM
    by_name = {e["name"]: e for e in entries}
    s = lambda *js: ["s%d" % j for j in js]  # noqa: E731
    cases = []
    for j, e in enumerate(entries):
        cases.append(("alone_" + e["name"], [e["name"]]))
        cases.append(("between_" + e["name"], s(2 * j % N_SUM) + [e["name"]] + s((2 * j + 1) % N_SUM)))
        if j & 1:
            cases.append(("valid_after_" + e["name"], s(j)))
    run66 = s(*range(66))
    run66[1] = run66[64] = "inf"  # lane 1: infinity, then a point; lane 0: a point, then infinity
    cases += [
        ("run_65", s(*range(65))),
        ("run_130", s(*range(N_SUM))),
        ("empty_between_full_runs", []),
        ("repeat_128", s(*[k % 64 for k in range(128)])),  # sigs[k] == sigs[k + 64]: a lane doubles
        ("pair_equal", s(3, 3)),
        ("four_equal", s(5, 5, 5, 5)),  # equal points at two tree levels
        ("cancel", ["s7", "f7"]),  # infinity, encoded 0xC0, status 0
        ("cancel_then_point", ["s7", "f7", "s8"]),
        ("infinity_between", ["s0", "inf", "s1"]),
        ("infinity_mid_stride", run66),
        ("all_infinity", ["inf", "inf"]),
    ]
    # the oracle decodes and validates a signature each time it meets it: remember the pure function's answers
    plain = o.signature_from_bytes
    memo = {}

    def remembered(b, validate=True):
        k = (bytes(b), validate)
        if k not in memo:
            try:
                memo[k] = (plain(b, validate), None)
            except o.BlstError as err:
                memo[k] = (None, err.code)
        if memo[k][1] is not None:
            raise o.BlstError(memo[k][1])
        return memo[k][0]

    o.signature_from_bytes = remembered
    try:
        out = []
        for name, refs in cases:
            code, agg = o.signatures_aggregate([resolve(r, sum_sigs, by_name) for r in refs])
            out.append({"name": name, "sigs": refs, "expect": code, "aggregate": agg.hex() if agg else None})
    finally:
        o.signature_from_bytes = plain
    got = {c["name"]: c for c in out}
    assert got["cancel"]["aggregate"] == INF_SIG.hex() and got["all_infinity"]["aggregate"] == INF_SIG.hex()
    assert got["cancel_then_point"]["aggregate"] == sum_sigs[8].hex()
    assert got["empty_between_full_runs"]["expect"] == 20
    assert sum(len(c["sigs"]) for c in out) < 700
    return sum_sigs, out


def main():
    exps = check_cofactor()
    rng = random.Random(0x516ED6E5)
    keys = json.load(open(os.path.join(GOLD, "keys.json")))
    golden = json.load(open(os.path.join(GOLD, "signatures.json")))["cases"]
    sig0 = bytes.fromhex(golden[0]["sig"])
    entries = []

    # ---- small order -------------------------------------------------------------------
    t13 = small_order_point(rng, 13, exps)
    t13b = small_order_point(rng, 13, exps)
    while t13b in [o.g2_mul(t13, k) for k in range(1, 13)]:  # a second subgroup of order 13
        t13b = small_order_point(rng, 13, exps)
    t23 = small_order_point(rng, 23, exps)
    t2713 = small_order_point(rng, 2713, exps)
    small = [("small_13", t13, 13), ("small_13_times5", o.g2_mul(t13, 5), 13), ("small_13_other", t13b, 13),
             ("small_23", t23, 23), ("small_299", o.g2_add(t13, t23), 299), ("small_2713", t2713, 2713)]
    for name, t, order in small:
        check_small(t, order)
        entries.append(entry(name, "small", o.g2_compress(t), order=order, hits_exceptional=hits_exceptional(order)))
    assert sum(e["hits_exceptional"] for e in entries) >= 2
    assert len({e["sig"] for e in entries}) == len(entries)

    # ---- mixed order: a golden signature plus a small-order point -------------------------
    for j, (name, t, order) in enumerate(small):
        g = golden[j]
        s = o.sign(int(keys["sk"][g["key"]], 16), bytes.fromhex(g["msg"]))
        assert o.g2_compress(s).hex() == g["sig"] and o.g2_in_group(s)
        st = o.g2_add(s, t)
        assert st is not None and o.g2_on_curve(st) and not o.g2_in_group(st)
        # the chain runs on integers mod order * r: 0, 1 or -1 is out of reach of a 64-bit prefix
        entries.append(entry("mixed_" + name[6:], "mixed", o.g2_compress(st), order=order, key=g["key"],
                             msg=g["msg"], hits_exceptional=False))
        assert entries[-1]["expect"] == o.BLST_POINT_NOT_IN_GROUP

    # ---- the square root's branches -------------------------------------------------------
    notes = []
    for kind, (x, y, b) in sorted(sqrt_branch_points().items()):
        for sort in (0, 1):
            sig = o.g2_compress((x, y))
            sig = bytes([(sig[0] & ~0x20) | (0x20 if sort else 0)]) + sig[1:]
            entries.append(entry("sqrt_%s_sort%d" % (kind, sort), "sqrt", sig, branch=kind, b=b))
            assert entries[-1]["expect"] == o.BLST_POINT_NOT_IN_GROUP
    notes.append("sqrt: no x with y^2 in Fp is off the curve (every element of Fp is a square in Fp2)")
    for kind, (x, y) in sorted(generic_delta_points().items()):
        entries.append(entry("sqrt_" + kind, "sqrt", o.g2_compress((x, y)), branch=kind))

    # ---- x = 0 ----------------------------------------------------------------------------
    for sort in (0, 1):
        entries.append(entry("x0_sort%d" % sort, "x0", raw_x(0, 0, 0x80 | (0x20 if sort else 0))))

    # ---- boundaries -----------------------------------------------------------------------
    g0 = o.g2_decompress(sig0)
    c0, c1 = g0[0]
    bnd = [
        ("c0_p_minus_1", raw_x(P - 1, c1)), ("c0_p", raw_x(P, c1)), ("c0_p_plus_1", raw_x(P + 1, c1)),
        ("c0_all_ones", raw_x((1 << 384) - 1, c1)),
        ("c1_p_minus_1", raw_x(c0, P - 1)), ("c1_p", raw_x(c0, P)), ("c1_p_plus_1", raw_x(c0, P + 1)),
        ("c1_mid", raw_x(c0, (P + (1 << 381)) // 2)), ("c1_all_ones", raw_x(c0, (1 << 381) - 1)),
        ("both_p_minus_1", raw_x(P - 1, P - 1)), ("both_p_minus_1_sort", raw_x(P - 1, P - 1, 0xA0)),
        ("infinity", bytes([0xC0]) + bytes(95)),
        ("infinity_sort_bit", bytes([0xE0]) + bytes(95)),
        ("infinity_stray_47", bytes([0xC0]) + bytes(46) + b"\x01" + bytes(48)),
        ("infinity_stray_48", bytes([0xC0]) + bytes(47) + b"\x80" + bytes(47)),
        ("infinity_stray_95", bytes([0xC0]) + bytes(94) + b"\x01"),
        ("infinity_stray_flag_low", bytes([0xC1]) + bytes(95)),
        ("flag_40_only_zero", bytes([0x40]) + bytes(95)),
        ("flag_40_only_point", bytes([(sig0[0] & 0x3F) | 0x40]) + sig0[1:]),
        ("flag_none_point", bytes([sig0[0] & 0x1F]) + sig0[1:]),
    ]
    for name, sig in bnd:
        entries.append(entry(name, "boundary", sig))

    # ---- sort-bit flips of valid signatures -------------------------------------------------
    for g in golden[8:12]:
        sig = bytes.fromhex(g["sig"])
        e = entry("flip_key%d" % g["key"], "flip", toggled(sig), key=g["key"], msg=g["msg"])
        assert e["expect"] == 0 and o.signature_from_bytes(toggled(sig)) == o.g2_neg(o.signature_from_bytes(sig))
        entries.append(e)

    # ---- lengths ------------------------------------------------------------------------------
    for name, sig in (("len_0", b""), ("len_95", sig0[:95]), ("len_97", sig0 + b"\0"),
                      ("len_192", o.g2_serialize(g0))):
        entries.append(entry(name, "length", sig))
        assert entries[-1]["expect"] == o.BLST_INVALID_SIZE

    assert len({e["name"] for e in entries}) == len(entries)
    sum_sigs, aggregates = aggregate_cases(entries)
    with open(OUT, "w") as f:
        json.dump({"note": "tools/gen_golden_sig_edges.py: crafted G2 wire bytes and the code of oracle/bls12381.py "
                           "signature_from_bytes (0 or the BLST number); x, y as [c0, c1] where the bytes decode.  "
                           "aggregates: one Signature.aggregate call's lists, each reference s<j> = sum_sigs[j], "
                           "f<j> = its sort-flipped twin, inf = the infinity encoding, else an entry's name; "
                           "expect / aggregate from oracle signatures_aggregate",
                   "notes": notes, "entries": entries, "sum_sigs": [s.hex() for s in sum_sigs],
                   "aggregates": aggregates}, f, indent=0, sort_keys=True)
        f.write("\n")
    for e in entries:
        print("%-34s %d%s" % (e["name"], e["expect"],
                              "  hits_exceptional" if e.get("hits_exceptional") else ""))
    for n in notes:
        print(n)
    print("%d entries, %d bytes" % (len(entries), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
