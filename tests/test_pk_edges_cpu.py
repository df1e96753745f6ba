"""CPU: the crafted G1 wire bytes of tests/golden/pk_edges.json (tools/gen_golden_pk_edges.py,
oracle only) through the host build of the device's pubkey decoding, tests/native/hostsim.cpp.

g1_decompress (48-byte keys: k_pk_validate, k_cache_put_compressed) and g1_deserialize (96-byte
records: k_cache_put_uncompressed, the record branch of pk_sum) give the oracle's code and, where
the bytes decode, the oracle's point, sign of y included.

The keys the device takes on trust may lie outside G1.  jac_mul_glv computes a P + b E(P) for the
randomizer r = a + b x^2; on G1 that is r P, off it the two differ by a point of the cofactor's
torsion, which [h] removes (and the final exponentiation on the device).  So for every torsion and
mixed-order point and a handful of the words of tests/randomizer_edges.py, [h] got must equal
[h] (r P) by the oracle, and for a point in G1 got must equal r P itself.

The fixture is re-derived in part from the oracle (every code; a sample of verdicts), as the other
golden tests do.  Integer work, bit-exact.
"""
import ctypes

import pytest

from oracle import bls12381 as o
from tests import hostsim as hs
from tests import pk_edges as pe
from tests import sig_edges as se
from tests.randomizer_edges import EDGE_WORDS, glv_scalar

CORPUS = pe.corpus()
H1 = 0x396C8C005555E1568C00AAAB0000AAAB
# digit 8 alone, every carry, c_8, c_8' into an accumulator at infinity, both halves alike, the full chain over a 7
WORDS = [EDGE_WORDS[i] for i in (4, 10, 15, 31, 36, len(EDGE_WORDS) - 1)]


@pytest.fixture(scope="module", params=["wide", "classic"])
def L(request):
    return hs.lib(request.param)


def test_corpus_shape():
    """What the other tests rely on: every kind is there, each form's code and point are what the
    oracle decodes, and the subgroup entries have the orders and verdicts they are named for."""
    assert {e["kind"] for e in CORPUS} == {"flags", "infinity", "field", "flip", "limb", "valid", "torsion", "mixed"}
    for e in CORPUS:
        for form, fn in ((48, o.g1_decompress), (96, o.g1_deserialize)):
            if "pk%d" % form not in e:
                continue
            try:
                pt = fn(e["pk%d" % form])
            except o.BlstError as err:
                assert err.code == e["expect%d" % form], e["name"]
                continue
            assert e["expect%d" % form] == 0 and (pt is None) == bool(e.get("infinity%d" % form)), e["name"]
            if pt is not None:
                assert pt == pe.point(e), e["name"]
        if "pk48" in e:
            assert o.pubkey_validate(e["pk48"]) == e["validate"], e["name"]
    assert {e["order"] for e in CORPUS if e["kind"] == "torsion"} >= {11, 10177, 859267, 52437899, 11 * 10177}
    for e in CORPUS:
        if e["kind"] == "torsion":
            assert o.g1_mul(pe.point(e), e["order"]) is None and e["verdict"] == 0 and e["validate"] == 3
        if e["kind"] == "mixed":
            pt = pe.point(e)
            assert o.g1_on_curve(pt) and o.g1_mul(pt, o.R) is not None and e["validate"] == 3 and e["deposit"] == 0
            assert o.g1_mul(pt, o.R * e["order"]) is None
        if e["kind"] == "limb":
            assert (e["x"] >> (28 * e["limb"])) & 0xFFFFFFF == (0 if e["name"].endswith("zero") else 0xFFFFFFF)
    assert sum(e["verdict"] for e in CORPUS if e["kind"] == "mixed") >= 6
    # non-canonical coordinates: at or above p, the three flag bits clear
    for name, off in (("noncanonical_x", 0), ("noncanonical_y", 48)):
        e = next(e for e in CORPUS if e["name"] == name)
        v = int.from_bytes(e["pk96"][off:off + 48], "big")
        assert o.P <= v < 1 << 381 and e["expect96"] == o.BLST_BAD_ENCODING


def test_fixture_regenerates():
    """A sample of verdicts again from the oracle: a valid key, a sort flip, a pure torsion point,
    two mixed-order keys (one with its 16-key sum), and three multi-record sets through the
    one-set and the two-set job."""
    by = {e["name"]: e for e in CORPUS}
    for name in ("valid_key8", "flip_key6", "torsion_11", "mixed_11", "mixed_111947"):
        e = by[name]
        sig = o.signature_from_bytes(e["sig"])
        assert int(o.core_verify(pe.point(e), e["root"], sig)) == e["verdict"], name
        assert int(o.deposit_valid(e["pk48"], e["root"], e["sig"])) == e["deposit"], name
    _, pk96 = pe.keys()
    e = by["mixed_11"]
    agg = pe.point(e)
    for j in pe.fixture()["agg_keys"]:
        agg = o.g1_add(agg, o.g1_deserialize(pk96[j]))
    assert int(o.core_verify(agg, e["root"], o.signature_from_bytes(e["agg_sig"]))) == e["agg_verdict"] == 1
    sets, partner = pe.record_sets(o)
    ppk = o.g1_deserialize(partner["records"][0])
    for s in sets:
        if s["name"] not in ("two_bad_codes", "cancel", "torsion_parts_cancel"):
            continue
        try:
            acc = o.pubkey_aggregate([o.g1_deserialize(r) for r in s["records"]])
        except o.BlstError as err:
            assert (s["expect"], s["pair_expect"]) == (-err.code, -err.code), s["name"]
            continue
        assert int(o.verify_signature_sets_maybe_batch([(acc, s["root"], s["sig"])])) == s["expect"], s["name"]
        try:
            pair = int(o.verify_signature_sets_maybe_batch(
                [(ppk, partner["root"], partner["sig"]), (acc, s["root"], s["sig"])], [3, 5]))
        except o.BlstError as err:
            pair = -err.code
        assert pair == s["pair_expect"], s["name"]


@pytest.mark.parametrize("form", [48, 96])
def test_decode(L, form):
    entries = pe.with_form(CORPUS, form)
    got = [hs.g1_decode(L, e["pk%d" % form]) for e in entries]
    assert se.mismatches(entries, [st for st, _ in got], lambda e: pe.decode_status(e, form)) == []
    ok = [(e, pt) for e, (st, pt) in zip(entries, got) if st == 0]
    assert se.mismatches([e for e, _ in ok], [pt for _, pt in ok], pe.point) == []  # the exact point, sign included
    assert len(ok) >= 20 and len(entries) - len(ok) >= 20


def test_record_sets_decode(L):
    """Every record of the multi-record sets through hs_g1_deserialize and a plain sum: the first
    undecodable record's code, else the oracle's sum (hs_g1_add is the complete addition)."""
    sets, _ = pe.record_sets(o)
    for s in sets:
        code, acc = 0, None
        for r in s["records"]:
            st, pt = hs.g1_decode(L, r)
            if st not in (0, se.ST_INFINITY):
                code = st
                break
            acc = o.g1_add(acc, pt)
        try:
            want = (0, o.pubkey_aggregate([o.g1_deserialize(r) for r in s["records"]]))
        except o.BlstError as err:
            want = (err.code, None)
        assert (code, acc if code == 0 else None) == want, s["name"]
        if code:
            assert s["expect"] == -code


def test_glv_off_subgroup():
    """G1 arithmetic is the same code in both host builds, so one of them runs this.  [h] (r P) is
    r ([h] P) with [h] P in G1, so the oracle multiplies that point, once per word."""
    L = hs.lib("wide")
    pts = [e for e in CORPUS if e["kind"] in ("torsion", "mixed") or e["name"] in ("valid_key8", "flip_key6")]
    assert sum(e["kind"] == "torsion" for e in pts) >= 5 and sum(e["kind"] == "mixed" for e in pts) >= 7
    out = hs.buf(96)
    bad = []
    for e in pts:
        p = pe.point(e)
        hp = o.g1_mul(p, H1)
        assert (hp is None) == (e["kind"] == "torsion")
        for k in WORDS:
            fin = L.hs_g1_mul_glv(out, hs.g1_b(p), ctypes.c_uint64(k))
            got = hs.b_g1(out.raw) if fin else None
            if not o.g1_on_curve(got):
                bad.append("%s %#x: off the curve" % (e["name"], k))
            elif e["validate"] == 0:
                if got != o.g1_mul(p, glv_scalar(k)):
                    bad.append("%s %#x: in G1, got differs" % (e["name"], k))
            elif o.g1_mul(got, H1) != o.g1_mul(hp, glv_scalar(k)):
                bad.append("%s %#x: [h] got differs" % (e["name"], k))
    assert bad == []


@pytest.mark.parametrize("wide", [1, 0], ids=["four-part", "plain"])
def test_team_g1_off_subgroup(wide):
    """k_prep_wide's r pk (bgv_tg1.h tg1_mul_glv on the generic-case addition programs) against
    the one-lane jac_mul_glv on every point a trusted key can be.  A pure torsion point of order
    11 meets exceptional additions for about a third of the words; each leaves Z = 0
    (tg1_exceptional), where the kernel and the host emulation repeat the multiplication with
    the complete formulas.  A wrong point with Z != 0 fails here."""
    L = hs.lib("wide")
    pts = [e for e in CORPUS if e["kind"] in ("torsion", "mixed", "limb")]
    bad = []
    L.hs_set_wide_rounds(wide)
    try:
        for e in pts:
            bad += ["%s %#x" % (e["name"], k) for k in EDGE_WORDS
                    if L.hs_tg1_check(hs.g1_b(pe.point(e)), ctypes.c_uint64(k)) != 1]
    finally:
        L.hs_set_wide_rounds(0)
    assert bad == []


def test_comparison_can_fail(L):
    """Negative control: with one entry's expected code swapped for its neighbour's, the helper
    reports exactly that entry."""
    wire = pe.with_form(CORPUS, 96)
    got = [hs.g1_decode(L, e["pk96"])[0] for e in wire]
    st = lambda e: pe.decode_status(e, 96)  # noqa: E731
    j = next(i for i in range(len(wire) - 1) if st(wire[i]) != st(wire[i + 1]))
    swapped = [dict(e) for e in wire]
    swapped[j]["expect96"], swapped[j]["infinity96"] = wire[j + 1]["expect96"], wire[j + 1].get("infinity96")
    bad = se.mismatches(swapped, got, st)
    assert len(bad) == 1 and bad[0].startswith(wire[j]["name"] + ":")

