"""CPU: the crafted G2 wire bytes of tests/golden/sig_edges.json (tools/gen_golden_sig_edges.py,
oracle only) through the host build of the device's signature decoding, tests/native/hostsim.cpp.

Lane decode: g2_decompress (fp2_sqrt_t<bgv_pow_lane>, fp2_lex_largest) and the one-lane
g2_in_subgroup (jac_mul_x_abs) give the oracle's code and, where the bytes decode, the oracle's y.

Team subgroup check: k_prep_wide's plane-2 schedule (tc_mul_x_abs on the generic-case addition
programs, then psi(P) == -[|x|]P) on tc_host_engine.  Its exceptional-addition flag is set exactly
for the points whose order makes the |x| chain meet 0, P or -P (`hits_exceptional`, worked out from
the integers by the generator), the verdict with the one-lane fallback is the oracle's, and with
the flag clear the chain's own verdict already is.

The length entries (0, 95, 97, 192 bytes) have no host function to go through: the kernels test
sig_len before they read a byte, so those run on the device only (tests/test_gpu_sig_edges.py).
The wave-cooperative square root (bgv_wfp.h bgv_pow_wave) is device code (cross-lane builtins);
tools/emu_wfp.py emulates its products, not fp2_sqrt_t, so route C's square root is left to the
GPU test as well.  Integer work, bit-exact.
"""
import ctypes

import pytest

from oracle import bls12381 as o
from tests import hostsim as hs
from tests import sig_edges as se

CORPUS = se.corpus()
WIRE = [e for e in CORPUS if len(e["sig"]) == 96]
POINTS = [e for e in WIRE if "x" in e]


@pytest.fixture(scope="module", params=["wide", "classic"])
def L(request):
    return hs.lib(request.param)


def test_corpus_shape():
    """What the other tests rely on: the kinds are all there, the stored points are what the
    oracle decodes, and at least two small-order points meet an exceptional addition."""
    kinds = {e["kind"] for e in CORPUS}
    assert kinds == {"small", "mixed", "sqrt", "x0", "boundary", "flip", "length"}
    assert sorted(len(e["sig"]) for e in CORPUS if e["kind"] == "length") == [0, 95, 97, 192]
    assert all(e["expect"] == o.BLST_INVALID_SIZE for e in CORPUS if e["kind"] == "length")
    assert sum(1 for e in CORPUS if e.get("hits_exceptional")) >= 2
    assert {e["order"] for e in CORPUS if e["kind"] == "small"} >= {13, 23, 13 * 23, 2713}
    assert {e["branch"] for e in CORPUS if e["kind"] == "sqrt"} == {
        "y2_fp_square", "y2_fp_nonsquare", "delta_square", "delta_nonsquare"}
    for e in WIRE:
        try:
            pt = o.g2_decompress(e["sig"])
        except o.BlstError as err:
            assert err.code == e["expect"] and "x" not in e, e["name"]
            continue
        assert (pt is None) == bool(e.get("infinity")), e["name"]
        if pt is not None:
            assert pt == (e["x"], e["y"]), e["name"]
    for e in CORPUS:
        if e.get("branch") == "y2_fp_square":
            assert e["y"][1] == 0 and e["y"][0] != 0
        if e.get("branch") == "y2_fp_nonsquare":
            assert e["y"][0] == 0 and e["y"][1] != 0


def lane_status(L, e):
    """(the route's status, the decoded point or None) of task_sig's decode and subgroup check."""
    out = hs.buf(192)
    rc = L.hs_g2_decompress(out, e["sig"])
    if rc:
        return rc, None
    pt = hs.b_g2(out.raw)
    return (0 if L.hs_g2_in_subgroup(out.raw) else o.BLST_POINT_NOT_IN_GROUP), pt


def test_lane_decode(L):
    got = [lane_status(L, e) for e in WIRE]
    assert se.mismatches(WIRE, [st for st, _ in got]) == []
    for e, (_, pt) in zip(WIRE, got):
        if "x" in e:
            assert pt == (e["x"], e["y"]), e["name"]  # the exact root, sign included
        else:
            assert pt is None, e["name"]
    assert len(POINTS) >= 20  # six small, six mixed, six sqrt, four flips at the least


def team_subgroup(L, pt):
    bad, plain = ctypes.c_int(7), ctypes.c_int(7)
    full = L.hs_team_subgroup(hs.g2_b(pt), ctypes.byref(bad), ctypes.byref(plain))
    assert bad.value in (0, 1) and plain.value in (0, 1) and full in (0, 1)
    return bad.value, plain.value, full


@pytest.mark.parametrize("wide", [1, 0], ids=["four-part", "plain"])
def test_team_subgroup_check(L, wide):
    L.hs_set_wide_rounds(wide)
    try:
        res = [team_subgroup(L, (e["x"], e["y"])) for e in POINTS]
        gold = [team_subgroup(L, o.g2_decompress(bytes.fromhex(c["sig"])))
                for c in se.load("signatures.json")["cases"][:4]]
    finally:
        L.hs_set_wide_rounds(0)
    # a valid signature: in the group, by the chain alone
    assert gold == [(0, 1, 1)] * 4
    flagged = [e for e in POINTS if e["kind"] in ("small", "mixed")]
    assert len(flagged) >= 12
    by_name = {e["name"]: r for e, r in zip(POINTS, res)}
    assert [(e["name"], by_name[e["name"]][0]) for e in flagged] == [
        (e["name"], int(e["hits_exceptional"])) for e in flagged]
    assert sum(r[0] for r in res) >= 2  # the fallback did run
    in_group = lambda e: int(e["expect"] == 0)  # noqa: E731
    assert se.mismatches(POINTS, [r[2] for r in res], in_group) == []
    clear = [(e, r) for e, r in zip(POINTS, res) if r[0] == 0]
    assert se.mismatches([e for e, _ in clear], [r[1] for _, r in clear], in_group) == []


def test_comparison_can_fail(L):
    """Negative control: with one entry's expected code swapped for its neighbour's, the helper
    reports exactly that entry."""
    got = [lane_status(L, e)[0] for e in WIRE]
    j = next(i for i in range(len(WIRE) - 1) if se.decode_status(WIRE[i]) != se.decode_status(WIRE[i + 1]))
    swapped = [dict(e) for e in WIRE]
    swapped[j]["expect"], swapped[j]["infinity"] = WIRE[j + 1]["expect"], WIRE[j + 1].get("infinity")
    bad = se.mismatches(swapped, got)
    assert len(bad) == 1 and bad[0].startswith(WIRE[j]["name"] + ":")
