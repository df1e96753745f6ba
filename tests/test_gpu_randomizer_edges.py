"""GPU: the six device multiplications by a set's batch randomizer, run over every edge word of
tests/randomizer_edges.py and pinned to oracle/bls12381.py.

A 64-bit word k stands for r = lo32(k) + hi32(k) x^2 mod the group order (glv_scalar).  The device
multiplies by it in six places (bgv_launch_prep in bgv_k_prep.hip routes by the padded slot count n
against BGV_PREP_WIDE_MAX of bgv_device.h, `wide = latency && n <= BGV_PREP_WIDE_MAX`):

  route  value   kernel                       call here
  1      r pk    k_prep (bulk)                debug_prepare(PATH_BULK), 2 sets (64 slots)
  2      r pk    k_prep_wide (latency)        debug_prepare(PATH_LATENCY), 2 sets (64 slots <= the threshold)
  3      r pk    k_prep_a (latency)           debug_prepare(PATH_LATENCY), N_TEAM sets (slots > the threshold)
  4      r sig   k_prep task_sig (bulk)       debug_uniform, 2 sets, one single-slot test
  5      r sig   k_prep_wide (latency)        set_rng_seed + verify_partial, 1 set (64 slots)
  6      r sig   k_prep_team (latency)        set_rng_seed + verify_partial, N_TEAM sets

bgv_profile names only the three launch stages (k_prep, k_miller, k_final), not the kernels inside
k_prep, so the routes are fixed from the routing code: N_TEAM is worked out from the header's
threshold below, and routes 5 / 6 (path chosen by size) skip when BGV_LATENCY_MAX overrides that.

One free slot per call gets the word (seed_for); the slot cycles with the word's index so that the
edge moves across lanes, teams and the 64-slot group boundary.  With pk_i = sk_i G1, sig = sk H(m)
and gt_m = e(G1, H(m)) every expected value is a power of gt_m.  Per route, final_exp(prod_e
v_e^(e + 1)) over all words must equal prod_e expected_e^(e + 1): one final exponentiation, the
distinct small weights keeping one wrong value from hiding behind another; only when that fails,
each word is checked on its own and the assertion names the route and the words.  Bit-exact
integer work, no tolerance.  Reference: packages/beacon-node/src/chain/bls/maybeBatch.ts:18-25
(blst's mul_n_aggregate randomizers).
"""
import hashlib
import os
import re

import pytest

from tests.randomizer_edges import EDGE_WORDS, glv_scalar, seed_for
from tests.test_pairing_golden import f12_from_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
WAVE = 64


def _padded(n):
    return (n + WAVE - 1) // WAVE * WAVE


def _prep_wide_max():
    text = open(os.path.join(CSRC, "bgv_device.h")).read()
    return int(re.search(r"^#define\s+BGV_PREP_WIDE_MAX\s+(\d+)\s*$", text, re.M).group(1))


PREP_WIDE_MAX = _prep_wide_max()  # 340
# the smallest set count whose padded slot count exceeds the threshold: 321 (384 slots) for 340
N_TEAM = next(n for n in range(1, 1 << 16) if _padded(n) > PREP_WIDE_MAX)
NKEYS = N_TEAM + WAVE  # 385: set i names key i; the edge set of slot p carries the signature of key p + 64
SLOTS_SMALL = (0, 1)
SLOTS_TEAM = (0, WAVE - 1, WAVE, N_TEAM - 1)  # 0, 63, 64, 320: both sides of a group boundary, the last set
ROUTES = {
    1: "r pk, k_prep (bulk)",
    2: "r pk, k_prep_wide (latency)",
    3: "r pk, k_prep_a (latency)",
    4: "r sig, k_prep task_sig (bulk)",
    5: "r sig, k_prep_wide (latency)",
    6: "r sig, k_prep_team (latency)",
}


def _slot(route, e):
    if route == 5:
        return 0  # a one-set call has one slot to choose
    slots = SLOTS_TEAM if route in (3, 6) else SLOTS_SMALL
    return slots[e % len(slots)]


@pytest.fixture(scope="module")
def world():
    from lodestar_amd import native
    from oracle import bls12381 as o  # checker only
    assert _padded(2) <= PREP_WIDE_MAX < _padded(N_TEAM) and _padded(N_TEAM - 1) <= PREP_WIDE_MAX
    sks = [o.interop_secret_key(i) for i in range(NKEYS)]
    skb = [sk.to_bytes(32, "big") for sk in sks]
    c = native.Context([0])
    c.keygen(b"".join(skb), cache_first=0, want_pubkeys=False)
    m = hashlib.sha256(b"randomizer-edges-root").digest()
    hm = o.hash_to_g2(m)
    # every key's signature over m (routes 1-4), and set i's over its own root (routes 5, 6)
    sig_m = c.sign(b"".join(skb[:N_TEAM]), m * N_TEAM)
    roots = [hashlib.sha256(b"randomizer-edges-root-%d" % i).digest() for i in range(N_TEAM)]
    sig_own = c.sign(b"".join(skb[:N_TEAM]), b"".join(roots))
    w = {"ctx": c, "sks": sks, "skb": skb, "m": m, "h192": o.g2_serialize(hm), "gt": o.pairing(o.G1, hm),
         "sig_m": [sig_m[96 * i:96 * i + 96] for i in range(N_TEAM)], "roots": roots,
         "sig_own": [sig_own[96 * i:96 * i + 96] for i in range(N_TEAM)], "gt_root": {}, "routes": {}}
    yield w
    c.close()


def _gt_root(world, i):
    """e(G1, H(roots[i])), once per edge root."""
    from oracle import bls12381 as o  # checker only
    if i not in world["gt_root"]:
        world["gt_root"][i] = o.pairing(o.G1, o.hash_to_g2(world["roots"][i]))
    return world["gt_root"][i]


def _confirm_slots(n, edge):
    """Set i of the one non-batchable job is slot i, for every set, in the host's own layout code
    (bgv_host_layout.h through its simulator, tests/retrysim.py; the layout does not look at which
    set is wrong): a layout change fails here, not as a wrong expected value."""
    from tests import retrysim as rs
    sc = rs.scenario("edges-%d" % n, [(n, False)], [(i, rs.WRONG if i == edge else rs.VALID, 0) for i in range(n)],
                     mode=1, layout=True)  # mode 1: BGV_MODE_PER_JOB, as bgv_verify_partial submits
    res = rs.run([sc])[0]
    assert res["nslots"] == _padded(n)
    assert res["slot_root"][:n] == list(range(n)) and all(r == -1 for r in res["slot_root"][n:])


def _prepare_route(world, route):
    """Routes 1-3: per word (value f of the edge slot, base gt, exponent r sk_slot)."""
    from lodestar_amd import native
    n = N_TEAM if route == 3 else 2
    path = native.PATH_BULK if route == 1 else native.PATH_LATENCY
    # real signatures: one of length 0 passes the hook's argument check, but the kernels report
    # BLST_INVALID_SIZE for it and the statuses below are asserted (0, 0); f does not depend on it
    sets =[native.SetSpec(world["m"], world["sig_m"][i], pk_indices=[i]) for i in range(n)]
    out = []
    for e, k in enumerate(EDGE_WORDS):
        slot = _slot(route, e)
        res = world["ctx"].debug_prepare(sets, path, seed=seed_for(k, slot))
        assert len(res) == n
        assert all((ss, ps) == (0, 0) for _, _, ss, ps in res), (route, hex(k))
        assert res[slot][0] == world["h192"], (route, hex(k), slot)
        out.append(([f12_from_bytes(res[slot][1])], "m", world["sks"][slot]))
    return out


def _uniform_route(world):
    """Route 4: per word ((the test's pubkey-sum pair, its signature pair), base gt, exponent)."""
    from lodestar_amd import native
    sets = [native.SetSpec(world["m"], world["sig_m"][i], pk_indices=[i]) for i in range(2)]
    out = []
    for e, k in enumerate(EDGE_WORDS):
        slot = _slot(4, e)
        _, vals = world["ctx"].debug_uniform(sets, seed_for(k, slot), [(1 << slot, False)])
        assert len(vals) == 1
        out.append(([f12_from_bytes(vals[0][0]), f12_from_bytes(vals[0][1])], "m", world["sks"][slot]))
    return out


def _partial_route(world, route):
    """Routes 5, 6: the product path.  Every set valid but the edge one, which names key p = its slot
    and carries the signature of key s = p + 64 over its own root: the valid sets give 1 and the call's
    product final-exponentiates to gt_root^(r (sk_p - sk_s))."""
    from lodestar_amd import native
    from oracle import bls12381 as o  # checker only
    if "BGV_LATENCY_MAX" in os.environ:
        pytest.skip("BGV_LATENCY_MAX is set: the product path's route is not the latency one by size alone")
    c = world["ctx"]
    n = N_TEAM if route == 6 else 1
    slots = sorted({_slot(route, e) for e in range(len(EDGE_WORDS))})
    _confirm_slots(n, slots[-1])
    foreign_sks = b"".join(world["skb"][p + WAVE] for p in slots)
    foreign = c.sign(foreign_sks, b"".join(world["roots"][p] for p in slots))
    foreign = {p: foreign[96 * j:96 * j + 96] for j, p in enumerate(slots)}
    valid = [native.SetSpec(world["roots"][i], world["sig_own"][i], pk_indices=[i]) for i in range(n)]
    out = []
    try:
        for e, k in enumerate(EDGE_WORDS):
            p = _slot(route, e)
            sets = list(valid)
            sets[p] = native.SetSpec(world["roots"][p], foreign[p], pk_indices=[p])
            c.set_rng_seed(seed_for(k, p))
            f576, sig_code, pk_code = c.verify_partial(sets)
            assert (sig_code, pk_code) == (0, 0), (route, hex(k))
            out.append(([f12_from_bytes(f576)], p, (world["sks"][p] - world["sks"][p + WAVE]) % o.R))
    finally:
        c.set_rng_seed(0)
    return out


def _route(world, route):
    """The route's device values over all of EDGE_WORDS, computed once: {"terms": per word (values,
    base, exponent factor), "got": per value position final_exp(prod_e v_e^(e + 1))}."""
    from oracle import bls12381 as o  # checker only
    if route not in world["routes"]:
        terms = (_prepare_route(world, route) if route <= 3 else
                 _uniform_route(world) if route == 4 else _partial_route(world, route))
        assert len(terms) == len(EDGE_WORDS)  # no word skipped
        got = []
        for pos in range(len(terms[0][0])):
            prod = o.F12_ONE
            for e, (vals, _, _) in enumerate(terms):
                prod = o.f12_mul(prod, o.f12_pow(vals[pos], e + 1))
            got.append(o.final_exp(prod))
        world["routes"][route] = {"terms": terms, "got": got}
    return world["routes"][route]


def _base(world, base):
    return world["gt"] if base == "m" else _gt_root(world, base)


def _expected(world, terms, words=EDGE_WORDS):
    """prod_e base_e^((e + 1) r_e factor_e), one power per distinct base."""
    from oracle import bls12381 as o  # checker only
    exps = {}
    for e, ((_, base, factor), k) in enumerate(zip(terms, words)):
        exps[base] = (exps.get(base, 0) + (e + 1) * glv_scalar(k) * factor) % o.R
    want = o.F12_ONE
    for base, a in sorted(exps.items(), key=lambda t: str(t[0])):
        want = o.f12_mul(want, o.f12_pow(_base(world, base), a))
    return want


def _offenders(world, terms, pos, invert):
    """The words whose own value is wrong (one final exponentiation each; only after a failure)."""
    from oracle import bls12381 as o  # checker only
    bad = []
    for (vals, base, factor), k in zip(terms, EDGE_WORDS):
        want = o.f12_pow(_base(world, base), glv_scalar(k) * factor % o.R)
        if o.final_exp(vals[pos]) != (o.f12_inv(want) if invert else want):
            bad.append(hex(k))
    return bad


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_edge_words(world, route):
    from oracle import bls12381 as o  # checker only
    r = _route(world, route)
    want = _expected(world, r["terms"])
    # route 4 returns two values per word: the pubkey-sum pair and the signature pair, its inverse
    for pos, got in enumerate(r["got"]):
        w = o.f12_inv(want) if pos == 1 else want
        if got != w:
            bad = _offenders(world, r["terms"], pos, pos == 1)
            pytest.fail("route %d (%s)%s: wrong for the words %s" % (
                route, ROUTES[route], ", signature pair" if pos == 1 else "", ", ".join(bad) or "(none singly)"))


@pytest.mark.parametrize("route", [2, 4, 5], ids=["r-pk", "bulk-r-sig", "latency-r-sig"])
def test_weighted_comparison_can_fail(world, route):
    """Negative control, one per family of route: with one word's expected exponent swapped for
    that of k ^ 1 the route's comparison must be unequal."""
    from oracle import bls12381 as o  # checker only
    r = _route(world, route)
    j = len(EDGE_WORDS) // 2
    words = list(EDGE_WORDS)
    words[j] ^= 1
    wrong = _expected(world, r["terms"], words)
    assert r["got"][0] != wrong
    if len(r["got"]) > 1:
        assert r["got"][1] != o.f12_inv(wrong)
