"""The call layout and the retry planner (bgv_host_layout.h, bgv_retry_plan.h) on the CPU.

tests/native/retrysim.cpp drives the library's own layout function and CallPlan through the
first pass and the retry rounds, with the verdict words from a model of the closing kernels.
Every scenario's per-job codes must be the truth (1 valid, 0 invalid, the negative BLST code
where the reference rejects), in an optimized build and in one under ASan + UBSan; the rounds,
the groups per round and the digests of the bgv_dgroup records are pinned by
tests/golden/retry_plans.json (every deterministic scenario, the first 50 of each random family).

    python tests/test_retry_plan.py --write-golden      rewrites the golden file
"""
import itertools
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import retrysim as rs  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retry_plans.json")
GOLDEN_RANDOM = 50  # of each random family


def _subset_name(n, bad):
    return "n%d:" % n + ".".join(str(i) for i in bad)


def family_one_group():
    """One group of n one-set batchable jobs: every invalid subset for n <= 8, every subset of
    size 1 and 2 for n = 37 and 64."""
    out = []
    for n in (2, 3, 5, 8):
        for k in range(n + 1):
            for bad in itertools.combinations(range(n), k):
                out.append(rs.one_set_jobs(_subset_name(n, bad), n, bad, seed=n))
    for n in (37, 64):
        for k in (0, 1, 2):
            for bad in itertools.combinations(range(n), k):
                out.append(rs.one_set_jobs(_subset_name(n, bad), n, bad, seed=n))
    return out


def family_one_group_random():
    """500 seeded random subsets of sizes 3..n (n = 37 and 64 in turn), with all-invalid."""
    rnd = random.Random(0x5EED01)
    out = []
    for q in range(500):
        n = (37, 64)[q % 2]
        k = n if q < 2 else rnd.randint(3, n)
        bad = sorted(rnd.sample(range(n), k))
        out.append(rs.one_set_jobs("rand%d-" % q + _subset_name(n, bad), n, bad, seed=1000 + q))
    return out


def _sized_jobs(name, sizes, bad_sets, **kw):
    """Batchable jobs of the given set counts, every set its own root; bad_sets: wrong sets."""
    n = sum(sizes)
    return rs.scenario(name, [(s, True) for s in sizes], [(i, rs.WRONG if i in bad_sets else rs.VALID, 0) for i in range(n)],
                       **kw)


def family_spanning():
    """Several groups, and jobs of 1-3 sets where some straddle a 64-slot boundary (the shapes of
    tests/test_gpu_retry.py)."""
    out = [rs.one_set_jobs("multi130", 130, [3, 70, 129], seed=130),
           rs.one_set_jobs("multi200", 200, [64, 65, 127, 128, 199], seed=200)]
    sizes = [1 + (i % 3) for i in range(70)]
    last = list(itertools.accumulate(sizes))  # one past each job's last set
    out.append(_sized_jobs("span70", sizes, {last[j] - 1 for j in (4, 21, 22, 40, 69)}, seed=70))
    return out


def family_spanning_random():
    rnd = random.Random(0x5EED02)
    out = []
    for q in range(200):
        sizes = [rnd.randint(1, 3) for _ in range(rnd.randint(40, 100))]
        first = [0] + list(itertools.accumulate(sizes))
        bad = {first[j] + rnd.randrange(sizes[j]) for j in rnd.sample(range(len(sizes)), rnd.randint(1, 6))}
        out.append(_sized_jobs("spanrand%d" % q, sizes, bad, seed=2000 + q))
    return out


def _uniform(name, counts, kinds, **kw):
    """One-set batchable jobs over len(counts) roots, counts[r] jobs of root r, dealt round robin
    (so roots recur and the layout groups them).  kinds: {(root, k): (kind, code) or "own-root"}
    for the k-th job of a root; "own-root" is a wrong message: the set gets a root of its own."""
    left, sets, seen = list(counts), [], [0] * len(counts)
    while any(left):
        for r in range(len(counts)):
            if not left[r]:
                continue
            left[r] -= 1
            what = kinds.get((r, seen[r]), (rs.VALID, 0))
            if what == "own-root":
                sets.append((10000 + len(sets), rs.WRONG, 0))
            else:
                sets.append((r, what[0], what[1]))
            seen[r] += 1
    return rs.scenario(name, [(1, True)] * len(sets), sets, uniform=True, layout=True, **kw)


COMMITTEES_17 = [64] * 17
COMMITTEE_127 = [127] + [64] * 15 + [1]  # 1,088 jobs again; the last root is a lone job
W, DEAD = (rs.WRONG, 0), (rs.UNDECODABLE, rs.BLST_BAD_ENCODING)


def family_uniform():
    """Bulk-uniform batches: 1,088 one-set jobs over 17 roots of 64, and a 127-job committee."""
    out = [_uniform("u17-valid", COMMITTEES_17, {}), _uniform("u127-valid", COMMITTEE_127, {})]
    for g in (0, 8, 16):
        for k in (0, 31, 63):
            out.append(_uniform("u17-one-g%d-s%d" % (g, k), COMMITTEES_17, {(g, k): W}, seed=17 * g + k))
    for k in (0, 31, 63):
        out.append(_uniform("u17-each-s%d" % k, COMMITTEES_17, {(g, k): W for g in range(17)}, seed=k))
    out.append(_uniform("u17-beside-dead", COMMITTEES_17, {(3, 10): DEAD, (3, 11): W}))
    out.append(_uniform("u17-beside-dead-first", COMMITTEES_17, {(5, 0): DEAD, (5, 1): W}))
    out.append(_uniform("u17-beside-dead-last", COMMITTEES_17, {(5, 62): W, (5, 63): DEAD}))
    out.append(_uniform("u17-two", COMMITTEES_17, {(2, 5): W, (2, 6): W}))
    out.append(_uniform("u17-two-apart", COMMITTEES_17, {(2, 0): W, (2, 63): W}))
    out.append(_uniform("u17-three", COMMITTEES_17, {(9, 0): W, (9, 17): W, (9, 33): W}))
    out.append(_uniform("u17-two-groups", COMMITTEES_17, {(1, 7): W, (1, 40): W, (12, 63): W}))
    out.append(_uniform("u17-wrong-message", COMMITTEES_17, {(4, 20): "own-root"}))
    out.append(_uniform("u17-wrong-message-and-key", COMMITTEES_17, {(4, 20): "own-root", (4, 21): W, (6, 0): W}))
    for k in (0, 63, 64, 126):
        out.append(_uniform("u127-one-s%d" % k, COMMITTEE_127, {(0, k): W}, seed=k))
    out.append(_uniform("u127-two", COMMITTEE_127, {(0, 63): W, (0, 64): W}))
    out.append(_uniform("u127-three-one-group", COMMITTEE_127, {(0, 70): W, (0, 71): W, (0, 126): W}))
    out.append(_uniform("u127-lone-root-wrong", COMMITTEE_127, {(16, 0): W}))
    out.append(_uniform("u127-wrong-message", COMMITTEE_127, {(0, 100): "own-root"}))
    return out


def family_precheck():
    """An undecodable signature and an infinity pubkey, in 1-set and 2-set jobs, inside a
    failing group: small (every job alone), pattern-tested and fanned-out units; batchable and
    not; both modes."""
    und, grp, ipk, isig = (rs.UNDECODABLE, rs.BLST_BAD_ENCODING), (rs.UNDECODABLE, rs.BLST_POINT_NOT_IN_GROUP), \
        (rs.INF_PK, 0), (rs.INF_SIG, 0)
    ok, bad = (rs.VALID, 0), (rs.WRONG, 0)
    special = [[und], [ipk], [isig], [und, ok], [ok, grp], [und, bad], [bad, und], [ipk, ok], [ok, ipk], [ipk, bad],
               [und, ipk], [ipk, und], [grp, und], [isig, ok]]
    out = []
    for fill in (0, 2, 20, 50):  # with the special jobs: a small unit, one group, two groups
        for batchable in (True, False):
            for mode in (0, 1):
                jobs, sets = [], []
                for q in range(fill):
                    jobs.append([bad if q in (1, fill - 1) else ok])
                    if q % 4 == 0:
                        jobs.append(special[(q // 4) % len(special)])
                jobs += special
                flat = [(i, k[0], k[1]) for i, k in enumerate(k for j in jobs for k in j)]
                out.append(rs.scenario("pre-f%d-b%d-m%d" % (fill, batchable, mode), [(len(j), batchable) for j in jobs],
                                       flat, mode=mode, seed=fill))
    return out


FAMILIES = [("one_group", family_one_group, None), ("one_group_random", family_one_group_random, GOLDEN_RANDOM),
            ("spanning", family_spanning, None), ("spanning_random", family_spanning_random, GOLDEN_RANDOM),
            ("uniform", family_uniform, None), ("precheck", family_precheck, None)]


@pytest.fixture(scope="module")
def results():
    """Every family through both builds, once: {family: (scenarios, O2 results, sanitizer results)}."""
    out = {}
    for name, make, _ in FAMILIES:
        sc = make()
        out[name] = (sc, rs.run(sc, "O2"), rs.run(sc, "san"))
    return out


@pytest.mark.parametrize("family", [f[0] for f in FAMILIES])
def test_codes_are_the_truth(results, family):
    sc, fast, san = results[family]
    assert len({s["name"] for s in sc}) == len(sc)
    for s, a, b in zip(sc, fast, san):
        assert a["codes"] == rs.truth(s), s["name"]
        assert a == b, s["name"]  # the sanitizer build decides the same, record for record
        assert a["rounds"] == len(a["groups"]) <= 4, s["name"]
        assert a["sets_verified"] == len(s["sets"])


@pytest.mark.parametrize("family", [f[0] for f in FAMILIES])
def test_plans_match_golden(results, family):
    golden = json.load(open(GOLDEN))[family]
    sc, fast, _ = results[family]
    keep = dict(zip((f[0] for f in FAMILIES), (f[2] for f in FAMILIES)))[family]
    got = [rs.plan_record(r) for r in fast[:keep]]  # the golden lists follow the family's order
    assert len(got) == len(golden)
    assert {s["name"]: (g, w) for s, g, w in zip(sc, got, golden) if g != w} == {}


def test_rounds_of_one_failing_group(results):
    """One invalid job costs one pattern round of ceil(log2 n) tests; two cost a second round."""
    by = {s["name"]: r for s, r in zip(*results["one_group"][:2])}
    assert by["n64:5"]["groups"] == [6]
    assert by["n37:36"]["groups"] == [6]
    assert by["n64:5.6"]["rounds"] == 2 and by["n64:5.6"]["groups"][0] == 6
    assert by["n64:"]["rounds"] == 0 and by["n64:"]["batch_retries"] == 0
    assert by["n64:5"]["batch_retries"] == 1 and by["n64:5"]["device_groups"] == 1 + 6


def test_weighted_test_names_a_lone_invalid_slot(results):
    """A failing uniform group with one invalid slot is settled by ONE test in one round."""
    by = {s["name"]: r for s, r in zip(*results["uniform"][:2])}
    for name in ("u17-one-g0-s0", "u17-one-g8-s31", "u17-one-g16-s63", "u127-one-s64", "u17-beside-dead"):
        assert by[name]["groups"] == [1], name
    assert by["u17-each-s31"]["groups"] == [17]
    assert by["u17-two"]["rounds"] >= 2  # the weighted test finds no lone slot: pattern tests follow


def _layout_groups(res):
    """(first_slot, n_slots, shared, uniform, roots of its slots) per first-pass group"""
    return [(f, n, sh, un, res["slot_root"][f:f + n]) for f, n, sh, un in res["layout_groups"]]


def test_root_aligned_layout(results):
    """DESIGN's layout properties: a root with >= 32 jobs starts a group, a 127-set committee
    fills 64 + 63 slots, uniq holds one slot per distinct root."""
    for s, res in zip(*results["uniform"][:2]):
        name = s["name"]
        count = {}
        for root, _, _ in s["sets"]:
            count[root] = count.get(root, 0) + 1
        groups = _layout_groups(res)
        assert res["nslots"] % 64 == 0 and all(f % 64 == 0 and 1 <= n <= 64 for f, n, _, _, _ in groups), name
        started = {}
        for f, n, shared, uniform, roots in groups:
            assert -1 not in roots, name  # pads lie outside the groups
            assert bool(uniform) == (len(set(roots)) == 1), name
            for k, r in enumerate(roots):
                started.setdefault(r, (f, k))
        for r, c in count.items():
            if c >= 32:  # its first job opens a group, and its groups hold nothing else
                assert started[r][1] == 0, (name, r)
                mine = [g for g in groups if r in g[4]]
                assert all(set(g[4]) == {r} for g in mine), (name, r)
                assert [g[1] for g in mine] == [64] * (c // 64) + ([c % 64] if c % 64 else []), (name, r)
        # one hashed slot per distinct root, and every slot uses the hash of its own root
        assert sorted(res["slot_root"][u] for u in res["uniq"]) == sorted(count), name
        assert res["hsrc_root"] == res["slot_root"], name
    by = {s["name"]: r for s, r in zip(*results["uniform"][:2])}
    assert [g[1] for g in _layout_groups(by["u127-valid"]) if 0 in g[4]] == [64, 63]
    assert len(by["u17-valid"]["layout_groups"]) == 17
    # a corrupted message leaves its committee one short: still its own group, of 63
    short = [g for g in _layout_groups(by["u17-wrong-message"]) if 4 in g[4]]
    assert [(g[1], g[3]) for g in short] == [(63, 1)]


def test_root_index_key_collision():
    """Two roots with the same first 8 bytes (the index's key): each slot still uses the hash of
    its own root; the second root is hashed again where it recurs apart (one extra hash, no more)."""
    a, b = 7, 7 + (1 << 32)  # retrysim: roots 2^32 apart share their first 8 bytes
    sets = [(r, rs.VALID, 0) for r in (a, b, a, b, b, 9)]
    for kind in ("O2", "san"):
        res = rs.run([rs.scenario("collide", [(1, True)] * len(sets), sets, layout=True)], kind)[0]
        assert res["hsrc_root"][:6] == res["slot_root"][:6] == [a, b, a, b, b, 9]
        assert res["uniq"] == [0, 1, 3, 5]
        assert res["codes"] == [1] * 6


def test_fast_layout_equals_builder():
    """layout_one_job_fast against Builder on one 2^17-set job, record by record."""
    for kind in ("O2", "san"):
        res = rs.run([{"name": "fast", "op": "fast_layout", "n": 1 << 17}], kind)[0]
        assert res["fast"] is True and res["differ"] == 0, (kind, res)
        assert res["nslots"] == 1 << 17 and res["ngroups"] == 2048


if __name__ == "__main__" and sys.argv[1:] == ["--write-golden"]:
    gold = {}
    for fam, make, keep in FAMILIES:
        sc = make()[:keep]
        gold[fam] = [rs.plan_record(r) for r in rs.run(sc, "O2")]
    with open(GOLDEN, "w") as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
