"""CPU checks of tests/merged_calls.py, the helper of tests/test_gpu_merged_calls.py: the
comparison that reports a merged super-batch's failures can fail, and names exactly what differs;
the submission orders put every kind of call first once."""
from tests import merged_calls as mc


def _cases():
    return [mc.MergedCall("a", "jobs", [1, 0, 1]), mc.MergedCall("b", "jobs", [1, 1], labels=["x", "y"]),
            mc.MergedCall("c", "jobs", [-1, 1]), mc.MergedCall("d", "partial", [0, 0, 1],
                                                               labels=["sig_code", "pk_code", "verdict"])]


def _truth(cases):
    return {c.name: list(c.want) for c in cases}


def test_mismatches_passes_the_truth():
    cases = _cases()
    assert mc.mismatches(cases, _truth(cases)) == []


def test_mismatches_names_two_swapped_calls_and_no_other():
    """A verdict region read one call off: b's results at c's place and c's at b's."""
    cases = _cases()
    got = _truth(cases)
    got["b"], got["c"] = got["c"], got["b"]
    assert mc.mismatches(cases, got) == ["b:x", "c:0"]  # [-1, 1] against [1, 1] and the reverse
    got = _truth(cases)
    got["a"], got["d"] = got["d"], got["a"]
    assert mc.mismatches(cases, got) == ["a:0", "d:sig_code"]  # [0, 0, 1] against [1, 0, 1] and the reverse


def test_mismatches_names_one_changed_code_alone():
    cases = _cases()
    for call in cases:
        for j, label in enumerate(call.labels):
            got = _truth(cases)
            got[call.name][j] = 0 if got[call.name][j] != 0 else 1
            assert mc.mismatches(cases, got) == ["%s:%s" % (call.name, label)]


def test_mismatches_names_missing_and_surplus_results():
    cases = _cases()
    got = _truth(cases)
    del got["b"]
    got["c"] = got["c"][:1]
    got["a"] = got["a"] + [1]
    assert mc.mismatches(cases, got) == ["a:+1", "b:x", "b:y", "c:1"]


def test_rotation_puts_every_kind_first_once():
    kinds = ["singles", "records", "bits", "spans", "multikey"]
    rots = mc.all_rotations(kinds)
    assert sorted(r[0] for r in rots) == sorted(kinds)
    for r in rots:
        assert sorted(r) == sorted(kinds) and len(r) == len(kinds)
        k = kinds.index(r[0])
        assert r == kinds[k:] + kinds[:k]  # a rotation: the cyclic order is kept
    # the two orders a case runs: as listed and rotated by two, never the same call first
    listed, rotated = mc.rotations(kinds)
    assert listed == kinds and rotated == kinds[2:] + kinds[:2]
    assert mc.rotations(kinds, 2) == [rots[0], rots[2]]
    assert mc.rotations([]) == [[], []]


def test_sizes_and_thresholds_read_from_the_headers():
    th = mc.thresholds()
    assert th["PREP_WIDE_MAX"] < th["MILLER_WIDE_MAX"] < th["LATENCY_MAX"]
    assert th["PK_TREE_MIN"] <= th["PK_TEAM_MAX"]
    calls = [mc.MergedCall("a", "jobs", [1], groups=1), mc.MergedCall("b", "jobs", [1], groups=3)]
    assert mc.sizes(calls) == (256, 4, 260)
