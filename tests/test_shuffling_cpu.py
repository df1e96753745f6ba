"""Device-side epoch shuffling on a CPU: bgv_shuffle.h (the table, the walk, the committee
bounds) run by tests/native/shufflesim.cpp as the kernels run it, against the reference's
unshuffleList vectors, a spec-pseudocode hashlib model and computeEpochShuffling's slices.
Every case also runs in the simulator's address/undefined sanitizer build."""
import hashlib
import itertools

import pytest

from tests import shufflesim as S

KINDS = ["O2", "san"]
SEEDS = [bytes([42, 32]) + bytes(30), hashlib.sha256(b"lodestar-amd epoch shuffling").digest()]
SIZES = [1, 2, 3, 255, 256, 257, 513, 2049]
ROUNDS = [0, 10, 90]
BOUNDS = [(2049, 32, 2), (20, 8, 4), (64, 8, 8), (1, 8, 1)]


def lists(n):
    return {"identity": list(range(n)), "gapped": S.gapped(n), "reversed": list(range(n - 1, -1, -1))}


@pytest.fixture(scope="module")
def parity_cases():
    cases = [(seed, rounds, lst) for n, rounds, seed in itertools.product(SIZES, ROUNDS, SEEDS)
             for lst in lists(n).values()]
    return cases, [S.model_shuffle(*c) for c in cases]


@pytest.mark.parametrize("kind", KINDS)
def test_kat_unshuffle_list(kind):
    vecs = S.fixture()["unshuffle"]
    assert len(vecs) == 2
    got = S.sim_shuffle([(bytes.fromhex(v["seed"]), v["rounds"], v["input"]) for v in vecs], kind)
    for v, g in zip(vecs, got):
        assert g == v["res"], v["id"]


def test_model_reproduces_kat():
    for v in S.fixture()["unshuffle"]:
        assert S.model_shuffle(bytes.fromhex(v["seed"]), v["rounds"], v["input"]) == v["res"]


@pytest.mark.parametrize("kind", KINDS)
def test_model_parity(kind, parity_cases):
    cases, want = parity_cases
    got = S.sim_shuffle(cases, kind)
    assert len(got) == len(want) == len(SIZES) * len(ROUNDS) * len(SEEDS) * 3
    for (seed, rounds, lst), g, w in zip(cases, got, want):
        assert g == w, (len(lst), rounds, seed.hex()[:8])
        assert sorted(g) == sorted(lst)
        if rounds == 0 or len(lst) == 1:
            assert g == lst  # the list stays as it is


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,slots,cps", BOUNDS)
def test_committee_bounds(kind, n, slots, cps):
    count = slots * cps
    want = S.model_committees(n, slots, cps)
    lines = [ln.split() for ln in S.run("bounds %d %d %d\n" % (n, slots, cps), kind)]
    com = [(int(k), int(lo), int(hi)) for op, k, lo, hi in (ln for ln in lines if ln[0] == "com")]
    assert [k for k, _, _ in com] == list(range(count))
    assert [(lo, hi) for _, lo, hi in com] == want
    # the slices concatenate to the shuffling
    shuffled = S.model_shuffle(SEEDS[0], 10, S.gapped(n))
    assert [v for lo, hi in want for v in shuffled[lo:hi]] == shuffled
    # empty committees exactly where n < count predicts
    empty = [k for k, lo, hi in com if lo == hi]
    assert bool(empty) == (n < count) and len(empty) == max(0, count - n)
    # the directory kernel's view: the j-th non-empty committee
    dirs = [tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] == "dir"]
    nonempty = [(k, lo, hi) for k, lo, hi in com if hi > lo]
    assert dirs == [(j, k, lo, hi) for j, (k, lo, hi) in enumerate(nonempty)]
    assert lines[-1] == ["longest", str(max(hi - lo for lo, hi in want)), "nonempty", str(len(nonempty))]
