"""Device-side balance-weighted sampling under Electra's rule on a CPU: bgv_sample.h's 16-bit item
functions, the ordered compaction and the pass loop run by tests/native/samplesim_electra.cpp as
the kernels run them, against the spec-pseudocode hashlib model of tests/samplesim_electra.py.
Every case also runs in the simulator's address/undefined sanitizer build (a stand-alone program)."""
import hashlib

import pytest

from tests import samplesim as M8
from tests import samplesim_electra as M

KINDS = ["O2", "san"]
PROPOSER_SIZES = [1, 2, 257, 513]
SYNC_CASES = [(40, 64, "full"), (300, 64, "min"), (2049, 512, "mixed"), (2049, 128, "min"), (1, 8, "min"),
              (300, 64, "high")]
# (seed, eff, max_incr, accepted): candidate 0 draws 0xFFFF under EDGE_FFFF and 0 under EDGE_0000
EDGE_CASES = [(M.EDGE_FFFF, 2048, 2048, True), (M.EDGE_FFFF, 2047, 2048, False), (M.EDGE_FFFF, 65535, 65535, True),
              (M.EDGE_FFFF, 65534, 65535, False), (M.EDGE_0000, 0, 2048, True)]
EDGE_IDS = ["ffff-2048of2048", "ffff-2047of2048", "ffff-65535of65535", "ffff-65534of65535", "0000-0of2048"]


def n_eff_of(n):
    return M.active(n)[-1] + 1


@pytest.fixture(scope="module")
def proposer_model():
    seeds = M.slot_seeds()
    return {(name, n): [M.proposer(s, M.active(n), M.table(name, n_eff_of(n))) for s in seeds]
            for name in M.TABLES for n in PROPOSER_SIZES}


@pytest.fixture(scope="module")
def sync_model():
    return {(n, size, name): M.sync_committee(M.SEED, M.active(n), M.table(name, n_eff_of(n)), size)
            for n, size, name in SYNC_CASES}


def zero_draws():
    """Candidates among the first 65,536 of SEED that draw 0: 4,096 digests, no shuffle."""
    return [i for i in range(M.MAX_TRIES) if M.rand16(M.SEED, i) == 0]


def test_model_facts(proposer_model, sync_model):
    """What the fixed inputs exercise, as the model sees them."""
    pm = proposer_model
    assert all(tries == 1 for n in PROPOSER_SIZES for _, tries in pm["full", n])
    assert [v for v, _ in pm["mixed", 1]] == [None] * 32
    assert [v for v, _ in pm["min", 1]] == [None] * 32
    assert [v for v, _ in pm["min", 2]] == [None] * 32
    t257 = [t for _, t in pm["min", 257]]
    assert sum(v is None for v, _ in pm["min", 257]) == 2
    assert sum(t > 16 for t in t257) == 27  # past the first digest of draws
    assert sum(t > 256 for t in t257) == 2 and max(t257) == 257
    t513 = [t for _, t in pm["min", 513]]
    assert sum(v is None for v, _ in pm["min", 513]) == 0
    assert sum(t > 16 for t in t513) == 27
    assert sum(t > 256 for t in t513) == 2 and max(t513) == 346  # two seeds enter a second pass
    assert sum(v is None for v, _ in pm["high", 1]) == 29
    assert sum(v is None for v, _ in pm["high", 2]) == 20
    assert max(t for _, t in pm["high", 257]) == 7
    assert max(t for _, t in pm["high", 513]) == 10
    facts = {(40, 64, "full"): (64, 40), (300, 64, "min"): (4134, 58), (2049, 512, "mixed"): (637, 512),
             (2049, 128, "min"): (8330, 123), (1, 8, "min"): (593, 1), (300, 64, "high"): (104, 64)}
    for case, (tries, distinct) in facts.items():
        idx, t = sync_model[case]
        assert (t, len(set(idx))) == (tries, distinct), case
    # the edge seeds and the 32-bit edge of the products
    assert M.EDGE_FFFF == hashlib.sha256(b"edge16" + (15322).to_bytes(4, "little")).digest()
    assert M.EDGE_0000 == hashlib.sha256(b"edge16" + (52444).to_bytes(4, "little")).digest()
    assert hashlib.sha256(M.EDGE_FFFF + bytes(8)).digest()[:2] == b"\xff\xff" and M.rand16(M.EDGE_FFFF, 0) == 0xFFFF
    assert hashlib.sha256(M.EDGE_0000 + bytes(8)).digest()[:2] == b"\x00\x00" and M.rand16(M.EDGE_0000, 0) == 0
    assert 65535 * 65535 == 4294836225 < 2 ** 32
    for seed, eff, max_incr, ok in EDGE_CASES:
        assert (M.proposer(seed, [0], [eff], max_incr)[0] == 0) == ok, (eff, max_incr)
    # the cap: all-zero balances accept exactly 2 of the first 65,536 candidates
    assert len(zero_draws()) == 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(M.TABLES))
def test_proposers(kind, name, proposer_model):
    seeds = M.slot_seeds()
    for n in PROPOSER_SIZES:
        want = proposer_model[name, n]
        got = M.sim_sample(seeds, M.active(n), M.table(name, n_eff_of(n)), 1, True, kind=kind)
        assert [(p[0] if have else None) for have, _, p in got["seeds"]] == [v for v, _ in want], (name, n)
        limit = min(n, M.MAX_TRIES)  # the proposer bound
        # a seed is in every pass until it has its pick or the bound is reached
        tries = [t for _, t in want]
        passes = M.model_passes(1, limit, max(tries), len(seeds))
        assert [(w, c) for w, c, _ in got["passes"]] == passes, (name, n)
        base = 0
        for (w, c, k) in got["passes"]:
            assert k == sum(t > base for t in tries)
            base += c
        for (have, nxt, _), (v, t) in zip(got["seeds"], want):
            assert have == (v is not None) and t <= nxt <= limit
    if name == "min":  # n = 513: the two seeds past candidate 256 make the second pass
        assert got["passes"] == [(256, 256, 32), (512, 257, 2)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,size,name", SYNC_CASES)
def test_sync_committee(kind, n, size, name, sync_model):
    want, tries = sync_model[n, size, name]
    got = M.sim_sample([M.SEED], M.active(n), M.table(name, n_eff_of(n)), size, False, kind=kind)
    have, nxt, picks = got["seeds"][0]
    assert have == size and picks == want
    assert [(w, c) for w, c, _ in got["passes"]] == M.model_passes(size, M.MAX_TRIES, tries)
    assert nxt == sum(c for _, c, _ in got["passes"]) >= tries


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed,eff,max_incr,ok", EDGE_CASES, ids=EDGE_IDS)
def test_edge_draws(kind, seed, eff, max_incr, ok):
    """Draws of 0xFFFF and 0 on one active index: equality accepts, one below rejects, and
    65535 * 65535 on both sides stays within 32 bits."""
    got = M.sim_sample([seed], [0], [eff], 1, True, max_incr=max_incr, kind=kind)
    assert got["seeds"] == ([(1, 1, [0])] if ok else [(0, 1, [])])
    assert got["passes"] == [(256, 1, 1)]


@pytest.mark.parametrize("kind", KINDS)
def test_cap(kind):
    """All-zero balances: a candidate is accepted only on a draw of 0, two of the first 65,536, so
    the cap ends the run of a committee of 8 with two members, and a proposer run ends at the
    list's end."""
    n = 5
    act, eff = M.active(n), [0] * n_eff_of(n)
    zero = zero_draws()
    got = M.sim_sample([M.SEED], act, eff, 8, False, rounds=2, kind=kind)
    have, nxt, picks = got["seeds"][0]
    assert (have, nxt) == (2, M.MAX_TRIES) == (len(zero), 65536)
    assert sum(c for _, c, _ in got["passes"]) == M.MAX_TRIES
    assert [(w, c) for w, c, _ in got["passes"]] == M.model_passes(8, M.MAX_TRIES, M.MAX_TRIES)
    assert picks == [act[M.S.compute_shuffled_index(i % n, n, M.SEED, 2)] for i in zero]
    # size 2 is what the cap leaves
    want, tries = M.sync_committee(M.SEED, act, eff, 2, rounds=2)
    assert want == picks and tries == zero[1] + 1
    # proposers stop at the list's end
    seeds = M.slot_seeds()[:3]
    got = M.sim_sample(seeds, act, eff, 1, True, rounds=2, kind=kind)
    assert [(p[0] if have else None) for have, _, p in got["seeds"]] == \
        [M.proposer(s, act, eff, rounds=2)[0] for s in seeds]
    assert [x[1] for x in got["seeds"]] == [n] * 3 and [(w, c) for w, c, _ in got["passes"]] == [(256, 5)]


@pytest.mark.parametrize("kind", KINDS)
def test_rule_differs_from_the_byte_rule(kind):
    """The same inputs under both rules give different committees, so the 16-bit entry points
    cannot be the byte rule's kernel under another name."""
    n, size = 300, 64
    act, eff = M.active(n), [1 + v % 4 for v in range(n_eff_of(n))]
    new = M.sync_committee(M.SEED, act, eff, size, max_incr=32)[0]
    old = M8.sync_committee(M.SEED, act, bytes(eff), size, max_incr=32)[0]
    assert new != old
    assert M.sim_sample([M.SEED], act, eff, size, False, max_incr=32, kind=kind)["seeds"][0][2] == new
    assert M8.sim_sample([M.SEED], act, bytes(eff), size, False, max_incr=32, kind=kind)["seeds"][0][2] == old


def test_mainnet_passes_pinned():
    """The plan of the mainnet shape quoted in DESIGN.md is the unchanged planner's, and with every
    balance at 32 of 2048 the 512th acceptance under SEED is where the model says (the draws
    alone decide it: no shuffle)."""
    ok = [i for i in range(M.MAINNET_SYNC_TRIES) if M.accepted(32, 2048, M.rand16(M.SEED, i))]
    assert len(ok) == 512 and ok[-1] + 1 == M.MAINNET_SYNC_TRIES
    passes = [(w, c) for w, c, _ in M.MAINNET_SYNC_PASSES]
    assert passes == M8.sim_plan(512, M.MAX_TRIES, 1)[:len(passes)]
