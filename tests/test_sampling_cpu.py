"""Device-side balance-weighted sampling on a CPU: bgv_sample.h (the per-candidate evaluation,
the ordered compaction, the pass loop and its planning) run by tests/native/samplesim.cpp as the
kernels run it, against the spec-pseudocode hashlib model of tests/samplesim.py.  Every case also
runs in the simulator's address/undefined sanitizer build (a stand-alone program)."""
import pytest

from tests import samplesim as M

KINDS = ["O2", "san"]
PROPOSER_SIZES = [1, 2, 257, 513]
SYNC_CASES = [(40, 64, "full"), (300, 64, "low"), (2049, 512, "mixed"), (2049, 512, "low"), (1, 8, "low")]


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


def test_model_facts(proposer_model, sync_model):
    """What the fixed inputs exercise, as the model sees them."""
    pm = proposer_model
    assert all(tries == 1 for n in PROPOSER_SIZES for _, tries in pm["full", n])
    assert [v for v, _ in pm["mixed", 1]] == [None] * 32
    assert sum(v is None for v, _ in pm["low", 2]) == 30
    low = [t for _, t in pm["low", 257]]
    assert sum(t > 32 for t in low) == 5 and max(low) - 1 == 39  # the longest goes to candidate number 39
    one = [t for _, t in pm["one", 257]]
    assert sum(t > 32 for t in one) == 17 and max(one) - 1 == 199  # the longest goes to candidate number 199
    assert all(v is not None for v, _ in pm["one", 257])
    sm = sync_model
    idx, tries = sm[40, 64, "full"]
    assert tries == 64 and len(set(idx)) == 40
    assert sm[300, 64, "low"][1] == 804
    assert sm[2049, 512, "mixed"][1] == 722
    idx, tries = sm[2049, 512, "low"]
    assert tries == 6342 and len(set(idx)) == 454
    assert sm[1, 8, "low"][1] == 140


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
def test_cap(kind):
    """All-zero balances: a candidate is accepted only on a random byte of 0, one in 256, so the
    cap of 65,536 candidates ends the run before a committee of 512 is full, and a proposer run
    ends at the list's end."""
    n = 5
    act, eff = M.active(n), bytes(n_eff_of(n))
    zero = sum(M.hashlib.sha256(M.SEED + q.to_bytes(8, "little")).digest().count(0) for q in range(M.MAX_TRIES // 32))
    assert 8 < zero < 512
    got = M.sim_sample([M.SEED], act, eff, 512, False, rounds=2, kind=kind)
    have, nxt, picks = got["seeds"][0]
    assert (have, nxt) == (zero, M.MAX_TRIES)
    assert sum(c for _, c, _ in got["passes"]) == M.MAX_TRIES
    assert picks == M.sync_committee(M.SEED, act, eff, zero, rounds=2)[0]
    # size 8 is reached long before the cap
    want, tries = M.sync_committee(M.SEED, act, eff, 8, rounds=2)
    got = M.sim_sample([M.SEED], act, eff, 8, False, rounds=2, kind=kind)
    assert got["seeds"][0][0] == 8 and got["seeds"][0][2] == want and tries < M.MAX_TRIES
    # proposers stop at the list's end
    seeds = M.slot_seeds()[:3]
    got = M.sim_sample(seeds, act, eff, 1, True, rounds=2, kind=kind)
    assert [(p[0] if have else None) for have, _, p in got["seeds"]] == \
        [M.proposer(s, act, eff, rounds=2)[0] for s in seeds]
    assert [x[1] for x in got["seeds"]] == [n] * 3 and [(w, c) for w, c, _ in got["passes"]] == [(256, 5)]


@pytest.mark.parametrize("kind", KINDS)
def test_pass_planning(kind):
    cap = M.MAX_TRIES
    # a proposer: 256, then twice the last window, the rest of the cap at the end
    assert M.sim_plan(1, cap, 1, kind) == [(256 << k, 256 << k) for k in range(8)] + [(256, 256)]
    # a mainnet sync committee: max(256, 2 * 512) first
    assert M.sim_plan(512, cap, 1, kind) == [(1024 << k, 1024 << k) for k in range(6)] + [(1024, 1024)]
    # windows are whole blocks of 256 and the last one stops at the limit
    assert M.sim_plan(1, 257, 32, kind) == [(256, 256), (256, 1)]
    assert M.sim_plan(300, 1000, 1, kind) == [(768, 768), (256, 232)]
    # 1024 seeds: a pass never examines more than 2^22 candidates
    assert M.sim_plan(1, cap, 1024, kind) == \
        [(256 << k, 256 << k) for k in range(5)] + [(4096, 4096)] * 14 + [(256, 256)]
    for want, limit, k in [(1, cap, 1), (512, cap, 1), (1, 257, 32), (65536, cap, 1), (7, 4000, 1024)]:
        plan = M.sim_plan(want, limit, k, kind)
        assert plan == M.model_passes(want, limit, limit, k)
        assert sum(c for _, c in plan) == limit
