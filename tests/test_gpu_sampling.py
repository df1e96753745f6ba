"""GPU tests of the device-side balance-weighted sampling (include/blsgpu.h bgv_proposers,
bgv_sync_committee_put): the proposers and sync committees read back from the device against the
spec-pseudocode hashlib model (tests/samplesim.py), the aggregate against bgv_aggregate_pubkeys of
the same list, and the committee a put leaves behind against the verdicts of the same sets given
as index lists.
"""
import functools
import hashlib

import pytest

from tests import samplesim as M
from tests.test_gpu_shuffling import NKEYS, World, _R, _sk, _sk_bytes, pack

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 257, 513]
SYNC_CASES = [(40, 64, "full"), (300, 64, "low"), (2049, 512, "mixed"), (2049, 512, "low"), (1, 8, "low")]


@functools.lru_cache(maxsize=None)
def eff(name, n_eff=NKEYS):
    return M.table(name, n_eff)


@functools.lru_cache(maxsize=None)
def model_sync(n, size, name):
    return M.sync_committee(M.SEED, M.active(n), eff(name), size)


def compress(rec96):
    """48-byte ZCash form of a 96-byte uncompressed G1 record"""
    from oracle import bls12381 as o  # the field modulus alone; never the code under test
    if rec96[0] & 0x40:
        return bytes([0xC0]) + bytes(47)
    y = int.from_bytes(rec96[48:], "big")
    return bytes([rec96[0] | 0x80 | (0x20 if y > (o.P - 1) // 2 else 0)]) + rec96[1:48]


def all_bits(n):
    return pack(range(n), n)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture(scope="module")
def repeats(world):
    """The (40, 64, full) committee, which holds repeats, under id 700; kept for the tests that read it."""
    idx, agg = world.ctx.sync_committee_put(700, M.SEED, M.active(40), eff("full"), 32, 64, 90)
    return 700, [int(v) for v in idx], agg


@pytest.mark.parametrize("name", list(M.TABLES))
def test_proposers_match_model(world, name):
    """32 slot seeds; n = 257 and 513 cross the 256-position hash block, `low` and `one` go past
    candidate 32 (the second random-byte digest), n = 1 and 2 end at the list's end."""
    seeds = M.slot_seeds()
    for n in SIZES:
        want = [M.proposer(s, M.active(n), eff(name))[0] for s in seeds]
        assert world.ctx.proposers(seeds, M.active(n), eff(name), 32, 90) == want, (name, n)
        if (name, n) == ("mixed", 1):
            assert want == [None] * 32
        if (name, n) == ("low", 2):
            assert want.count(None) == 30


@pytest.mark.parametrize("n,size,name", SYNC_CASES)
def test_sync_committee_matches_model(world, n, size, name):
    want, tries = model_sync(n, size, name)
    idx, agg = world.ctx.sync_committee_put(900, M.SEED, M.active(n), eff(name), 32, size, 90)
    try:
        assert [int(v) for v in idx] == want, tries
        rec = world.ctx.aggregate_pubkeys(want)
        assert agg == compress(rec)
        assert world.ctx.aggregate_committee_bits(900, all_bits(size), size) == rec
    finally:
        world.ctx.committee_drop(900)


def test_repeats_and_partial_bits(world, repeats):
    cid, idx, agg = repeats
    assert idx == model_sync(40, 64, "full")[0] and len(set(idx)) == 40
    assert agg == compress(world.ctx.aggregate_pubkeys(idx))
    pos = [p for p in range(64) if p % 3 != 1]
    assert world.ctx.aggregate_committee_bits(cid, pack(pos, 64), 64) == \
        world.ctx.aggregate_pubkeys([idx[p] for p in pos])


def test_verdicts(world, repeats):
    """A valid set with a partial bitfield and one with a flipped bit on the committee with
    repeats; the signature comes from the sum of the participants' secret keys, repeats counted;
    the index-list form decides the same."""
    native = world.native
    cid, idx, _ = repeats
    pos = [p for p in range(64) if p % 5 != 2]
    assert len(set(idx[p] for p in pos)) < len(pos)  # a participant counted twice
    msg = hashlib.sha256(b"sampled sync committee").digest()
    sig = world.ctx.sign(_sk_bytes(sum(world.sks[idx[p]] for p in pos) % _R()), msg)
    cj, ij = [], []
    for p in (pos, pos[1:]):
        cj.append(([native.SetSpec(msg, sig, committee=cid, bits=pack(p, 64), n_bits=64)], False))
        ij.append(([native.SetSpec(msg, sig, pk_indices=[idx[q] for q in p])], False))
    got = world.ctx.verify_jobs(cj)
    assert got == [1, 0]
    assert world.ctx.verify_jobs(ij) == got


def test_errors_and_atomicity(world):
    native, ctx = world.native, world.ctx
    cid, n, size = 1200, 300, 64
    act, bal = M.active(n), eff("low")
    put = ctx.sync_committee_put

    def gone():
        assert world.code_of(ctx.aggregate_committee_bits, cid, all_bits(size), size) == native.BGV_E_BAD_INDEX

    # All-zero balances: a candidate is accepted on a random byte of 0 only (0 * 255 >= 32 * 0),
    # about one in 256, so 65,536 candidates hold fewer than 512 acceptances: the cap, a bounded run.
    zero = sum(hashlib.sha256(M.SEED + q.to_bytes(8, "little")).digest().count(0) for q in range(2048))
    assert 8 <= zero < 512
    assert world.code_of(put, cid, M.SEED, act, bytes(NKEYS), 32, 512, 90) == native.BGV_E_ARG
    gone()
    # ... and a committee of 8 is what the reference's loop gives, long before the cap
    want8 = M.sync_committee(M.SEED, act, bytes(NKEYS), 8)[0]
    assert [int(v) for v in put(cid, M.SEED, act, bytes(NKEYS), 32, 8, 90)[0]] == want8
    ctx.committee_drop(cid)
    ctx.committee_put(cid, [1, 2, 3])  # a live id
    assert world.code_of(put, cid, M.SEED, act, bal, 32, size, 90) == native.BGV_E_ARG
    assert ctx.aggregate_committee_bits(cid, bytes([7]), 3) == ctx.aggregate_pubkeys([1, 2, 3])  # untouched
    ctx.committee_drop(cid)
    for bad in (dict(max_incr=0), dict(rounds=256), dict(active=act[:-1] + [NKEYS - 1], eff=bal[:NKEYS - 1])):
        a = dict(active=act, eff=bal, max_incr=32, rounds=90)
        a.update(bad)
        assert world.code_of(put, cid, M.SEED, a["active"], a["eff"], a["max_incr"], size, a["rounds"]) == \
            native.BGV_E_ARG
        gone()
    assert world.code_of(put, cid, M.SEED, act[:-1] + [NKEYS], bytes([32]) * (NKEYS + 1), 32, size, 90) == \
        native.BGV_E_BAD_INDEX
    gone()
    # the proposers' argument checks
    seeds = M.slot_seeds()[:2]
    for a in ((seeds, act, bal, 0, 90), (seeds, act, bal, 256, 90), (seeds, act, bal, 32, 256), ([], act, bal, 32, 90),
              (seeds, [], bal, 32, 90), (seeds, act[:-1] + [NKEYS], bal, 32, 90)):
        assert world.code_of(ctx.proposers, *a) == native.BGV_E_ARG
    # a following put on the id succeeds
    idx, agg = put(cid, M.SEED, act, bal, 32, size, 90)
    assert [int(v) for v in idx] == model_sync(n, size, "low")[0]
    assert agg == compress(ctx.aggregate_committee_bits(cid, all_bits(size), size))
    ctx.committee_drop(cid)
    gone()


def test_pubkey_overwrite_refreshes_sampled_committee():
    w = World(nkeys=64)
    try:
        act = list(range(3, 63))
        bal = M.table("mixed", 64)
        want = M.sync_committee(M.SEED, act, bal, 16, rounds=10)[0]
        idx, agg = w.ctx.sync_committee_put(10, M.SEED, act, bal, 32, 16, 10)
        assert [int(v) for v in idx] == want
        bits = all_bits(16)
        before = w.ctx.aggregate_committee_bits(10, bits, 16)
        assert before == w.ctx.aggregate_pubkeys(want) and agg == compress(before)
        pk = w.ctx.keygen(_sk_bytes(_sk(10 ** 6)), -1)
        w.ctx.pubkeys_put(want[2], pk)
        after = w.ctx.aggregate_committee_bits(10, bits, 16)
        assert after != before
        assert after == w.ctx.aggregate_pubkeys(want)
    finally:
        w.close()


def test_two_device_entries():
    w = World([0, 0], nkeys=300)
    try:
        act = list(range(299, 42, -1))  # 257 indices, reversed
        bal = M.table("low", 300)
        want = M.sync_committee(M.SEED, act, bal, 64)[0]
        idx, agg = w.ctx.sync_committee_put(100, M.SEED, act, bal, 32, 64, 90)
        assert [int(v) for v in idx] == want
        rec = w.ctx.aggregate_pubkeys(want)
        assert agg == compress(rec) and w.ctx.aggregate_committee_bits(100, all_bits(64), 64) == rec
        seeds = M.slot_seeds()[:4]
        assert w.ctx.proposers(seeds, act, bal, 32, 90) == [M.proposer(s, act, bal)[0] for s in seeds]
        # both device entries hold the committee: sets spread over them decide alike
        msg = hashlib.sha256(b"two entries").digest()
        sig = w.ctx.sign(_sk_bytes(sum(w.sks[v] for v in want) % _R()), msg)
        s = w.native.SetSpec(msg, sig, committee=100, bits=all_bits(64), n_bits=64)
        assert w.ctx.verify_jobs([([s], False)] * 8) == [1] * 8
        w.ctx.committee_drop(100)
    finally:
        w.close()
