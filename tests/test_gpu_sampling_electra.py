"""GPU tests of the device-side balance-weighted sampling under Electra's rule (include/blsgpu.h
bgv_proposers_electra, bgv_sync_committee_put_electra): the proposers and sync committees read back
from the device against the spec-pseudocode hashlib model (tests/samplesim_electra.py), the
aggregate against bgv_aggregate_pubkeys of the same list, and the committee a put leaves behind
against the verdicts of the same sets given as index lists.

The shapes are the smallest that cross each boundary: 16 candidates per digest of draws, the
256-candidate block, the second pass, and the 256-position shuffle block at n = 257 and 513.
"""
import functools
import hashlib

import numpy as np
import pytest

from tests import samplesim_electra as M
from tests.test_gpu_shuffling import NKEYS, World, _R, _sk_bytes, pack

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 257, 513]
SYNC_CASES = [(40, 64, "full"), (300, 64, "min"), (2049, 512, "mixed"), (2049, 128, "min"), (1, 8, "min"),
              (300, 64, "high")]
# (seed, eff, max_incr, accepted): candidate 0 draws 0xFFFF under EDGE_FFFF and 0 under EDGE_0000
EDGE_CASES = [(M.EDGE_FFFF, 2048, 2048, True), (M.EDGE_FFFF, 2047, 2048, False), (M.EDGE_FFFF, 65535, 65535, True),
              (M.EDGE_FFFF, 65534, 65535, False), (M.EDGE_0000, 0, 2048, True)]
EDGE_IDS = ["ffff-2048of2048", "ffff-2047of2048", "ffff-65535of65535", "ffff-65534of65535", "0000-0of2048"]


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
    """The (40, 64, full) committee, which holds repeats, under id 710; kept for the test that reads it."""
    idx, agg = world.ctx.sync_committee_put_electra(710, M.SEED, M.active(40), eff("full"), 2048, 64, 90)
    return 710, [int(v) for v in idx], agg


@pytest.mark.parametrize("name", list(M.TABLES))
def test_proposers_match_model(world, name):
    """32 slot seeds; `min` goes past candidate 16 (the second digest of draws) and, at n = 513,
    past candidate 256 (a second pass); `high` has a zero low byte in every balance."""
    seeds = M.slot_seeds()
    for n in SIZES:
        want = [M.proposer(s, M.active(n), eff(name))[0] for s in seeds]
        assert world.ctx.proposers_electra(seeds, M.active(n), eff(name), 2048, 90) == want, (name, n)
        if (name, n) in (("mixed", 1), ("min", 1), ("min", 2)):
            assert want == [None] * 32
        if (name, n) == ("high", 2):
            assert want.count(None) == 20


@pytest.mark.parametrize("n,size,name", SYNC_CASES)
def test_sync_committee_matches_model(world, n, size, name):
    want, tries = model_sync(n, size, name)
    idx, agg = world.ctx.sync_committee_put_electra(910, M.SEED, M.active(n), eff(name), 2048, size, 90)
    try:
        assert [int(v) for v in idx] == want, tries
        rec = world.ctx.aggregate_pubkeys(want)
        assert agg == compress(rec)
        assert world.ctx.aggregate_committee_bits(910, all_bits(size), size) == rec
    finally:
        world.ctx.committee_drop(910)


@pytest.mark.parametrize("seed,e,max_incr,ok", EDGE_CASES, ids=EDGE_IDS)
def test_edge_draws(world, seed, e, max_incr, ok):
    """One active index, n_eff = 1, a draw of 0xFFFF or 0: equality accepts, one below rejects,
    and 65535 * 65535 on both sides does not wrap."""
    assert world.ctx.proposers_electra([seed], [0], [e], max_incr, 90) == [0 if ok else None]


def test_accepts_uint16_arrays_and_refuses_wider_values(world):
    seeds = M.slot_seeds()[:4]
    act = M.active(257)
    want = [M.proposer(s, act, eff("high"))[0] for s in seeds]
    assert world.ctx.proposers_electra(seeds, act, np.array(eff("high"), dtype=np.uint16)) == want
    assert world.ctx.proposers_electra(seeds, act, np.array(eff("high"), dtype=np.int64)) == want
    for bad in ([65536] * NKEYS, [-1] * NKEYS):
        with pytest.raises(ValueError):
            world.ctx.proposers_electra(seeds, act, bad)
        with pytest.raises(ValueError):
            world.ctx.sync_committee_put_electra(911, M.SEED, act, bad, 2048, 8, 90)
    assert world.code_of(world.ctx.aggregate_committee_bits, 911, all_bits(8), 8) == world.native.BGV_E_BAD_INDEX


def test_verdicts(world, repeats):
    """A valid set with a partial bitfield and one with a flipped bit on the committee with
    repeats; the signature comes from the sum of the participants' secret keys, repeats counted;
    the index-list form decides the same."""
    native = world.native
    cid, idx, agg = repeats
    assert idx == model_sync(40, 64, "full")[0] and len(set(idx)) == 40
    assert agg == compress(world.ctx.aggregate_pubkeys(idx))
    pos = [p for p in range(64) if p % 5 != 2]
    assert len(set(idx[p] for p in pos)) < len(pos)  # a participant counted twice
    msg = hashlib.sha256(b"sampled sync committee, electra").digest()
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
    cid, n, size = 1210, 300, 64
    act, bal = M.active(n), eff("mixed")
    put = ctx.sync_committee_put_electra

    def gone():
        assert world.code_of(ctx.aggregate_committee_bits, cid, all_bits(size), size) == native.BGV_E_BAD_INDEX

    # All-zero balances: a candidate is accepted on a draw of 0 only (0 * 65535 >= 2048 * 0), and the
    # first 65,536 candidates of SEED hold two of them: a committee of 8 hits the cap, a bounded run.
    assert sum(M.rand16(M.SEED, i) == 0 for i in range(M.MAX_TRIES)) == 2
    assert world.code_of(put, cid, M.SEED, act, [0] * NKEYS, 2048, 8, 90) == native.BGV_E_ARG
    gone()
    ctx.committee_put(cid, [1, 2, 3])  # a live id
    assert world.code_of(put, cid, M.SEED, act, bal, 2048, size, 90) == native.BGV_E_ARG
    assert ctx.aggregate_committee_bits(cid, bytes([7]), 3) == ctx.aggregate_pubkeys([1, 2, 3])  # untouched
    ctx.committee_drop(cid)
    for bad in (dict(max_incr=0), dict(max_incr=65536), dict(rounds=256),
                dict(active=act[:-1] + [NKEYS - 1], eff=bal[:NKEYS - 1])):
        a = dict(active=act, eff=bal, max_incr=2048, rounds=90)
        a.update(bad)
        assert world.code_of(put, cid, M.SEED, a["active"], a["eff"], a["max_incr"], size, a["rounds"]) == \
            native.BGV_E_ARG
        gone()
    # an index the balances cover and the pubkey cache does not
    assert world.code_of(put, cid, M.SEED, act[:-1] + [NKEYS], [2048] * (NKEYS + 1), 2048, size, 90) == \
        native.BGV_E_BAD_INDEX
    gone()
    # the proposers' argument checks
    seeds = M.slot_seeds()[:2]
    for a in ((seeds, act, bal, 0, 90), (seeds, act, bal, 65536, 90), (seeds, act, bal, 2048, 256),
              ([], act, bal, 2048, 90), (seeds, [], bal, 2048, 90), (seeds, act[:-1] + [NKEYS], bal, 2048, 90)):
        assert world.code_of(ctx.proposers_electra, *a) == native.BGV_E_ARG
    # max_incr 65535 is in range
    assert ctx.proposers_electra(seeds, act, bal, 65535, 90) == [M.proposer(s, act, bal, 65535)[0] for s in seeds]
    # a following put on the id succeeds
    idx, agg = put(cid, M.SEED, act, bal, 2048, size, 90)
    assert [int(v) for v in idx] == M.sync_committee(M.SEED, act, bal, size)[0]
    assert agg == compress(ctx.aggregate_committee_bits(cid, all_bits(size), size))
    ctx.committee_drop(cid)
    gone()


def test_two_device_entries():
    w = World([0, 0], nkeys=300)
    try:
        act = list(range(299, 42, -1))  # 257 indices, reversed
        bal = M.table("mixed", 300)
        want = M.sync_committee(M.SEED, act, bal, 64)[0]
        idx, agg = w.ctx.sync_committee_put_electra(100, M.SEED, act, bal, 2048, 64, 90)
        assert [int(v) for v in idx] == want
        rec = w.ctx.aggregate_pubkeys(want)
        assert agg == compress(rec) and w.ctx.aggregate_committee_bits(100, all_bits(64), 64) == rec
        seeds = M.slot_seeds()[:4]
        low = M.table("min", 300)
        assert w.ctx.proposers_electra(seeds, act, low, 2048, 90) == [M.proposer(s, act, low)[0] for s in seeds]
        # both device entries hold the committee: sets spread over them decide alike
        msg = hashlib.sha256(b"two entries, electra").digest()
        sig = w.ctx.sign(_sk_bytes(sum(w.sks[v] for v in want) % _R()), msg)
        s = w.native.SetSpec(msg, sig, committee=100, bits=all_bits(64), n_bits=64)
        assert w.ctx.verify_jobs([([s], False)] * 8) == [1] * 8
        w.ctx.committee_drop(100)
    finally:
        w.close()
