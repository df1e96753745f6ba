"""GPU tests of the device-side epoch shuffling (include/blsgpu.h bgv_shuffling_put,
bgv_committee_drop_range): the shuffling read back from the device against the spec-pseudocode
hashlib model (tests/shufflesim.py) and the reference's unshuffleList vectors, and the committees
it fills against bgv_aggregate_pubkeys over the expected members and against the verdicts of the
same sets given as index lists.
"""
import functools
import hashlib

import pytest

from tests import shufflesim as S

pytestmark = pytest.mark.gpu

NKEYS = 2400
SEED = hashlib.sha256(b"lodestar-amd gpu shuffling").digest()


def _R():
    from oracle import bls12381 as o  # the group order alone; never the code under test
    return o.R


def _sk(i):
    return 1 + int.from_bytes(hashlib.sha256(b"shuffling sk %d" % i).digest(), "big") % (_R() - 1)


def _sk_bytes(v):
    return int(v).to_bytes(32, "big")


def gapped(n):
    """n distinct validator indices below NKEYS with every seventh index left out."""
    return [i + i // 6 for i in range(n)]


def pack(positions, n):
    b = bytearray((n + 7) // 8)
    for p in positions:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def model(n, rounds=90, seed=SEED):
    return S.model_shuffle(seed, rounds, gapped(n))


def committees_of(shuffling, slots, cps):
    return [shuffling[lo:hi] for lo, hi in S.model_committees(len(shuffling), slots, cps)]


class World:
    def __init__(self, devices=None, nkeys=NKEYS):
        from lodestar_amd import native
        self.native = native
        self.sks = [_sk(i) for i in range(nkeys)]
        self.ctx = native.Context(devices)
        self.ctx.keygen(b"".join(_sk_bytes(s) for s in self.sks), 0, want_pubkeys=False)
        assert self.ctx.pubkeys_count() == nkeys

    def check_committees(self, first_id, coms):
        """all-bits aggregate of every non-empty committee == bgv_aggregate_pubkeys of its members"""
        bad = [k for k, m in enumerate(coms) if m and
               self.ctx.aggregate_committee_bits(first_id + k, pack(range(len(m)), len(m)), len(m))
               != self.ctx.aggregate_pubkeys(m)]
        assert not bad, bad

    def code_of(self, fn, *a):
        with pytest.raises(self.native.BlsGpuError) as e:
            fn(*a)
        return e.value.code

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture(scope="module")
def epoch(world):
    """(2049, 32, 2) under ids 2048..2111, kept for the tests that read it."""
    got = world.ctx.shuffling_put(2048, SEED, gapped(2049), 32, 2, 90)
    return 2048, [int(v) for v in got], committees_of(model(2049), 32, 2)


@pytest.mark.parametrize("n,rounds", [(1, 90), (2, 90), (255, 90), (256, 90), (257, 90), (513, 90), (513, 10),
                                      (2049, 90)])
def test_readback_matches_model(world, n, rounds):
    """Around the 256-position hash block, more than one thread block (256 threads) and more
    than eight table blocks; one committee holds the whole list."""
    got = world.ctx.shuffling_put(0, SEED, gapped(n), 1, 1, rounds)
    try:
        assert [int(v) for v in got] == model(n, rounds)
        world.check_committees(0, [model(n, rounds)])
    finally:
        assert world.ctx.committee_drop_range(0, 1) == 1


def test_readback_kat(world):
    v = S.fixture()["unshuffle"][1]
    assert len(v["input"]) == 16
    got = world.ctx.shuffling_put(0, bytes.fromhex(v["seed"]), v["input"], 1, 1, v["rounds"])
    try:
        assert [int(x) for x in got] == v["res"]
    finally:
        assert world.ctx.committee_drop_range(0, 1) == 1


def test_committees(world, epoch):
    first, got, coms = epoch
    assert got == model(2049)
    assert len(coms) == 64 and all(coms)
    world.check_committees(first, coms)
    for k in (0, 31, 63):  # a partial bitfield
        m = coms[k]
        pos = [p for p in range(len(m)) if p % 3 != 1]
        assert world.ctx.aggregate_committee_bits(first + k, pack(pos, len(m)), len(m)) == \
            world.ctx.aggregate_pubkeys([m[p] for p in pos])


def test_empty_committees(world):
    native = world.native
    n, slots, cps, first = 20, 8, 4, 4096
    got = world.ctx.shuffling_put(first, SEED, gapped(n), slots, cps, 90)
    try:
        assert [int(v) for v in got] == model(n)
        coms = committees_of(model(n), slots, cps)
        empty = [k for k, m in enumerate(coms) if not m]
        assert len(empty) == 12
        for k in empty:
            assert world.code_of(world.ctx.aggregate_committee_bits, first + k, bytes([1]), 1) == native.BGV_E_BAD_INDEX
        msg = hashlib.sha256(b"empty").digest()
        sig = world.ctx.sign(_sk_bytes(world.sks[0]), msg)
        s = native.SetSpec(msg, sig, committee=first + empty[0], bits=bytes([1]), n_bits=1)
        assert world.ctx.verify_jobs([([s], False)]) == [-native.BGV_E_BAD_INDEX]
        world.check_committees(first, coms)
    finally:
        assert world.ctx.committee_drop_range(first, slots * cps) == 20


def test_verdicts(world, epoch):
    """A valid set and one with a flipped bit on three shuffled committees; the signature comes
    from the sum of the participants' secret keys; the index-list form decides the same."""
    native = world.native
    first, _, coms = epoch
    R = _R()
    cj, ij, want = [], [], []
    for k in (1, 17, 62):
        m = coms[k]
        pos = [p for p in range(len(m)) if p % 5 != 2]
        msg = hashlib.sha256(b"shuffled committee %d" % k).digest()
        sig = world.ctx.sign(_sk_bytes(sum(world.sks[m[p]] for p in pos) % R), msg)
        for p, code in ((pos, 1), (pos[1:], 0)):
            cj.append(([native.SetSpec(msg, sig, committee=first + k, bits=pack(p, len(m)), n_bits=len(m))], False))
            ij.append(([native.SetSpec(msg, sig, pk_indices=[m[q] for q in p])], False))
            want.append(code)
    got = world.ctx.verify_jobs(cj)
    assert got == want
    assert world.ctx.verify_jobs(ij) == got


def test_errors_and_atomicity(world):
    native, ctx = world.native, world.ctx
    first, n, slots, cps = 8192, 513, 8, 2
    act = gapped(n)
    ctx.committee_put(first + 5, [1, 2, 3])  # a live id in the middle of the range
    assert world.code_of(ctx.shuffling_put, first, SEED, act, slots, cps, 90) == native.BGV_E_ARG
    assert world.code_of(ctx.aggregate_committee_bits, first, bytes([1]), 1) == native.BGV_E_BAD_INDEX
    assert ctx.committee_drop_range(first, slots * cps) == 1
    assert world.code_of(ctx.shuffling_put, first, SEED, act[:-1] + [NKEYS], slots, cps, 90) == native.BGV_E_BAD_INDEX
    assert world.code_of(ctx.shuffling_put, first, SEED, act, slots, cps, 256) == native.BGV_E_ARG
    assert world.code_of(ctx.shuffling_put, first, SEED, act, 0, cps, 90) == native.BGV_E_ARG
    assert world.code_of(ctx.shuffling_put, native.MAX_COMMITTEES - 15, SEED, act, slots, cps, 90) == native.BGV_E_ARG
    assert ctx.committee_drop_range(first, slots * cps) == 0  # none of the failed calls left an id
    coms = committees_of(model(n), slots, cps)
    bits = [pack(range(len(m)), len(m)) for m in coms]
    ctx.shuffling_put(first, SEED, act, slots, cps, 90)
    agg1 = [ctx.aggregate_committee_bits(first + k, bits[k], len(m)) for k, m in enumerate(coms)]
    world.check_committees(first, coms)
    assert ctx.committee_drop_range(first, slots * cps) == slots * cps
    assert world.code_of(ctx.aggregate_committee_bits, first, bits[0], len(coms[0])) == native.BGV_E_BAD_INDEX
    got = ctx.shuffling_put(first, SEED, act, slots, cps, 90)
    assert [int(v) for v in got] == model(n)
    assert [ctx.aggregate_committee_bits(first + k, bits[k], len(m)) for k, m in enumerate(coms)] == agg1
    assert ctx.committee_drop_range(first, slots * cps) == slots * cps


def test_pubkey_overwrite_refreshes_shuffled_committee():
    """bgv_pubkeys_put over a member: the committee's sum is recomputed from the host mirror
    that was read back from the device."""
    w = World(nkeys=64)
    try:
        act = list(range(3, 63))
        shuf = S.model_shuffle(SEED, 10, act)
        assert [int(v) for v in w.ctx.shuffling_put(10, SEED, act, 4, 2, 10)] == shuf
        coms = committees_of(shuf, 4, 2)
        m = coms[5]
        bits = pack(range(len(m)), len(m))
        before = w.ctx.aggregate_committee_bits(15, bits, len(m))
        assert before == w.ctx.aggregate_pubkeys(m)
        pk = w.ctx.keygen(_sk_bytes(_sk(10 ** 6)), -1)
        w.ctx.pubkeys_put(m[2], pk)
        after = w.ctx.aggregate_committee_bits(15, bits, len(m))
        assert after != before
        assert after == w.ctx.aggregate_pubkeys(m)
        w.check_committees(10, coms)
    finally:
        w.close()


def test_two_device_entries():
    w = World([0, 0], nkeys=300)
    try:
        act = list(range(299, 42, -1))  # 257 indices, reversed
        shuf = S.model_shuffle(SEED, 90, act)
        assert [int(v) for v in w.ctx.shuffling_put(100, SEED, act, 8, 2, 90)] == shuf
        w.check_committees(100, committees_of(shuf, 8, 2))
        assert w.ctx.committee_drop_range(100, 16) == 16
    finally:
        w.close()
