"""GPU tests of the device-resident signature pools (include/blsgpu.h: bgv_sigpool_open /
bgv_sigpool_drop_range / bgv_sigpool_get / bgv_verify_accumulate; bgv_sigpool_plan.h,
bgv_k_sigpool.hip).

Keys and signatures are the deterministic ones of tests/golden/sig_aggregate.json (World of
tests/test_gpu_verify_aggregate.py).  The expected bytes of an entry never come from the pool: they
are the fixture's recorded oracle aggregates, oracle.bls12381.signatures_aggregate of small subsets,
and Context.aggregate_signatures of everything added so far; the codes must equal verify_jobs' on
the same input under the same set_rng_seed."""
import ctypes
import hashlib
import threading

import pytest

from tests import committeesim as cs
from tests.test_gpu_verify_aggregate import INF_SIG, NO_AGG, SEED, ZERO, World, _o, _twelve

pytestmark = pytest.mark.gpu

ORACLE_MAX = 8  # signatures the CPU oracle is asked to sum in one expectation (it does ~8 a second)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


class Pool:
    """What the entries must hold: per id the signatures added so far, in any order."""

    def __init__(self, w, ids):
        self.w, self.held = w, {}
        for i in ids:
            w.ctx.sigpool_open(i)
            self.held[i] = []

    def add(self, jobs, tags, mode=0, form=None, call=None):
        """verify_jobs and verify_accumulate on the same input under the same seed: the codes agree,
        out_added is `code == 1 and tagged`, and the launch counters show the decoding form."""
        w = self.w
        packed = w.native.PackedCall(jobs)
        w.ctx.set_rng_seed(SEED)
        want_codes = w.ctx.verify_jobs(packed, mode)
        w.ctx.set_rng_seed(SEED)
        before = w.ctx.sigpool_launches()
        codes, added = (call or w.ctx.verify_accumulate)(packed, tags, mode)
        assert codes == want_codes
        after = w.ctx.sigpool_launches()
        want_added, i = [], 0
        for (sets, _), code in zip(jobs, want_codes):
            for s in sets:
                want_added.append(code == 1 and tags[i] != NO_AGG)
                if want_added[-1]:
                    self.held[tags[i]].append(s.sig)
                i += 1
        assert added == want_added
        if form is None:
            form = "wave" if any(want_added) else "none"
        assert (after[0] - before[0], after[1] - before[1]) == {"wave": (1, 0), "lane": (0, 1), "none": (0, 0)}[form]
        return codes, added

    def check(self, ids=None, golden=None):
        """One bgv_sigpool_get of the ids against the references; returns what it gave."""
        w, native = self.w, self.w.native
        ids = list(self.held) if ids is None else ids
        got = w.ctx.sigpool_get(ids)
        dev = w.ctx.aggregate_signatures([self.held.get(i, []) for i in ids])
        for k, i in enumerate(ids):
            sub = self.held.get(i)
            if sub is None:  # not an entry of this pool: not live
                assert got[k] == (-native.BGV_E_BAD_INDEX, 0, ZERO), i
                continue
            if not sub:
                assert got[k] == (-native.BGV_E_EMPTY_AGGREGATE, 0, ZERO), i
                continue
            assert got[k][:2] == (0, len(sub)), i
            assert (0, got[k][2]) == dev[k], i
            if len(sub) <= ORACLE_MAX:
                assert (0, got[k][2]) == w.oracle_aggregate(sub), i
            if golden is not None and golden[k] is not None:
                assert got[k][2] == bytes.fromhex(golden[k]), i
        return got

    def drop(self):
        for i in self.held:
            self.w.ctx.sigpool_drop_range(i, 1)


def _jobs(w, ks):
    return [([w.good(k)], True) for k in ks]


def test_sizes_over_several_calls(world):
    """Six entries receive the fixture's runs of 1, 2, 63, 64, 65 and 129 signatures, each cut into
    two calls at a different point (the 129 as 1 + 64 + 64 over three): the accumulator is read back
    as lane 0's start, the strided loop has none, one and two terms per lane, the tree has idle
    lanes, and one call touches sparse ids."""
    w = world
    case = w.fx["cases"]["sizes"]
    assert [c for _, c in case["runs"]] == [1, 2, 63, 64, 65, 129]
    ids = [16383, 0, 7, 100, 4095, 101]
    cuts = [(1, 0, 0), (1, 1, 0), (31, 32, 0), (63, 1, 0), (1, 64, 0), (1, 64, 64)]
    pool = Pool(w, ids)
    try:
        for part in range(3):
            ks, tags = [], []
            for (first, count), cut, i in zip(case["runs"], cuts, ids):
                assert sum(cut) == count
                lo = first + sum(cut[:part])
                ks += range(lo, lo + cut[part])
                tags += [i] * cut[part]
            codes, _ = pool.add(_jobs(w, ks), tags)
            assert codes == [1] * len(ks)
            pool.check(ids)  # all six in one call, after every call
        got = pool.check(ids, golden=case["aggregates"])
        assert w.ctx.sigpool_get(ids) == got  # reading changes nothing
        assert [g[1] for g in got] == [1, 2, 63, 64, 65, 129]
    finally:
        pool.drop()


def test_both_decoding_forms(world):
    """Signatures [0, 2048) into one entry over seven calls, every step in the wavefront form: the
    fixture's wave_max aggregate; one more signature: its wave_max_plus_1 aggregate.  One call of
    2,049 into a second entry decodes one per lane and gives the same bytes."""
    w = world
    wm = w.native.SIGAGG_WAVE_MAX
    sizes = [1, 2, 63, 64, 65, 129, 1724]
    assert sum(sizes) == wm == w.fx["cases"]["wave_max"]["runs"][0][1]
    pool = Pool(w, [11, 12])
    try:
        at = 0
        for n in sizes:
            pool.add(_jobs(w, range(at, at + n)), [11] * n, form="wave")
            at += n
            pool.check([11])
        pool.check([11], golden=w.fx["cases"]["wave_max"]["aggregates"])
        pool.add(_jobs(w, [wm]), [11], form="wave")
        a = pool.check([11], golden=w.fx["cases"]["wave_max_plus_1"]["aggregates"])
        pool.add(_jobs(w, range(wm + 1)), [12] * (wm + 1), form="lane")
        b = pool.check([12], golden=w.fx["cases"]["wave_max_plus_1"]["aggregates"])
        assert a[0] == b[0] and a[0][1] == wm + 1
    finally:
        pool.drop()


def test_doubling_and_cancellation_across_calls(world):
    """jac_add's special cases against the stored accumulator: P + P, P + (-P), infinity + P."""
    w = world
    pool = Pool(w, [20, 21, 22])
    try:
        s = [w.good(0)]
        pool.add([(s, True)], [20])
        pool.add([(s, True)], [20])
        pool.add([(s, True), (s, True)], [21, 21])
        got = pool.check([20, 21])
        assert got[0] == got[1] and got[0][1] == 2
        assert (0, got[0][2]) == w.oracle_aggregate([w.sigs[0], w.sigs[0]])
        # secret keys sk and r - sk on one root, in two calls
        neg = w.native.SetSpec(w.roots[w.n], w.sigs[w.n], pk_indices=[w.n])
        pool.add([(s, True)], [22])
        pool.add([([neg], True)], [22])
        assert pool.check([22]) == [(0, 2, INF_SIG)]
        pool.add(_jobs(w, [1]), [22])
        assert pool.check([22]) == [(0, 3, w.sigs[1])]
    finally:
        pool.drop()


@pytest.mark.parametrize("mode", [0, 1], ids=["worker", "per_job"])
def test_bad_sets_are_left_out(world, mode):
    """The twelve-job mix (a wrong signer that goes through the retry rounds, a 95-byte signature,
    an off-curve one, one outside G2): eight are added, each exactly once."""
    w = world
    pool = Pool(w, [30])
    try:
        jobs, want = _twelve(w)
        codes, added = pool.add(jobs, [30] * 12, mode)
        assert codes == want
        assert added == [c == 1 for c in want] and sum(added) == 8
        assert pool.check([30])[0][:2] == (0, 8)  # the bytes: the oracle's over the eight (ORACLE_MAX)
    finally:
        pool.drop()


def test_rejected_job_and_empty_call(world):
    """A 3-set non-batchable job with one wrong signer adds none of its sets; a call that accepts
    nothing launches nothing and leaves the entry untouched."""
    w, native = world, world.native
    pool = Pool(w, [31, 32])
    try:
        ok = ([w.good(0), w.good(1), w.good(2)], False)
        bad = ([w.good(3), native.SetSpec(w.roots[4], w.sigs[5], pk_indices=[4]), w.good(6)], False)
        codes, added = pool.add([ok, bad], [31, 32, 31, 31, 32, 32])
        assert codes == [1, 0] and added == [True, True, True, False, False, False]
        before = pool.check([31, 32])
        assert [g[1] for g in before] == [2, 1]
        wrong = [([native.SetSpec(w.roots[k], w.sigs[k + 1], pk_indices=[k])], True) for k in (0, 3)]
        codes, added = pool.add(wrong, [31, 32], form="none")
        assert codes == [0, 0] and added == [False, False]
        assert pool.check([31, 32]) == before
    finally:
        pool.drop()


def test_committee_and_span_sets(world):
    """A committee-bitfield set and a span set carrying tags (the spans argument), beside a plain set."""
    w, native = world, world.native
    o = _o()
    a, b = [1, 2, 3, 4], [5, 6, 7]
    w.ctx.committee_put(100, a)
    w.ctx.committee_put(101, b)
    pool = Pool(w, [40, 41])
    try:
        msg = hashlib.sha256(b"sig-aggregate committees").digest()
        sk_com = (w.sks[1] + w.sks[3] + w.sks[4]) % o.R  # positions 0, 2, 3 of a
        sk_span = (w.sks[2] + w.sks[5] + w.sks[7]) % o.R  # position 1 of a; 0 and 2 of b
        com = native.SetSpec(msg, w.sign(sk_com, msg), committee=100, bits=cs.pack([0, 2, 3], 4), n_bits=4)
        span = native.SetSpec(msg, w.sign(sk_span, msg), committees=[100, 101], bits=cs.pack([1, 4, 6], 7), n_bits=7)
        for sets, tags in (([com, w.good(0)], [40, 41]), ([com, span, w.good(0)], [41, 40, NO_AGG])):
            codes, _ = pool.add([([s], True) for s in sets], tags)
            assert codes == [1] * len(sets)
        assert [g[1] for g in pool.check([40, 41])] == [2, 2]
    finally:
        pool.drop()
        w.ctx.committee_drop(100)
        w.ctx.committee_drop(101)


def test_argument_checks_change_nothing(world):
    """A tag on an unopened id, a tag equal to BGV_MAX_SIGPOOL, open on a live id and on an id past
    the end: each returns its code, the outputs keep their sentinel bytes and every entry is as it was."""
    w, native = world, world.native
    pool = Pool(w, [50, 51])
    try:
        pool.add(_jobs(w, [0, 1, 2]), [50, 51, 50])
        before = pool.check([50, 51, 52])
        assert before[2] == (-native.BGV_E_BAD_INDEX, 0, ZERO)
        packed = native.PackedCall(_jobs(w, [3, 4]))
        for tags, want in (([50, 52], native.BGV_E_BAD_INDEX), ([50, native.MAX_SIGPOOL], native.BGV_E_ARG),
                           ([52, native.MAX_SIGPOOL], native.BGV_E_ARG), ([NO_AGG - 1, 50], native.BGV_E_ARG)):
            out = (ctypes.c_int32 * 2)(7, 7)
            added = (ctypes.c_uint8 * 2)(7, 7)
            launches = w.ctx.sigpool_launches()
            rc = w.ctx.lib.bgv_verify_accumulate(w.ctx.handle, packed.jobs, 2, packed.sets, 2, None, 0,
                                                 (ctypes.c_uint32 * 2)(*tags), out, added, None)
            assert rc == -want, tags
            assert list(out) == [7, 7] and list(added) == [7, 7]
            assert w.ctx.sigpool_launches() == launches
            with pytest.raises(native.BlsGpuError) as e:
                w.ctx.verify_accumulate_async(packed, tags)
            assert e.value.code == want
        for bad_id in (50, native.MAX_SIGPOOL, 0xFFFFFFFF):
            with pytest.raises(native.BlsGpuError) as e:
                w.ctx.sigpool_open(bad_id)
            assert e.value.code == native.BGV_E_ARG
        # an id past the end in a get: nothing is written
        buf = ctypes.create_string_buffer(b"\xAA" * 192, 192)
        cnt, st = (ctypes.c_uint32 * 2)(7, 7), (ctypes.c_int32 * 2)(7, 7)
        rc = w.ctx.lib.bgv_sigpool_get(w.ctx.handle, (ctypes.c_uint32 * 2)(50, native.MAX_SIGPOOL), 2, buf, cnt, st)
        assert rc == -native.BGV_E_ARG
        assert buf.raw == b"\xAA" * 192 and list(cnt) == [7, 7] and list(st) == [7, 7]
        assert pool.check([50, 51, 52]) == before
        # a null pool_of_set is the plain call
        out = (ctypes.c_int32 * 2)(7, 7)
        assert w.ctx.lib.bgv_verify_accumulate(w.ctx.handle, packed.jobs, 2, packed.sets, 2, None, 0, None, out,
                                               None, None) == 0
        assert list(out) == [1, 1] and pool.check([50, 51]) == before[:2]
    finally:
        pool.drop()


def test_drop_and_reopen(world):
    w, native = world, world.native
    pool = Pool(w, [60, 61, 63])
    try:
        pool.add(_jobs(w, [0, 1, 2]), [60, 61, 60])
        full = pool.check([60])[0]
        assert w.ctx.sigpool_drop_range(60, 4) == 3  # 60, 61 and 63 are live, 62 is not
        assert w.ctx.sigpool_drop_range(60, 4) == 0
        assert w.ctx.sigpool_get([60]) == [(-native.BGV_E_BAD_INDEX, 0, ZERO)]
        with pytest.raises(native.BlsGpuError) as e:
            w.ctx.verify_accumulate(_jobs(w, [0]), [60])
        assert e.value.code == native.BGV_E_BAD_INDEX
        for i in (60, 61):  # at once
            w.ctx.sigpool_open(i)
            pool.held[i] = []
        assert w.ctx.sigpool_get([60]) == [(-native.BGV_E_EMPTY_AGGREGATE, 0, ZERO)]
        pool.add(_jobs(w, [5]), [61])  # the reopened entry starts from infinity, not from what it held
        one = (0, 1, w.sigs[5])
        empty, gone = (-native.BGV_E_EMPTY_AGGREGATE, 0, ZERO), (-native.BGV_E_BAD_INDEX, 0, ZERO)
        assert w.ctx.sigpool_get([61, 60, 63, 61, 62, 61]) == [one, empty, gone, one, gone, one]
        assert full[1] == 2 and full != one
        assert w.ctx.sigpool_drop_range(native.MAX_SIGPOOL - 1, 0xFFFFFFFF) == 0  # the range ends with the ids
        assert w.ctx.sigpool_get([]) == []
    finally:
        w.ctx.sigpool_drop_range(60, 4)


def test_async_form(world):
    """The asynchronous form: the additions are visible to get once wait() returns."""
    w = world
    pool = Pool(w, [70, 71])
    try:
        jobs, want = _twelve(w)

        def call(packed, tags, mode):
            return w.ctx.verify_accumulate_async(packed, tags, mode).wait(60)

        codes, added = pool.add(jobs, [70, 71] * 6, call=call)
        assert codes == want
        assert [g[:2] for g in pool.check([70, 71])] == [(0, 4), (0, 4)]
        pending = [w.ctx.verify_accumulate_async(_jobs(w, range(20 + 8 * k, 28 + 8 * k)), [70] * 8) for k in range(4)]
        for k, p in enumerate(pending):
            assert p.wait(60) == ([1] * 8, [True] * 8)
            pool.held[70] += [w.sigs[i] for i in range(20 + 8 * k, 28 + 8 * k)]
        assert pool.check([70])[0][1] == 36
    finally:
        pool.drop()


def test_exactly_once_under_concurrency(world):
    """Eight threads, four synchronous calls each of eight one-set jobs into the same two entries
    (ctypes releases the GIL; the verdict passes merge into super-batches as they fall)."""
    w = world
    pool = Pool(w, [80, 81])
    errors = []

    def worker(t):
        try:
            for c in range(4):
                ks = range(32 * t + 8 * c, 32 * t + 8 * c + 8)
                got = w.ctx.verify_accumulate(_jobs(w, ks), [80 + (k & 1) for k in ks])
                assert got == ([1] * 8, [True] * 8), (t, c, got)
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    try:
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for k in range(256):
            pool.held[80 + (k & 1)].append(w.sigs[k])
        assert [g[1] for g in pool.check([80, 81])] == [128, 128]
    finally:
        pool.drop()


def test_agrees_with_the_fused_call(world):
    """bgv_verify_aggregate's per-call aggregates over the same calls, summed by the oracle, are
    the pool's bytes."""
    w = world
    pool = Pool(w, [90])
    try:
        per_call = []
        for ks in ([0, 1, 2], [3, 4, 5, 6, 7], [8, 2]):
            jobs = _jobs(w, ks)
            pool.add(jobs, [90] * len(ks))
            codes, aggs = w.ctx.verify_aggregate(jobs, [0] * len(ks), 1)
            assert codes == [1] * len(ks) and aggs[0][:2] == (0, len(ks))
            per_call.append(aggs[0][2])
        got = w.ctx.sigpool_get([90])[0]
        assert got[:2] == (0, 10)
        assert (0, got[2]) == w.oracle_aggregate(per_call)
        pool.check([90])
    finally:
        pool.drop()


def test_python_verifier_pool_same_message(world):
    """verifier.BlsGpuVerifier.verify_and_pool_same_message: one bool per set, True iff accepted
    and added."""
    import asyncio

    from lodestar_amd.verifier import BlsGpuVerifier
    w = world
    ks = [0, 3, 6, 9]  # signers of one root
    sets = [(k, w.sigs[k]) for k in ks]
    sets[1] = (3, w.sigs[6])  # a wrong signer
    sets[2] = (6, w.sigs[6][:95])  # undecodable
    pool = Pool(w, [95])
    try:
        async def run():
            v = BlsGpuVerifier(ctx=w.ctx)
            return await v.verify_and_pool_same_message(sets, w.roots[0], 95), \
                await v.verify_and_pool_same_message([], w.roots[0], 95)

        assert asyncio.run(run()) == ([True, False, False, True], [])
        pool.held[95] = [w.sigs[0], w.sigs[9]]
        assert pool.check([95])[0][1] == 2
    finally:
        pool.drop()


def test_call_after_close():
    from lodestar_amd import native
    ctx = native.Context()
    try:
        sk = int(_o().interop_secret_key(0)).to_bytes(32, "big")
        ctx.keygen(sk, cache_first=0, want_pubkeys=False)
        msg = hashlib.sha256(b"sig-aggregate root 0").digest()
        sig = ctx.sign(sk, msg)
        jobs = [([native.SetSpec(msg, sig, pk_indices=[0])], True)]
        ctx.sigpool_open(0)
        assert ctx.verify_accumulate(jobs, [0]) == ([1], [True])
        assert ctx.sigpool_get([0]) == [(0, 1, sig)]
        assert ctx.lib.bgv_close(ctx.handle) == 0
        calls = [lambda: ctx.sigpool_open(1), lambda: ctx.sigpool_drop_range(0, 1), lambda: ctx.sigpool_get([0]),
                 lambda: ctx.verify_accumulate(jobs, [0]), lambda: ctx.verify_accumulate_async(jobs, [0]),
                 ctx.sigpool_launches]
        for call in calls:
            with pytest.raises(native.BlsGpuError) as e:
                call()
            assert e.value.code == native.BGV_E_CLOSED
    finally:
        ctx.close()
