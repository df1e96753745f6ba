"""GPU tests of pool entries with participation bits and of entry sums (include/blsgpu.h:
bgv_sigpool_open_bits / bgv_verify_accumulate_bits / bgv_sigpool_get_bits / bgv_sigpool_sum;
bgv_sigpool_bits_plan.h, k_sigpool_sum of bgv_k_sigpool.hip).

Keys and signatures are the deterministic ones of tests/golden/sig_aggregate.json (World of
tests/test_gpu_verify_aggregate.py).  No expected byte comes from the pool itself: they are
oracle.bls12381.signatures_aggregate of up to 8 signatures, Context.aggregate_signatures of the same
multiset, and the oracle's recorded aggregates of tests/golden/sigpool_sum.json
(tools/gen_golden_sigpool_sum.py).  The codes must equal verify_jobs' on the same input under the
same set_rng_seed."""
import ctypes
import hashlib
import json
import os
import random
import threading

import pytest

from tests import sig_edges as se
from tests.test_gpu_sigpool import Pool, _jobs
from tests.test_gpu_verify_aggregate import INF_SIG, NO_AGG, SEED, ZERO, World, _o, _twelve

pytestmark = pytest.mark.gpu

NOT_ADDED, ADDED, KNOWN, OVERLAP = 0, 1, 2, 3
ORACLE_MAX = 8


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture(scope="module")
def golden(world):
    with open(os.path.join(se.GOLD, "sigpool_sum.json")) as f:
        fx = json.load(f)
    assert hashlib.sha256(b"".join(world.sigs[:fx["n"]])).hexdigest() == fx["sigs_sha256"], \
        "regenerate tests/golden/sigpool_sum.json"
    return {int(k): bytes.fromhex(v) for k, v in fx["runs"].items()}


def field(positions, n_bits):
    b = bytearray((n_bits + 7) // 8)
    for k in positions:
        b[k // 8] |= 1 << (k % 8)
    return bytes(b)


def step(w, jobs, tags, members, mode=0, call=None):
    """verify_jobs and verify_accumulate_bits on the same input under the same seed: the codes
    agree.  Returns (codes, outcome, (wavefront, lane) launches of this call)."""
    packed = w.native.PackedCall(jobs)
    w.ctx.set_rng_seed(SEED)
    want = w.ctx.verify_jobs(packed, mode)
    w.ctx.set_rng_seed(SEED)
    before = w.ctx.sigpool_launches()
    codes, outcome = (call or w.ctx.verify_accumulate_bits)(packed, tags, members, mode)
    after = w.ctx.sigpool_launches()
    assert codes == want
    return codes, outcome, (after[0] - before[0], after[1] - before[1])


def expect(w, sigs):
    """The bytes an entry holding exactly sigs must give: the device's aggregation of the multiset,
    and the oracle's for small ones."""
    code, b = w.ctx.aggregate_signatures([sigs])[0]
    assert code == 0
    if len(sigs) <= ORACLE_MAX:
        assert (0, b) == w.oracle_aggregate(sigs)
    return b


def test_singles(world):
    """Ten members of a 130-position entry over two calls; position 8 twice within the first call,
    positions 7 and 64 again in the second."""
    w = world
    w.ctx.sigpool_open(200, 130)
    try:
        assert w.ctx.sigpool_get_bits([200]) == [(-w.native.BGV_E_EMPTY_AGGREGATE, 0, ZERO, 130, bytes(17))]
        pos = [0, 7, 8, 63, 64, 127, 128, 129, 1, 2]  # of signatures 0 .. 9
        ks = [0, 1, 2, 2, 3, 4, 5]
        codes, outcome, launches = step(w, _jobs(w, ks), [200] * 7, [(130, pos[k]) for k in ks])
        assert codes == [1] * 7 and outcome == [ADDED, ADDED, ADDED, KNOWN, ADDED, ADDED, ADDED]
        assert launches == (1, 0)
        got = w.ctx.sigpool_get_bits([200])[0]
        assert got == (0, 6, expect(w, w.sigs[:6]), 130, field(pos[:6], 130))
        ks = [6, 1, 7, 8, 4, 9]
        codes, outcome, launches = step(w, _jobs(w, ks), [200] * 6, [(130, pos[k]) for k in ks])
        assert codes == [1] * 6 and outcome == [ADDED, KNOWN, ADDED, ADDED, KNOWN, ADDED]
        assert launches == (1, 0)
        got = w.ctx.sigpool_get_bits([200])[0]
        assert got == (0, 10, expect(w, w.sigs[:10]), 130, field(pos, 130))
        assert w.ctx.sigpool_get([200]) == [got[:3]]
    finally:
        w.ctx.sigpool_drop_range(200, 1)


def _pair(w, a, b):
    """The two-signer aggregate of signers a and b (one root: both are multiples of 3)."""
    code, sig = w.ctx.aggregate_signatures([[w.sigs[a], w.sigs[b]]])[0]
    assert code == 0 and w.roots[a] == w.roots[b]
    return w.native.SetSpec(w.roots[a], sig, pk_indices=[a, b])


def test_fields_in_set_order(world):
    """A = {0,1}, B = {1,2}, C = {2,3} on one entry in one call: added, overlap, added; then A again:
    known; then a superset of B: overlap.  The entry is the sum of A and C alone."""
    w = world
    signer = [0, 3, 6, 9]  # position -> signer
    A, B, C = _pair(w, 0, 3), _pair(w, 3, 6), _pair(w, 6, 9)
    w.ctx.sigpool_open(210, 4)
    try:
        members = [(4, field(p, 4)) for p in ([0, 1], [1, 2], [2, 3])]
        codes, outcome, launches = step(w, [([s], True) for s in (A, B, C)], [210] * 3, members)
        assert codes == [1, 1, 1] and outcome == [ADDED, OVERLAP, ADDED] and launches == (1, 0)
        want = (0, 2, expect(w, [w.sigs[k] for k in signer]), 4, b"\x0f")
        assert w.ctx.sigpool_get_bits([210]) == [want]
        code, big = w.ctx.aggregate_signatures([[w.sigs[0], w.sigs[3], w.sigs[6]]])[0]
        sup = w.native.SetSpec(w.roots[0], big, pk_indices=[0, 3, 6])
        codes, outcome, launches = step(w, [([A], True), ([sup], True)], [210] * 2,
                                        [(4, field([0, 1], 4)), (4, field([0, 1, 2], 4))])
        assert codes == [1, 1] and outcome == [KNOWN, KNOWN] and launches == (0, 0)
        assert w.ctx.sigpool_get_bits([210]) == [want]
    finally:
        w.ctx.sigpool_drop_range(210, 1)
    # a superset of B that reaches past what the entry holds
    w.ctx.sigpool_open(210, 4)
    try:
        codes, outcome, _ = step(w, [([B], True), ([sup], True), ([w.good(9)], True)], [210] * 3,
                                 [(4, field([1, 2], 4)), (4, field([0, 1, 2], 4)), (4, 3)])
        assert codes == [1, 1, 1] and outcome == [ADDED, OVERLAP, ADDED]
        assert w.ctx.sigpool_get_bits([210]) == [(0, 2, expect(w, [w.sigs[3], w.sigs[6], w.sigs[9]]), 4, b"\x0e")]
    finally:
        w.ctx.sigpool_drop_range(210, 1)


def test_all_known_call_does_no_device_work(world):
    w = world
    w.ctx.sigpool_open(220, 9)
    try:
        step(w, _jobs(w, [0, 1, 2]), [220] * 3, [(9, 0), (9, 8), (9, 4)])
        before = w.ctx.sigpool_get_bits([220])
        counters = w.ctx.sigpool_launches()
        codes, outcome, launches = step(w, _jobs(w, [2, 0, 1]), [220] * 3, [(9, 4), (9, 0), (9, field([8], 9))])
        assert codes == [1, 1, 1] and outcome == [KNOWN] * 3 and launches == (0, 0)
        assert w.ctx.sigpool_launches() == counters
        assert w.ctx.sigpool_get_bits([220]) == before == [(0, 3, expect(w, w.sigs[:3]), 9, b"\x11\x01")]
    finally:
        w.ctx.sigpool_drop_range(220, 1)


@pytest.mark.parametrize("mode", [0, 1], ids=["worker", "per_job"])
def test_rejected_sets_set_no_bit(world, mode):
    """The twelve-job mix with position k for set k: the four bad sets set no bit."""
    w = world
    w.ctx.sigpool_open(230, 12)
    try:
        jobs, want = _twelve(w)
        codes, outcome, _ = step(w, jobs, [230] * 12, [(12, k) for k in range(12)], mode)
        assert codes == want
        assert outcome == [ADDED if c == 1 else NOT_ADDED for c in want] and outcome.count(ADDED) == 8
        good = [k for k in range(12) if want[k] == 1]
        assert w.ctx.sigpool_get_bits([230]) == [(0, 8, expect(w, [w.sigs[k] for k in good]), 12, field(good, 12))]
    finally:
        w.ctx.sigpool_drop_range(230, 1)


def test_plain_entry_and_untagged_sets_beside_a_bits_entry(world):
    w = world
    w.ctx.sigpool_open(240, 8)
    w.ctx.sigpool_open(241)
    try:
        codes, outcome, _ = step(w, _jobs(w, [0, 1, 2, 3, 1]), [240, 241, NO_AGG, 241, 240],
                                 [(8, 7), None, (99, 5), (3, 200), (8, 7)])
        assert codes == [1] * 5 and outcome == [ADDED, ADDED, NOT_ADDED, ADDED, KNOWN]
        got = w.ctx.sigpool_get_bits([240, 241])
        assert got == [(0, 1, w.sigs[0], 8, b"\x80"), (0, 2, expect(w, [w.sigs[1], w.sigs[3]]), 0, b"")]
        # no bits_of_set at all is fine while only plain entries are tagged
        codes, outcome, _ = step(w, _jobs(w, [4]), [241], None)
        assert codes == [1] and outcome == [ADDED] and w.ctx.sigpool_get([241])[0][1] == 3
    finally:
        w.ctx.sigpool_drop_range(240, 2)


def test_argument_checks_change_nothing(world):
    w, native = world, world.native
    w.ctx.sigpool_open(250, 130)
    w.ctx.sigpool_open(251)
    try:
        step(w, _jobs(w, [0, 1]), [250, 251], [(130, 129), None])
        ids = [250, 251, 252]
        before, counters = w.ctx.sigpool_get_bits(ids), w.ctx.sigpool_launches()
        packed = native.PackedCall(_jobs(w, [3, 4]))
        E_ARG, E_IDX = native.BGV_E_ARG, native.BGV_E_BAD_INDEX
        stray = bytearray(17)
        stray[0], stray[16] = 1, 0x04  # position 130
        cases = [
            ([250, native.MAX_SIGPOOL], [(130, 0), None], E_ARG),
            ([252, 250], [(130, 0), (130, 130)], E_IDX),  # the tag checks come first
            ([250, 251], None, E_ARG),
            ([250, 251], [(129, 0), None], E_ARG),
            ([250, 251], [(131, 0), None], E_ARG),
            ([251, 250], [None, (130, 130)], E_ARG),
            ([251, 250], [None, (130, 0xFFFFFFFF)], E_ARG),
            ([250, 251], [(130, bytes(stray)), None], E_ARG),
            ([250, 251], [(130, bytes(17)), None], E_ARG),
            ([250, 250], [(130, 5), None], E_ARG),  # n_bits 0 is not the entry's
        ]
        for tags, members, want in cases:
            out = (ctypes.c_int32 * 2)(7, 7)
            outcome = (ctypes.c_uint8 * 2)(7, 7)
            bits, _keep = native.pack_poolbits(members, 2)
            rc = w.ctx.lib.bgv_verify_accumulate_bits(w.ctx.handle, packed.jobs, 2, packed.sets, 2, None, 0,
                                                      (ctypes.c_uint32 * 2)(*tags), bits, out, outcome, None)
            assert rc == -want, (tags, members)
            assert list(out) == [7, 7] and list(outcome) == [7, 7]
            with pytest.raises(native.BlsGpuError) as e:
                w.ctx.verify_accumulate_bits_async(packed, tags, members)
            assert e.value.code == want
        # the plain call on an entry that has bits
        out, added = (ctypes.c_int32 * 2)(7, 7), (ctypes.c_uint8 * 2)(7, 7)
        rc = w.ctx.lib.bgv_verify_accumulate(w.ctx.handle, packed.jobs, 2, packed.sets, 2, None, 0,
                                             (ctypes.c_uint32 * 2)(251, 250), out, added, None)
        assert rc == -E_ARG and list(out) == [7, 7] and list(added) == [7, 7]
        with pytest.raises(native.BlsGpuError) as e:
            w.ctx.verify_accumulate_async(packed, [250, 250])
        assert e.value.code == E_ARG
        for bad in ((250, 8), (253, 0), (253, native.SIGPOOL_MAX_BITS + 1), (native.MAX_SIGPOOL, 8)):
            rc = w.ctx.lib.bgv_sigpool_open_bits(w.ctx.handle, *bad)
            assert rc == -E_ARG, bad
        # get_bits: an id past the end, a missing output: nothing is written
        buf = ctypes.create_string_buffer(b"\xAA" * 192, 192)
        fb = ctypes.create_string_buffer(b"\xAA" * 512, 512)
        cnt, st, nb = (ctypes.c_uint32 * 2)(7, 7), (ctypes.c_int32 * 2)(7, 7), (ctypes.c_uint32 * 2)(7, 7)
        for idv, bits_arg in (((250, native.MAX_SIGPOOL), fb), ((250, 251), None)):
            rc = w.ctx.lib.bgv_sigpool_get_bits(w.ctx.handle, (ctypes.c_uint32 * 2)(*idv), 2, buf, cnt, st, bits_arg, nb)
            assert rc == -E_ARG
            assert buf.raw == b"\xAA" * 192 and fb.raw == b"\xAA" * 512
            assert list(cnt) == [7, 7] and list(st) == [7, 7] and list(nb) == [7, 7]
        assert w.ctx.sigpool_get_bits(ids) == before and w.ctx.sigpool_launches() == counters
        assert before[0][3:] == (130, field([129], 130)) and before[2] == (-E_IDX, 0, ZERO, 0, b"")
        # the largest field, and a null pool_of_set is the plain call
        w.ctx.sigpool_open(253, native.SIGPOOL_MAX_BITS)
        codes, outcome, _ = step(w, _jobs(w, [5, 6]), [253, 253], [(2048, 2047), (2048, field([0, 2047], 2048))])
        assert outcome == [ADDED, OVERLAP]
        assert w.ctx.sigpool_get_bits([253]) == [(0, 1, w.sigs[5], 2048, field([2047], 2048))]
        out = (ctypes.c_int32 * 2)(7, 7)
        assert w.ctx.lib.bgv_verify_accumulate_bits(w.ctx.handle, packed.jobs, 2, packed.sets, 2, None, 0, None, None,
                                                    out, None, None) == 0
        assert list(out) == [1, 1]
    finally:
        w.ctx.sigpool_drop_range(250, 4)


def test_drop_and_reopen(world):
    w, native = world, world.native
    empty = lambda n: (-native.BGV_E_EMPTY_AGGREGATE, 0, ZERO, n, bytes((n + 7) // 8))
    w.ctx.sigpool_open(260, 16)
    try:
        step(w, _jobs(w, [0, 1]), [260, 260], [(16, 3), (16, 15)])
        assert w.ctx.sigpool_get_bits([260])[0][3:] == (16, b"\x08\x80")
        assert w.ctx.sigpool_drop_range(260, 1) == 1
        assert w.ctx.sigpool_get_bits([260]) == [(-native.BGV_E_BAD_INDEX, 0, ZERO, 0, b"")]
        w.ctx.sigpool_open(260, 16)  # the same size: the bits are clear
        assert w.ctx.sigpool_get_bits([260]) == [empty(16)]
        codes, outcome, _ = step(w, _jobs(w, [2]), [260], [(16, 3)])
        assert outcome == [ADDED] and w.ctx.sigpool_get_bits([260]) == [(0, 1, w.sigs[2], 16, b"\x08\x00")]
        w.ctx.sigpool_drop_range(260, 1)
        w.ctx.sigpool_open(260, 9)  # another size
        assert w.ctx.sigpool_get_bits([260]) == [empty(9)]
        with pytest.raises(native.BlsGpuError) as e:
            w.ctx.verify_accumulate_bits(_jobs(w, [3]), [260], [(16, 3)])
        assert e.value.code == native.BGV_E_ARG
        codes, outcome, _ = step(w, _jobs(w, [3]), [260], [(9, 8)])
        assert outcome == [ADDED] and w.ctx.sigpool_get_bits([260]) == [(0, 1, w.sigs[3], 9, b"\x00\x01")]
        w.ctx.sigpool_drop_range(260, 1)
        w.ctx.sigpool_open(260)  # and as a plain entry: a repeated signature counts again
        assert w.ctx.verify_accumulate(_jobs(w, [3, 3]), [260, 260]) == ([1, 1], [True, True])
        assert w.ctx.sigpool_get_bits([260]) == [(0, 2, expect(w, [w.sigs[3]] * 2), 0, b"")]
    finally:
        w.ctx.sigpool_drop_range(260, 1)


def test_exactly_once_under_concurrency(world):
    """Eight threads each submit the same 64 valid singles into one 64-position entry: per position
    one thread is told added and seven known, and the entry holds each signature once."""
    w = world
    w.ctx.sigpool_open(270, 64)
    results, errors = [None] * 8, []

    def worker(t):
        try:
            results[t] = w.ctx.verify_accumulate_bits(_jobs(w, range(64)), [270] * 64, [(64, k) for k in range(64)])
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    try:
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert all(r[0] == [1] * 64 for r in results)
        for k in range(64):
            per = sorted(r[1][k] for r in results)
            assert per == [ADDED] + [KNOWN] * 7, (k, per)
        assert w.ctx.sigpool_get_bits([270]) == [(0, 64, expect(w, w.sigs[:64]), 64, b"\xff" * 8)]
    finally:
        w.ctx.sigpool_drop_range(270, 1)


def test_async_form(world):
    w = world
    w.ctx.sigpool_open(280, 12)
    try:
        jobs, want = _twelve(w)

        def call(packed, tags, members, mode):
            return w.ctx.verify_accumulate_bits_async(packed, tags, members, mode).wait(60)

        codes, outcome, _ = step(w, jobs, [280] * 12, [(12, k) for k in range(12)], call=call)
        assert codes == want and outcome == [ADDED if c == 1 else NOT_ADDED for c in want]
        pending = [w.ctx.verify_accumulate_bits_async(_jobs(w, [0, 2, 5]), [280] * 3, [(12, 0), (12, 2), (12, 5)])
                   for _ in range(3)]
        got = [p.wait(60) for p in pending]
        assert all(g[0] == [1, 1, 1] for g in got)
        # position 0 is held; 2 and 5 were rejected in the first call: whichever of the three steps
        # runs first adds both
        assert sorted(g[1] for g in got) == [[KNOWN, ADDED, ADDED]] + [[KNOWN] * 3] * 2
        good = [k for k in range(12) if want[k] == 1] + [2, 5]
        assert w.ctx.sigpool_get_bits([280]) == [(0, 10, expect(w, [w.sigs[k] for k in good]), 12, field(good, 12))]
    finally:
        w.ctx.sigpool_drop_range(280, 1)


def test_python_verifier_pool_bits_same_message(world):
    import asyncio

    from lodestar_amd.verifier import BlsGpuVerifier
    w = world
    sets = [(0, w.sigs[0], 0), (3, w.sigs[6], 1), (6, w.sigs[6][:95], 2), (9, w.sigs[9], field([3], 4)),
            (0, w.sigs[0], 0)]
    w.ctx.sigpool_open(290, 4)
    try:
        async def run():
            v = BlsGpuVerifier(ctx=w.ctx)
            return await v.verify_and_pool_bits_same_message(sets, w.roots[0], 290, 4), \
                await v.verify_and_pool_bits_same_message([], w.roots[0], 290, 4)

        assert asyncio.run(run()) == ([(True, "added"), (False, None), (False, None), (True, "added"),
                                       (True, "known")], [])
        assert w.ctx.sigpool_get_bits([290]) == [(0, 2, expect(w, [w.sigs[0], w.sigs[9]]), 4, b"\x09")]
    finally:
        w.ctx.sigpool_drop_range(290, 1)


def test_call_after_close():
    from lodestar_amd import native
    ctx = native.Context()
    try:
        sk = int(_o().interop_secret_key(0)).to_bytes(32, "big")
        ctx.keygen(sk, cache_first=0, want_pubkeys=False)
        msg = hashlib.sha256(b"sig-aggregate root 0").digest()
        sig = ctx.sign(sk, msg)
        jobs = [([native.SetSpec(msg, sig, pk_indices=[0])], True)]
        ctx.sigpool_open(0, 8)
        assert ctx.verify_accumulate_bits(jobs, [0], [(8, 1)]) == ([1], [ADDED])
        assert ctx.sigpool_get_bits([0]) == [(0, 1, sig, 8, b"\x02")]
        assert ctx.sigpool_sum([[0]]) == [(0, 1, sig, 8, b"\x02")]
        assert ctx.lib.bgv_close(ctx.handle) == 0
        calls = [lambda: ctx.sigpool_open(1, 8), lambda: ctx.sigpool_get_bits([0]), lambda: ctx.sigpool_sum([[0]]),
                 lambda: ctx.verify_accumulate_bits(jobs, [0], [(8, 2)]),
                 lambda: ctx.verify_accumulate_bits_async(jobs, [0], [(8, 2)])]
        for call in calls:
            with pytest.raises(native.BlsGpuError) as e:
                call()
            assert e.value.code == native.BGV_E_CLOSED
    finally:
        ctx.close()


# --- bgv_sigpool_sum -----------------------------------------------------------------------------

SIZE_IDS = [16383, 0, 7, 100, 4095, 101]
ONES = list(range(1000, 1064))  # 64 entries of one signature each: entry 1000 + k holds signature k


@pytest.fixture(scope="module")
def filled(world):
    """The six "sizes" entries (1, 2, 63, 64, 65 and 129 signatures: signatures [0, 324)) filled as
    tests/test_gpu_sigpool.py's test_sizes_over_several_calls fills them, and 64 one-signature
    entries.  The sum tests read them and change none."""
    w = world
    case = w.fx["cases"]["sizes"]
    cuts = [(1, 0, 0), (1, 1, 0), (31, 32, 0), (63, 1, 0), (1, 64, 0), (1, 64, 64)]
    pool = Pool(w, SIZE_IDS + ONES)
    for part in range(3):
        ks, tags = [], []
        for (first, count), cut, i in zip(case["runs"], cuts, SIZE_IDS):
            lo = first + sum(cut[:part])
            ks += range(lo, lo + cut[part])
            tags += [i] * cut[part]
        pool.add(_jobs(w, ks), tags)
    pool.add(_jobs(w, range(64)), ONES)
    everything = w.ctx.sigpool_get(SIZE_IDS + ONES)
    yield pool
    assert w.ctx.sigpool_get(SIZE_IDS + ONES) == everything  # no sum changed an entry
    pool.drop()


def _sum_want(w, pool, ids):
    sigs = [s for i in ids for s in pool.held[i]]
    return (0, len(sigs), expect(w, sigs))


def test_sum_of_the_sizes_entries(world, filled, golden):
    w, pool = world, filled
    alone = w.ctx.sigpool_sum([[i] for i in SIZE_IDS])
    assert [g[:3] for g in alone] == w.ctx.sigpool_get(SIZE_IDS)
    assert [g[3:] for g in alone] == [(0, b"")] * 6
    got = w.ctx.sigpool_sum([SIZE_IDS, SIZE_IDS[::-1], SIZE_IDS[2:4]])
    assert got[0] == got[1] == (0, 324, golden[324], 0, b"")
    assert got[0][:3] == _sum_want(w, pool, SIZE_IDS)
    assert got[2][:3] == _sum_want(w, pool, SIZE_IDS[2:4])
    assert w.ctx.sigpool_sum([SIZE_IDS], with_bits=False) == [got[0]]


def test_sum_repeated_id_and_cancellation(world, filled):
    """P + P inside the tree, and {sk} with {r - sk}: the infinity encoding with count 2."""
    w, pool = world, filled
    one = SIZE_IDS[0]
    neg = w.native.SetSpec(w.roots[w.n], w.sigs[w.n], pk_indices=[w.n])
    w.ctx.sigpool_open(300)
    try:
        assert w.ctx.verify_accumulate([([neg], True)], [300]) == ([1], [True])
        got = w.ctx.sigpool_sum([[one, one], [ONES[0], 300], [300, ONES[0], ONES[1]], [7, 7, one, 7]])
        assert got[0][:3] == (0, 2) + (w.oracle_aggregate([w.sigs[0], w.sigs[0]])[1],)
        assert got[1][:3] == (0, 2, INF_SIG)
        assert got[2][:3] == (0, 3, w.sigs[1])
        assert got[3][:3] == _sum_want(w, pool, [7, 7, one, 7]) and got[3][1] == 190
    finally:
        w.ctx.sigpool_drop_range(300, 1)


def test_sum_skips_unwritten_slots(world, filled, golden):
    """An opened-empty entry and a dropped-and-reopened one (its slot still holds the old point) in
    the group change nothing."""
    w = world
    w.ctx.sigpool_open(310)
    w.ctx.sigpool_open(311)
    try:
        assert w.ctx.verify_accumulate(_jobs(w, [400, 401]), [311, 311]) == ([1, 1], [True, True])
        w.ctx.sigpool_drop_range(311, 1)
        w.ctx.sigpool_open(311, 5)
        group = [311, SIZE_IDS[0], 310] + SIZE_IDS[1:] + [310, 311]
        got = w.ctx.sigpool_sum([group, [310, 311], [311, ONES[3], 310]])
        assert got[0] == (0, 324, golden[324], 10, b"\x00\x00")
        assert got[1] == (-w.native.BGV_E_EMPTY_AGGREGATE, 0, ZERO, 5, b"\x00")
        assert got[2] == (0, 1, w.sigs[3], 5, b"\x00")
    finally:
        w.ctx.sigpool_drop_range(310, 2)


def test_sum_of_63_and_64_entries(world, filled, golden):
    w = world
    got = w.ctx.sigpool_sum([ONES[:63], ONES, ONES[::-1], ONES[:1]])
    assert got[0][:3] == (0, 63, golden[63])
    assert got[1][:3] == got[2][:3] == (0, 64, golden[64])
    assert got[3][:3] == (0, 1, w.sigs[0])


def test_sum_twenty_groups_and_statuses(world, filled):
    """Twenty groups over sparse ids in one call, one of them with an id that is not live."""
    w, pool, native = world, filled, world.native
    rnd = random.Random(0x5C0)
    groups = [rnd.sample(SIZE_IDS + ONES, rnd.choice([1, 2, 3, 5, 17, 40])) for _ in range(20)]
    groups[7] = groups[7] + [5000]  # never opened
    groups[12] = [ONES[5]] * 64
    got = w.ctx.sigpool_sum(groups)
    dev = w.ctx.aggregate_signatures([[s for i in g for s in pool.held.get(i, [])] for g in groups])
    for k, g in enumerate(groups):
        if k == 7:
            assert got[k] == (-native.BGV_E_BAD_INDEX, 0, ZERO, 0, b"")
            continue
        assert got[k] == (0, sum(len(pool.held[i]) for i in g), dev[k][1], 0, b"") and dev[k][0] == 0, k
    assert w.ctx.sigpool_sum([]) == []


def test_sum_bits(world, filled):
    """130 | 5 | 128 with a plain entry between them, an empty subnet, and an all-empty group."""
    w, native = world, world.native
    for i, n in ((320, 130), (321, 5), (322, 128), (323, 128)):
        w.ctx.sigpool_open(i, n)
    try:
        pa, pb, pc = [0, 64, 129], [0, 4], [0, 1, 127]
        ks = list(range(8))
        tags = [320] * 3 + [321] * 2 + [322] * 3
        codes, outcome, _ = step(w, _jobs(w, ks), tags, [(130, p) for p in pa] + [(5, p) for p in pb] +
                                 [(128, p) for p in pc])
        assert outcome == [ADDED] * 8
        plain = ONES[9]
        got = w.ctx.sigpool_sum([[320, plain, 321, 322], [322, 323, 321], [323], [323, 323]])
        want = field(pa + [130 + p for p in pb] + [135 + p for p in pc], 263)
        assert got[0] == (0, 9, expect(w, w.sigs[:8] + [w.sigs[9]])[:96], 263, want)
        assert got[1] == (0, 5, expect(w, w.sigs[3:8]), 261, field(pc + [256 + p for p in pb], 261))
        empty = -native.BGV_E_EMPTY_AGGREGATE
        assert got[2] == (empty, 0, ZERO, 128, bytes(16)) and got[3] == (empty, 0, ZERO, 256, bytes(32))
        # the stride: 33 bytes hold 263 bits, 32 do not; the rest of a stride is zeroed
        assert w.ctx.sigpool_sum([[320, plain, 321, 322]], bits_stride=33) == [got[0]]
        gs = (native.BgvPoolGroup * 1)()
        arr = (ctypes.c_uint32 * 4)(320, plain, 321, 322)
        gs[0].ids, gs[0].n_ids = ctypes.cast(arr, ctypes.c_void_p), 4
        out = ctypes.create_string_buffer(b"\xAA" * 96, 96)
        fb = ctypes.create_string_buffer(b"\xAA" * 40, 40)
        cnt, st, nb = (ctypes.c_uint32 * 1)(7), (ctypes.c_int32 * 1)(7), (ctypes.c_uint32 * 1)(7)
        untouched = lambda: (out.raw == b"\xAA" * 96 and fb.raw == b"\xAA" * 40 and
                             (cnt[0], st[0], nb[0]) == (7, 7, 7))
        sum_ = w.ctx.lib.bgv_sigpool_sum
        assert sum_(w.ctx.handle, gs, 1, out, cnt, st, fb, 32, nb) == -native.BGV_E_ARG and untouched()
        assert sum_(w.ctx.handle, gs, 65537, out, cnt, st, None, 0, nb) == -native.BGV_E_ARG and untouched()
        assert sum_(w.ctx.handle, gs, 1, None, cnt, st, fb, 40, nb) == -native.BGV_E_ARG and untouched()
        assert sum_(w.ctx.handle, gs, 1, out, cnt, st, fb, 40, None) == -native.BGV_E_ARG and untouched()
        assert sum_(w.ctx.handle, None, 1, out, cnt, st, fb, 40, nb) == -native.BGV_E_ARG and untouched()
        gs[0].n_ids = 0
        assert sum_(w.ctx.handle, gs, 1, out, cnt, st, fb, 40, nb) == -native.BGV_E_ARG and untouched()
        gs[0].n_ids = 4
        arr[2] = native.MAX_SIGPOOL
        assert sum_(w.ctx.handle, gs, 1, out, cnt, st, fb, 40, nb) == -native.BGV_E_ARG and untouched()
        arr[2] = 321
        long_ids = (ctypes.c_uint32 * 65)(*([320] * 65))
        gs[0].ids, gs[0].n_ids = ctypes.cast(long_ids, ctypes.c_void_p), 65
        assert sum_(w.ctx.handle, gs, 1, out, cnt, st, fb, 40, nb) == -native.BGV_E_ARG and untouched()
        gs[0].ids, gs[0].n_ids = ctypes.cast(arr, ctypes.c_void_p), 4
        assert sum_(w.ctx.handle, gs, 1, out, cnt, st, fb, 40, nb) == 0
        assert (st[0], cnt[0], out.raw, nb[0]) == got[0][:4] and fb.raw == want + bytes(7)
        assert w.ctx.sigpool_get_bits([320, 321, 322, 323])[0][3:] == (130, field(pa, 130))
    finally:
        w.ctx.sigpool_drop_range(320, 4)
