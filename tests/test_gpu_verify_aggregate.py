"""GPU tests of bgv_verify_aggregate (include/blsgpu.h): a verify call that also returns, per
caller-chosen aggregate, the compressed sum of the signatures it accepted (bgv_sigagg_plan.h,
bgv_k_sigagg.hip).

Keys and signatures come from bgv_keygen and bgv_sign.  Every expected aggregate is computed twice,
by oracle.bls12381.signatures_aggregate of the accepted subset and by Context.aggregate_signatures
of the same subset, and all three must be byte-equal; the codes must equal verify_jobs' on the same
input under the same set_rng_seed.  The oracle decodes and subgroup-checks ~8 signatures a second,
so its aggregates of the large cases (324, BGV_SIGAGG_WAVE_MAX and BGV_SIGAGG_WAVE_MAX + 1
signatures) are recorded in tests/golden/sig_aggregate.json (tools/gen_golden_sig_aggregate.py,
signatures_aggregate over the same, deterministic, signatures: the digest of bgv_sign's output is
compared with the fixture's) and the small cases call it here.
"""
import ctypes
import hashlib
import json
import os

import pytest

from tests import committeesim as cs
from tests import sig_edges as se

pytestmark = pytest.mark.gpu

SEED = 0x5161A66
INF_SIG = bytes([0xC0]) + bytes(95)
ZERO = bytes(96)
NO_AGG = 0xFFFFFFFF


def _o():
    from oracle import bls12381 as o  # secret keys and expected aggregates; never the code under test
    return o


def _root(k):
    return hashlib.sha256(b"sig-aggregate root %d" % (k % 3)).digest()  # tools/gen_golden_sig_aggregate.py


class World:
    """One context holding the fixture's keys (interop secret key k at index k), key n = r - sk_0,
    and signature k = sk_k over _root(k)."""

    def __init__(self):
        from lodestar_amd import native
        o = _o()
        self.native = native
        with open(os.path.join(se.GOLD, "sig_aggregate.json")) as f:
            self.fx = json.load(f)
        assert self.fx["wave_max"] == native.SIGAGG_WAVE_MAX, "regenerate tests/golden/sig_aggregate.json"
        self.n = n = self.fx["n"]
        self.sks = [o.interop_secret_key(k) for k in range(n)] + [(o.R - o.interop_secret_key(0)) % o.R]
        self.ctx = native.Context()
        skb = b"".join(int(s).to_bytes(32, "big") for s in self.sks)
        self.ctx.keygen(skb, cache_first=0, want_pubkeys=False)
        self.roots = [_root(k) for k in range(n)] + [_root(0)]
        raw = self.ctx.sign(skb, b"".join(self.roots))
        self.sigs = [raw[96 * k:96 * k + 96] for k in range(n + 1)]
        assert hashlib.sha256(b"".join(self.sigs[:n])).hexdigest() == self.fx["sigs_sha256"]
        self.oracle_cache = {}

    def good(self, k):
        """The valid single-key set of signature k."""
        return self.native.SetSpec(self.roots[k], self.sigs[k], pk_indices=[k])

    def sign(self, sk, msg):
        return self.ctx.sign(int(sk).to_bytes(32, "big"), msg)

    def oracle_aggregate(self, sigs):
        key = hashlib.sha256(b"".join(sigs)).digest()
        if key not in self.oracle_cache:
            self.oracle_cache[key] = _o().signatures_aggregate(list(sigs))
        return self.oracle_cache[key]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def check_call(w, jobs, tags, naggs, mode=0, golden=None, call=None, form=None):
    """form: the decoding form the aggregation step must launch, "wave", "lane" or "none" (read
    from the library's launch counters).  Runs verify_jobs and verify_aggregate on the same input under the same seed and checks the
    codes against each other and every aggregate against both references of the accepted subset
    (golden: the recorded oracle aggregates, where the subsets are the fixture's).  Returns
    (codes, aggregates)."""
    native = w.native
    packed = native.PackedCall(jobs)
    w.ctx.set_rng_seed(SEED)
    want_codes = w.ctx.verify_jobs(packed, mode)
    w.ctx.set_rng_seed(SEED)
    before = w.ctx.sigagg_launches()
    codes, aggs = (call or w.ctx.verify_aggregate)(packed, tags, naggs, mode)
    assert codes == want_codes
    if form is not None:
        after = w.ctx.sigagg_launches()
        assert (after[0] - before[0], after[1] - before[1]) == {"wave": (1, 0), "lane": (0, 1), "none": (0, 0)}[form]
    subsets, i = [[] for _ in range(naggs)], 0
    for (sets, _), code in zip(jobs, want_codes):
        for s in sets:
            if code == 1 and tags[i] != NO_AGG:
                subsets[tags[i]].append(s.sig)
            i += 1
    dev = w.ctx.aggregate_signatures(subsets)
    for a, sub in enumerate(subsets):
        status, count, got = aggs[a]
        assert count == len(sub), a
        if not sub:
            assert (status, got) == (-native.BGV_E_EMPTY_AGGREGATE, ZERO), a
            assert dev[a] == (-native.BGV_E_EMPTY_AGGREGATE, ZERO)
            continue
        want = bytes.fromhex(golden[a]) if golden is not None else None
        if want is None:
            code, want = w.oracle_aggregate(sub)
            assert code == 0
        assert status == 0, a
        assert got == want, a
        assert dev[a] == (0, want), a
    return codes, aggs


def _fixture_jobs(w, case):
    """The fixture case as batchable one-set jobs in signature order; a set's tag is its run."""
    jobs, tags = [], []
    for a, (first, count) in enumerate(case["runs"]):
        for k in range(first, first + count):
            jobs.append(([w.good(k)], True))
            tags.append(a)
    return jobs, tags


def test_aggregate_sizes(world):
    """Aggregates of 1, 2, 63, 64, 65 and 129 signatures in one call: the strided loop of the sum
    with none, one and three terms per lane and a tree with idle lanes; 324 signatures are below
    BGV_SIGAGG_WAVE_MAX and decode one per wavefront."""
    case = world.fx["cases"]["sizes"]
    assert [c for _, c in case["runs"]] == [1, 2, 63, 64, 65, 129]
    jobs, tags = _fixture_jobs(world, case)
    assert 324 <= world.native.SIGAGG_WAVE_MAX
    codes, _ = check_call(world, jobs, tags, 6, golden=case["aggregates"], form="wave")
    assert codes == [1] * 324


@pytest.mark.parametrize("name", ["wave_max", "wave_max_plus_1"])
def test_both_decoding_forms(world, name):
    """BGV_SIGAGG_WAVE_MAX accepted signatures decode one per wavefront, one more one per lane:
    the library's launch counters say which kernel ran, with nothing set in the environment."""
    assert "BGV_SIGAGG_WAVE_MAX" not in os.environ
    case = world.fx["cases"][name]
    want = world.native.SIGAGG_WAVE_MAX + (name == "wave_max_plus_1")
    assert case["runs"] == [[0, want]]
    jobs, tags = _fixture_jobs(world, case)
    codes, aggs = check_call(world, jobs, tags, 1, golden=case["aggregates"],
                             form="lane" if name == "wave_max_plus_1" else "wave")
    assert codes == [1] * want and aggs[0][1] == want


def _edge(name):
    return next(e for e in se.corpus() if e["name"] == name)


def _twelve(w):
    """Twelve one-set jobs for one aggregate, four of them bad: a wrong signer (its group fails and
    goes through the retry rounds), a 95-byte signature, an off-curve one and one outside G2."""
    bad = {
        2: (w.native.SetSpec(w.roots[2], w.sigs[5], pk_indices=[2]), 0),
        5: (w.native.SetSpec(w.roots[5], _edge("len_95")["sig"], pk_indices=[5]), -8),
        6: (w.native.SetSpec(w.roots[6], _edge("x0_sort0")["sig"], pk_indices=[6]), -2),
        9: (w.native.SetSpec(w.roots[9], _edge("small_13")["sig"], pk_indices=[9]), -3),
    }
    jobs = [([bad[k][0] if k in bad else w.good(k)], True) for k in range(12)]
    return jobs, [bad[k][1] if k in bad else 1 for k in range(12)]


@pytest.mark.parametrize("mode", [0, 1], ids=["worker", "per_job"])
def test_bad_sets_are_left_out(world, mode):
    """The bad sets are absent from the sum and from the count; the valid sets that came through the
    retry rounds behind the wrong signer are in it."""
    jobs, want = _twelve(world)
    codes, aggs = check_call(world, jobs, [0] * 12, 1, mode)
    assert codes == want
    assert aggs[0][:2] == (0, 8)


def test_rejected_aggregate_is_empty(world):
    """An aggregate all of whose sets are rejected beside one that has members, then a call that
    accepts nothing at all (no device work)."""
    w, native = world, world.native
    wrong = [([native.SetSpec(w.roots[k], w.sigs[k + 1], pk_indices=[k])], True) for k in (0, 3)]
    jobs = [wrong[0], ([w.good(1)], True), wrong[1], ([w.good(2)], True)]
    codes, aggs = check_call(w, jobs, [1, 0, 1, 0], 2, form="wave")
    assert codes == [0, 1, 0, 1]
    assert aggs[1] == (-native.BGV_E_EMPTY_AGGREGATE, 0, ZERO) and aggs[0][:2] == (0, 2)
    codes, aggs = check_call(w, wrong, [0, 1], 2, form="none")
    assert codes == [0, 0]
    assert aggs == [(-native.BGV_E_EMPTY_AGGREGATE, 0, ZERO)] * 2


def test_sum_at_infinity(world):
    """Secret keys s and r - s on one root: both sets are accepted and their signatures cancel."""
    w = world
    neg = w.native.SetSpec(w.roots[w.n], w.sigs[w.n], pk_indices=[w.n])
    codes, aggs = check_call(w, [([w.good(0)], True), ([neg], True)], [0, 0], 1)
    assert codes == [1, 1]
    assert aggs[0] == (0, 2, INF_SIG)


@pytest.mark.parametrize("mode", [0, 1], ids=["worker", "per_job"])
def test_untagged_and_interleaved(world, mode):
    """Untagged sets beside tagged ones, two aggregates with interleaved members and a repeated
    signature, which counts again."""
    w = world
    order = [0, 1, 2, 3, 4, 1, 5, 6, 7, 1]
    jobs = [([w.good(k)], True) for k in order]
    tags = [0, 1, NO_AGG, 0, 1, 1, NO_AGG, 1, 0, 1]
    codes, aggs = check_call(w, jobs, tags, 2, mode)
    assert codes == [1] * 10
    assert [a[1] for a in aggs] == [3, 5]


def test_multi_set_job_splits_over_aggregates(world):
    """A 3-set non-batchable job whose sets go to two aggregates, and one with a wrong signer among
    its sets, none of which is accepted."""
    w, native = world, world.native
    ok = ([w.good(0), w.good(1), w.good(2)], False)
    bad = ([w.good(3), native.SetSpec(w.roots[4], w.sigs[5], pk_indices=[4]), w.good(6)], False)
    codes, aggs = check_call(w, [ok, bad], [0, 1, 0, 0, 1, 1], 2)
    assert codes == [1, 0]
    assert [a[1] for a in aggs] == [2, 1]


def test_committee_and_span_sets(world):
    """A committee-bitfield set and a span set carrying tags (the spans argument), beside a plain set."""
    w, native = world, world.native
    o = _o()
    a, b = [1, 2, 3, 4], [5, 6, 7]
    w.ctx.committee_put(100, a)
    w.ctx.committee_put(101, b)
    try:
        msg = hashlib.sha256(b"sig-aggregate committees").digest()
        sk_com = (w.sks[1] + w.sks[3] + w.sks[4]) % o.R  # positions 0, 2, 3 of a
        sk_span = (w.sks[2] + w.sks[5] + w.sks[7]) % o.R  # position 1 of a; 0 and 2 of b
        com = native.SetSpec(msg, w.sign(sk_com, msg), committee=100, bits=cs.pack([0, 2, 3], 4), n_bits=4)
        span = native.SetSpec(msg, w.sign(sk_span, msg), committees=[100, 101], bits=cs.pack([1, 4, 6], 7), n_bits=7)
        for sets in ([com, w.good(0)], [com, span, w.good(0)]):  # the pkbits form alone, then with a span
            jobs = [([s], True) for s in sets]
            codes, aggs = check_call(w, jobs, [0] * len(sets), 1)
            assert codes == [1] * len(sets) and aggs[0][1] == len(sets)
    finally:
        w.ctx.committee_drop(100)
        w.ctx.committee_drop(101)


def test_bad_tag_runs_nothing(world):
    """A tag that is neither BGV_NO_AGG nor below naggs: -BGV_E_ARG, every output untouched."""
    w, native = world, world.native
    packed = native.PackedCall([([w.good(0)], True), ([w.good(1)], True)])
    for tags, naggs in (([0, 2], 2), ([0, 0xFFFFFFFE], 2), ([0, 0], (1 << 20) + 1)):
        out = (ctypes.c_int32 * 2)(7, 7)
        agg = ctypes.create_string_buffer(b"\xAA" * 192, 192)
        ast = (ctypes.c_int32 * 2)(7, 7)
        cnt = (ctypes.c_uint32 * 2)(7, 7)
        rc = w.ctx.lib.bgv_verify_aggregate(w.ctx.handle, packed.jobs, 2, packed.sets, 2, None, 0,
                                            (ctypes.c_uint32 * 2)(*tags), naggs, out, agg, ast, cnt, None)
        assert rc == -native.BGV_E_ARG
        assert list(out) == [7, 7] and agg.raw == b"\xAA" * 192 and list(ast) == [7, 7] and list(cnt) == [7, 7]
    with pytest.raises(native.BlsGpuError) as e:
        w.ctx.verify_aggregate(packed, [0, 5], 2)
    assert e.value.code == native.BGV_E_ARG
    # naggs == 0 is the plain call
    assert w.ctx.verify_aggregate(packed, [NO_AGG, NO_AGG], 0) == ([1, 1], [])


def test_async_form(world):
    """The asynchronous form: the aggregates are filled when done() fires."""
    w = world
    jobs, want = _twelve(w)

    def call(packed, tags, naggs, mode):
        return w.ctx.verify_aggregate_async(packed, tags, naggs, mode).wait(60)

    codes, aggs = check_call(w, jobs, [0, 1] * 6, 2, call=call)
    assert codes == want
    assert [a[1] for a in aggs] == [4, 4]


def test_python_verifier_same_message(world):
    """verifier.BlsGpuVerifier's same-message methods: one bool per set, an undecodable signature
    False for its set, and the aggregate of the accepted ones (None when there is none)."""
    import asyncio

    from lodestar_amd.verifier import BlsGpuVerifier
    w = world
    ks = [0, 3, 6, 9]  # signers of one root
    assert len({w.roots[k] for k in ks}) == 1
    sets = [(k, w.sigs[k]) for k in ks]
    sets[1] = (3, w.sigs[6])  # a wrong signer
    sets[2] = (6, w.sigs[6][:95])  # undecodable

    async def run():
        v = BlsGpuVerifier(ctx=w.ctx)
        plain = await v.verify_signature_sets_same_message(sets, w.roots[0])
        both = await v.verify_and_aggregate_same_message(sets, w.roots[0])
        none = await v.verify_and_aggregate_same_message(sets[1:3], w.roots[0])
        return plain, both, none

    plain, (results, sig), none = asyncio.run(run())
    assert plain == results == [True, False, False, True]
    assert (0, sig) == w.oracle_aggregate([w.sigs[0], w.sigs[9]])
    assert none == ([False, False], None)


def test_call_after_close():
    from lodestar_amd import native
    ctx = native.Context()
    try:
        sk = int(_o().interop_secret_key(0)).to_bytes(32, "big")
        ctx.keygen(sk, cache_first=0, want_pubkeys=False)
        msg = _root(0)
        jobs = [([native.SetSpec(msg, ctx.sign(sk, msg), pk_indices=[0])], True)]
        assert ctx.verify_aggregate(jobs, [0], 1)[0] == [1]
        assert ctx.lib.bgv_close(ctx.handle) == 0
        for call in (ctx.verify_aggregate, ctx.verify_aggregate_async):
            with pytest.raises(native.BlsGpuError) as e:
                call(jobs, [0], 1)
            assert e.value.code == native.BGV_E_CLOSED
    finally:
        ctx.close()
