"""GPU tests of the span sets (include/blsgpu.h bgv_verify_spans, bgv_aggregate_span): a set lays
one participation bitfield over several device-resident committees and the device sums, per
committee, the shorter side (k_pk_agg_span, bgv_pk_bits.h).  Expected aggregates are the oracle's
(tests/golden/multi_committee.json); verdicts are checked against signatures made with the sum
of the participants' secret keys and against the same sets given as index lists.
"""
import hashlib

import pytest

from tests import committeesim as cs
from tests import multicomsim as ms
from tests.test_gpu_committee_bits import INF96, World, _o, _sk_bytes, _sks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = World()
    w.mfx = ms.fixture()
    yield w
    w.close()


def span_set(w, msg, sig, ids, lens, per):
    """A set over committees ids (lengths lens) with per[c] the positions selected in committee c."""
    pos, off = [], 0
    for n, sel in zip(lens, per):
        pos += [off + p for p in sel]
        off += n
    return w.native.SetSpec(msg, sig, committees=list(ids), bits=cs.pack(pos, off), n_bits=off)


def case_set(w, c, msg, sig, bits=None):
    return w.native.SetSpec(msg, sig, committees=[w.ids[n] for n in c["committees"]],
                            bits=bytes.fromhex(c["bits"]) if bits is None else bits, n_bits=c["n_bits"])


def case_sk(w, c):
    return sum(w.sks[i] for i in ms.expand(c)) % w.R


def test_aggregates_match_oracle(world):
    """Every fixture case: unaligned committee edges, a repeated id, direct / complement / empty /
    full committees together, 64 committees, M on both sides of the team and wave switches, bits in
    the last word only, infinity totals and infinity results."""
    w, bad = world, []
    for c in w.mfx["cases"]:
        got = w.ctx.aggregate_span([w.ids[n] for n in c["committees"]], bytes.fromhex(c["bits"]), c["n_bits"])
        if got.hex() != c["agg"]:
            bad.append(c["name"])
        idx = ms.expand(c)
        if len(set(idx)) == len(idx) and w.ctx.aggregate_pubkeys(idx) != got:
            bad.append(c["name"] + " (index form)")
    assert not bad, bad
    # one listed committee is the committee form itself
    one = w.fx["cases"][5]
    assert w.ctx.aggregate_span([w.ids[one["committee"]]], bytes.fromhex(one["bits"]), one["n"]).hex() == one["agg"]


def _flip(c):
    """The case's bitfield with one participant's bit cleared (or one added where one takes part)."""
    b = bytearray.fromhex(c["bits"])
    on = [p for p in range(c["n_bits"]) if (b[p >> 3] >> (p & 7)) & 1]
    p = on[len(on) // 2] if len(on) > 1 else (on[0] + 1) % c["n_bits"]
    b[p >> 3] ^= 1 << (p & 7)
    return bytes(b)


def _verdict_jobs(w):
    cases = [c for c in w.mfx["cases"] if c["agg"] != INF96.hex()]
    msgs = [hashlib.sha256(b"span " + c["name"].encode()).digest() for c in cases]
    sigs = w.ctx.sign(b"".join(_sk_bytes(case_sk(w, c)) for c in cases), b"".join(msgs))
    sj, ij, want, small = [], [], [], []
    for i, c in enumerate(cases):
        if c["name"] in ("m16", "m17", "m48", "m49"):
            small += [len(sj), len(sj) + 1]
        sig = sigs[96 * i:96 * i + 96]
        for bits, code in ((bytes.fromhex(c["bits"]), 1), (_flip(c), 0)):
            sj.append(([case_set(w, c, msgs[i], sig, bits)], False))
            ij.append(([w.native.SetSpec(msgs[i], sig, pk_indices=ms.expand(dict(c, bits=bits.hex())))], False))
            want.append(code)
    return sj, ij, want, small


@pytest.mark.parametrize("mode", [0, 1], ids=["worker", "per_job"])
def test_verdicts(world, mode):
    """Valid, and 0 with one wrong bit, per finite fixture case as one-set jobs in one call; then
    the cases around M = 16 and M = 48 / 49 as calls of their own: the smallest calls' path, where
    a block sums the set and 49 terms switch from the 16-lane team to the wave."""
    sj, ij, want, small = _verdict_jobs(world)
    got = world.ctx.verify_jobs(sj, mode)
    assert got == want
    assert world.ctx.verify_jobs(ij, mode) == got  # the expanded index lists decide the same
    for i in small:
        assert world.ctx.verify_jobs([sj[i]], mode) == [want[i]], i


def test_infinity_aggregates(world):
    """A one-set job whose aggregate is infinity is false, a two-set job BLST_PK_IS_INFINITY."""
    w, native = world, world.native
    msg = hashlib.sha256(b"span inf").digest()
    sig = w.ctx.sign(_sk_bytes(w.sks[3]), msg)
    good = native.SetSpec(msg, sig, pk_indices=[3])
    for c in (c for c in w.mfx["cases"] if c["agg"] == INF96.hex()):
        inf = case_set(w, c, msg, sig)
        for mode in (native.MODE_WORKER, native.MODE_PER_JOB):
            got = w.ctx.verify_jobs([([inf], False), ([good, inf], False), ([good], False)], mode)
            assert got == [0, -native.BLST_PK_IS_INFINITY, 1], (c["name"], mode)


def test_error_codes(world):
    """Each argument error as its job's code, in the documented order of the checks."""
    w, native = world, world.native
    msg = hashlib.sha256(b"span errors").digest()
    a, b = w.ids["n17"], w.ids["n33"]
    sig = w.ctx.sign(_sk_bytes(w.sks[0]), msg)
    S = lambda ids, bits, n: native.SetSpec(msg, sig, committees=ids, bits=bits, n_bits=n)  # noqa: E731
    big = w.put([i % 521 for i in range(65536)])
    jobs = [
        S([a, 9999], cs.pack([0], 50), 50),                      # an unknown id
        S([a] * 65 + [9999], cs.pack([0], 3), 3),                # ... which comes before the count and n_bits
        S([w.ids["n1"]] * 65, cs.pack([0], 65), 65),             # more than 64 committees
        S([big] * 3, cs.pack([0], 3 * 65536), 3 * 65536),        # more than BGV_MAX_SPAN_BITS bits
        S([a, b], cs.pack([0], 49), 49),                         # n_bits is not 17 + 33
        S([a, b], bytes(6) + bytes([0x04]), 50),                 # a set bit at bit 50, nothing else
        S([a, b], bytes(7), 50),                                 # no bit set
        S([a, b], cs.pack([16, 17], 50), 50),                    # fine: the last of n17, the first of n33
    ]
    got = w.ctx.verify_jobs([([s], False) for s in jobs])
    E = native
    assert got == [-E.BGV_E_BAD_INDEX, -E.BGV_E_BAD_INDEX, -E.BGV_E_ARG, -E.BGV_E_ARG, -E.BGV_E_ARG, -E.BGV_E_ARG,
                   -E.BGV_E_EMPTY_AGGREGATE, 0]
    with pytest.raises(native.BlsGpuError) as e:
        w.ctx.aggregate_span([a, b], bytes(7), 50)
    assert e.value.code == native.BGV_E_EMPTY_AGGREGATE


def test_mixed_worker_call_with_retry(world):
    """One worker-mode call of batchable jobs mixing span, one-committee, index and single sets,
    some corrupted: the codes are those of the same call with every set expanded to indices."""
    w, native = world, world.native
    fxc = w.fx["committees"]
    names = ["n16", "n17", "n31", "n32", "n33", "n64", "n65", "n15"]
    plan, sk = [], []
    for j in range(96):
        kind = j % 4
        if kind == 0:  # a span of 2..4 committees, participation from sparse to full
            cn = [names[(j + q) % 8] for q in range(2 + j % 3)]
            per = [[p for p in range(len(fxc[n])) if (p * 7 + j + q) % (2 + j % 5) != 0] for q, n in enumerate(cn)]
            idx = [fxc[n][p] for n, sel in zip(cn, per) for p in sel]
            plan.append(("span", cn, per, idx))
        elif kind == 1:
            n = names[j % 8]
            sel = [p for p in range(len(fxc[n])) if (p + j) % 3]
            plan.append(("com", n, sel, [fxc[n][p] for p in sel]))
        elif kind == 2:
            plan.append(("idx", None, None, [(j + 11 * q) % 520 for q in range(1 + j % 9)]))
        else:
            plan.append(("single", None, None, [j]))
        sk.append(sum(w.sks[i] for i in plan[-1][3]) % w.R)
    msgs = [hashlib.sha256(b"span mixed %d" % j).digest() for j in range(96)]
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))
    wrong = {8, 41, 42, 77}  # a span, a one-committee, an index and another one-committee set
    sj, ij = [], []
    for j, (kind, cn, per, idx) in enumerate(plan):
        sig = sigs[96 * (j - 1):96 * j] if j in wrong else sigs[96 * j:96 * j + 96]
        if kind == "span":
            s = span_set(w, msgs[j], sig, [w.ids[n] for n in cn], [len(fxc[n]) for n in cn], per)
        elif kind == "com":
            s = native.SetSpec(msgs[j], sig, committee=w.ids[cn], bits=cs.pack(per, len(fxc[cn])), n_bits=len(fxc[cn]))
        else:
            s = native.SetSpec(msgs[j], sig, pk_indices=idx)
        sj.append(([s], True))
        ij.append(([native.SetSpec(msgs[j], sig, pk_indices=idx)], True))
    st = native.BgvStats()
    got = w.ctx.verify_jobs(sj, native.MODE_WORKER, st)
    assert got == [0 if j in wrong else 1 for j in range(96)]
    assert st.batch_retries >= 1
    assert w.ctx.verify_jobs(ij, native.MODE_WORKER) == got


BLOCK_COMS = ["n16", "n17", "n31", "n32", "n33", "n64", "n65", "n32"]  # 16..65 members each


def _block(w, participation, flip=False):
    """A block-shaped call: 8 attestation sets each spanning 8 committees, the 512-member sync
    aggregate as a one-committee set and two single-key sets, one non-batchable job of 11 sets."""
    native, fxc = w.native, w.fx["committees"]
    msgs = [hashlib.sha256(b"span block %d" % j).digest() for j in range(11)]

    def present(j, n):
        gone = {(j * 7 + 13 * q) % n for q in range(n * (100 - participation) // 100)}
        return [p for p in range(n) if p not in gone]

    spans, sk = [], []
    for j in range(8):
        cn = BLOCK_COMS[j:] + BLOCK_COMS[:j]
        per = [present(j + q, len(fxc[n])) for q, n in enumerate(cn)]
        spans.append((cn, per))
        sk.append(sum(w.sks[fxc[n][p]] for n, sel in zip(cn, per) for p in sel) % w.R)
    sync = present(1, 512)
    sk += [w.sum_sk(fxc["n512"], sync), w.sks[11], w.sks[12]]
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))
    sg = lambda j: sigs[96 * j:96 * j + 96]  # noqa: E731
    if flip:
        spans[5][1][3] = spans[5][1][3][:-1]
    sets = [span_set(w, msgs[j], sg(j), [w.ids[n] for n in cn], [len(fxc[n]) for n in cn], per)
            for j, (cn, per) in enumerate(spans)]
    sets.append(native.SetSpec(msgs[8], sg(8), committee=w.ids["n512"], bits=cs.pack(sync, 512), n_bits=512))
    sets += [native.SetSpec(msgs[9], sg(9), pk_indices=[11]), native.SetSpec(msgs[10], sg(10), pk_indices=[12])]
    return [(sets, False)]


@pytest.mark.parametrize("participation", [100, 95, 50])
def test_block_import_latency_path(world, participation):
    """11 sets are 64 slots and one group: far below BGV_PREP_WIDE_MAX = 340 slots, so
    bgv_launch_prep takes the wide branch, where k_pk_agg_span runs a block per span set ahead of
    k_prep_wide and pk_bits_one sums the sync set.  A span here has 290 members: 8 totals at
    100 % (a team), 8 totals and ~12 absentees at 95 %, ~145 terms at 50 % (the wave, from
    BGV_PK_ONE_WAVE_MIN = 49 terms)."""
    assert world.ctx.verify_jobs(_block(world, participation), world.native.MODE_WORKER) == [1]
    assert world.ctx.verify_jobs(_block(world, participation, flip=True), world.native.MODE_WORKER) == [0]


def test_block_import_split_over_devices():
    """The same call on a context over two device entries with the split threshold below its
    size: each device's run of sets carries its spans, same code."""
    w = World([0, 0])
    try:
        w.ctx.set_split(4)
        assert w.ctx.verify_jobs(_block(w, 95), w.native.MODE_WORKER) == [1]
        assert w.ctx.verify_jobs(_block(w, 95, flip=True), w.native.MODE_WORKER) == [0]
    finally:
        w.close()


def test_bulk_path(world):
    """16,640 one-set batchable jobs, each a span of two 16-member committees: 16,640 slots + 260
    groups exceed bgv_latency_max() = 16,384 pairs, so the batch takes bgv_launch_prep's bulk
    branch (k_pk_agg_span on teams, four sets per block, before k_prep).  All valid, then one set
    with a wrong bit: exactly its job fails."""
    w, native = world, world.native
    N = 16640
    coms = [[(11 * c + 3 * i) % 520 for i in range(16)] for c in range(32)]
    ids = [w.put(m) for m in coms]
    msgs, per, sk = [], [], []
    for j in range(N):
        msgs.append(hashlib.sha256(b"span bulk %d" % j).digest())
        ka, kb = (j * 7) % 17, 1 + (j * 5) % 16  # 0..16 and 1..16 participants: every side, empty and full
        pa, pb = sorted((j + 5 * q) % 16 for q in range(ka)), sorted((j + 3 * q) % 16 for q in range(kb))
        per.append((pa, pb))
        a, b = coms[j % 32], coms[(j + 7) % 32]
        sk.append((sum(w.sks[a[p]] for p in pa) + sum(w.sks[b[p]] for p in pb)) % w.R)
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))

    def jobs(wrong=None):
        out = []
        for j in range(N):
            pa, pb = per[j]
            if j == wrong:
                pb = pb[1:] if len(pb) > 1 else sorted(pb + [(pb[0] + 1) % 16])
            out.append(([span_set(w, msgs[j], sigs[96 * j:96 * j + 96], [ids[j % 32], ids[(j + 7) % 32]], [16, 16],
                                  [pa, pb])], True))
        return out

    assert w.ctx.verify_jobs(jobs(), native.MODE_WORKER) == [1] * N
    got = w.ctx.verify_jobs(jobs(12345), native.MODE_WORKER)
    assert [j for j in range(N) if got[j] != 1] == [12345] and got[12345] == 0


def test_lifecycle():
    """A drop of one listed committee rejects later sets with BAD_INDEX; a pubkey overwrite of a
    member changes the aggregate of a complement committee in a span; a listed committee that
    holds a marked key rejects."""
    from lodestar_amd import native
    o = _o()
    fx, sks = cs.fixture(), _sks()
    c = native.Context()
    try:
        c.pubkeys_put(0, b"".join(bytes.fromhex(k) for k in fx["keys"][:16]))
        c.committee_put(3, [0, 1, 2, 3, 4])
        c.committee_put(4, [5, 6, 7])
        c.committee_put(5, [8, 9])
        bits = cs.pack([0, 1, 2, 3, 5, 8, 9], 10)  # 4 of 5 (complement), 1 of 3 (direct), 2 of 2 (the total)
        want = o.g1_serialize(o.g1_mul(o.G1, sum(sks[i] for i in (0, 1, 2, 3, 5, 8, 9)) % o.R))
        assert c.aggregate_span([3, 4, 5], bits, 10) == want
        c.pubkeys_put(2, bytes.fromhex(fx["keys"][300]))  # index 2 now holds key 300
        new = [sks[0], sks[1], sks[300], sks[3], sks[5], sks[8], sks[9]]
        want = o.g1_serialize(o.g1_mul(o.G1, sum(new) % o.R))
        assert c.aggregate_span([3, 4, 5], bits, 10) == want  # the complement committee's new total
        msg = hashlib.sha256(b"span lifecycle").digest()
        sig = c.sign(_sk_bytes(sum(new) % o.R), msg)
        s = native.SetSpec(msg, sig, committees=[3, 4, 5], bits=bits, n_bits=10)
        assert c.verify_jobs([([s], False)]) == [1]
        c.committee_drop(4)
        assert c.verify_jobs([([s], False)]) == [-native.BGV_E_BAD_INDEX]
        c.committee_put(4, [5, 6, 7])
        assert c.verify_jobs([([s], False)]) == [1]
        with pytest.raises(native.BlsGpuError):
            c.pubkeys_put(6, bytes(48))  # undecodable: index 6 is marked, committee 4 holds it
        none = native.SetSpec(msg, sig, committees=[3, 4, 5], bits=bytes(2), n_bits=10)
        assert c.verify_jobs([([s], False), ([none], False)]) == [-native.BGV_E_BAD_INDEX,
                                                                  -native.BGV_E_EMPTY_AGGREGATE]
    finally:
        c.close()
