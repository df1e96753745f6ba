"""GPU tests of the committee-bitfield sets (include/blsgpu.h bgv_committee_put,
bgv_verify_bits, bgv_aggregate_committee_bits): a set names (committee, participation bitfield)
and the device sums the shorter side (k_pk_agg_bits, bgv_pk_bits.h).  Expected aggregates are
the oracle's (tests/golden/committee_bits.json); verdicts are checked against signatures made
with the sum of the participants' secret keys and against the same sets given as index lists.
"""
import hashlib

import pytest

from tests import committeesim as cs

pytestmark = pytest.mark.gpu

INF96 = bytes([0x40]) + bytes(95)


def _o():
    from oracle import bls12381 as o  # secret keys and one expected point; never the code under test
    return o


def _sks():
    o = _o()
    sks = [o.interop_secret_key(i) for i in range(520)]
    return sks + [(o.R - sks[0]) % o.R]


def _sk_bytes(v):
    return int(v).to_bytes(32, "big")


class World:
    """One context with the fixture's 521 keys and every fixture committee uploaded."""

    def __init__(self, devices=None):
        from lodestar_amd import native
        self.native = native
        self.fx = cs.fixture()
        self.sks = _sks()
        self.R = _o().R
        self.ctx = native.Context(devices)
        self.ctx.pubkeys_put(0, b"".join(bytes.fromhex(k) for k in self.fx["keys"]))
        self.ids = {}
        for i, (name, members) in enumerate(sorted(self.fx["committees"].items())):
            self.ids[name] = 100 + i
            self.ctx.committee_put(100 + i, members)
        self.next_id = 1000

    def put(self, members):
        self.next_id += 1
        self.ctx.committee_put(self.next_id, members)
        return self.next_id

    def sum_sk(self, members, positions):
        return sum(self.sks[members[p]] for p in positions) % self.R

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def positions_of(bits, n):
    return [p for p in range(n) if (bits[p >> 3] >> (p & 7)) & 1]


def com_set(w, msg, sig, cid, positions, n):
    return w.native.SetSpec(msg, sig, committee=cid, bits=cs.pack(positions, n), n_bits=n)


def test_aggregates_match_oracle(world):
    """Every fixture case: sizes across the bitfield's word boundaries, the 16-lane team and the
    whole wave, more terms than BGV_PK_TEAM_MAX; patterns on either side of the mode switch;
    cancelling members, infinity totals and infinity results."""
    bad = []
    for c in world.fx["cases"]:
        got = world.ctx.aggregate_committee_bits(world.ids[c["committee"]], bytes.fromhex(c["bits"]), c["n"])
        if got.hex() != c["agg"]:
            bad.append(c["name"])
    assert not bad, bad
    assert world.ctx.aggregate_committee_bits(world.ids["cancel"], cs.pack([1, 4], 20), 20) == INF96


def _verdict_jobs(w):
    """Per finite fixture case a valid job and (n > 1) one with one participant's bit flipped; the
    committee form and the same sets as index lists.  Returns (committee jobs, index jobs, want)."""
    native = w.native
    cases = [c for c in w.fx["cases"] if c["agg"] != INF96.hex()]
    msgs = [hashlib.sha256(b"committee-bits " + c["name"].encode()).digest() for c in cases]
    sk = [w.sum_sk(w.fx["committees"][c["committee"]], positions_of(bytes.fromhex(c["bits"]), c["n"])) for c in cases]
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))
    cj, ij, want = [], [], []
    for i, c in enumerate(cases):
        members, n = w.fx["committees"][c["committee"]], c["n"]
        sig = sigs[96 * i:96 * i + 96]
        pos = positions_of(bytes.fromhex(c["bits"]), n)
        variants = [(pos, 1)]
        if n > 1:  # flip one bit: drop a participant, or add one where only one takes part
            flipped = pos[1:] if len(pos) > 1 else sorted(pos + [(pos[0] + 1) % n])
            variants.append((flipped, 0))
        for p, code in variants:
            cj.append(([com_set(w, msgs[i], sig, w.ids[c["committee"]], p, n)], False))
            ij.append(([native.SetSpec(msgs[i], sig, pk_indices=[members[q] for q in p])], False))
            want.append(code)
    return cj, ij, want


@pytest.mark.parametrize("mode", [0, 1], ids=["worker", "per_job"])
def test_verdicts(world, mode):
    cj, ij, want = _verdict_jobs(world)
    got = world.ctx.verify_jobs(cj, mode)
    assert got == want
    assert world.ctx.verify_jobs(ij, mode) == got  # the expanded index lists decide the same


def test_infinity_aggregates(world):
    """A one-set job whose aggregate is infinity is false, a two-set job BLST_PK_IS_INFINITY
    (direct mode: pk_0 + (-pk_0); complement mode over an infinity total)."""
    w, native = world, world.native
    msg = hashlib.sha256(b"inf").digest()
    sig = w.ctx.sign(_sk_bytes(w.sks[3]), msg)
    good = native.SetSpec(msg, sig, pk_indices=[3])
    for name, pos, n in (("cancel", [1, 4], 20), ("inf_total2", [0, 1], 2), ("inf_total4", [0, 1, 2, 3], 4)):
        inf = com_set(w, msg, sig, w.ids[name], pos, n)
        same = native.SetSpec(msg, sig, pk_indices=[w.fx["committees"][name][p] for p in pos])
        for mode in (native.MODE_WORKER, native.MODE_PER_JOB):
            got = w.ctx.verify_jobs([([inf], False), ([good, inf], False), ([good], False)], mode)
            assert got == [0, -native.BLST_PK_IS_INFINITY, 1], (name, mode)
            assert w.ctx.verify_jobs([([same], False), ([good, same], False), ([good], False)], mode) == got


def test_mixed_call_with_retry(world):
    """130 one-set batchable jobs over three device groups mixing committee sets, index sets and
    pk_bytes sets; one corrupted signature, which the retry rounds pin to its job."""
    w, native = world, world.native
    keys96 = w.ctx.pubkeys_validate([bytes.fromhex(k) for k in w.fx["keys"][:130]])[1]
    members = w.fx["committees"]["n128"]
    msgs = [hashlib.sha256(b"mixed %d" % j).digest() for j in range(130)]
    plan, sk = [], []
    for j in range(130):
        if j % 3 == 0:  # a committee set: participation from one member to all of them
            pos = list(range(0, 128, 1 + j % 7))[:1 + (j * 5) % 128] if j % 2 else list(range(128 - j % 9))
            plan.append(("com", pos))
            sk.append(w.sum_sk(members, pos))
        else:
            plan.append(("idx" if j % 3 == 1 else "bytes", j))
            sk.append(w.sks[j])
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))
    jobs = []
    for j, (kind, v) in enumerate(plan):
        sig = sigs[96 * j:96 * j + 96]
        if j == 77:
            sig = sigs[96 * 76:96 * 77]  # another set's (valid) signature
        if kind == "com":
            s = com_set(w, msgs[j], sig, w.ids["n128"], v, 128)
        elif kind == "idx":
            s = native.SetSpec(msgs[j], sig, pk_indices=[v])
        else:
            s = native.SetSpec(msgs[j], sig, pk_bytes=[keys96[v]])
        jobs.append(([s], True))
    st = native.BgvStats()
    got = w.ctx.verify_jobs(jobs, native.MODE_WORKER, st)
    assert got == [0 if j == 77 else 1 for j in range(130)]
    assert st.batch_retries >= 1


def _block_import(w, participation, flip=False):
    """The block-import shape: 128 attestation aggregates over 128-member committees, the
    512-member sync aggregate and two single-key sets, one non-batchable job of 131 sets."""
    native = w.native
    if not hasattr(w, "att_ids"):
        w.att = [[(5 * j + 3 * i) % 520 for i in range(128)] for j in range(128)]
        w.att_ids = [w.put(m) for m in w.att]
    sync = w.fx["committees"]["n512"]
    msgs = [hashlib.sha256(b"block %d" % j).digest() for j in range(131)]

    def absent(j, n):
        return [(j * 7 + 13 * q) % n for q in range(n * (100 - participation) // 100)]

    pos, sk = [], []
    for j in range(128):
        a = set(absent(j, 128))
        pos.append([p for p in range(128) if p not in a])
        sk.append(w.sum_sk(w.att[j], pos[-1]))
    a = set(absent(1, 512))
    pos.append([p for p in range(512) if p not in a])
    sk.append(w.sum_sk(sync, pos[-1]))
    sk += [w.sks[11], w.sks[12]]
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))
    sg = lambda j: sigs[96 * j:96 * j + 96]
    if flip:
        pos[40] = pos[40][:-1]
    sets = [com_set(w, msgs[j], sg(j), w.att_ids[j], pos[j], 128) for j in range(128)]
    sets.append(com_set(w, msgs[128], sg(128), w.ids["n512"], pos[128], 512))
    sets += [native.SetSpec(msgs[129], sg(129), pk_indices=[11]), native.SetSpec(msgs[130], sg(130), pk_indices=[12])]
    return [(sets, False)]


@pytest.mark.parametrize("participation", [100, 95, 50])
def test_block_import_latency_path(world, participation):
    """131 sets: the smallest calls' path (k_prep_wide sums the committee sets on its pubkey plane).
    The call is 192 slots (three groups of 64) and 3 groups: within BGV_PREP_WIDE_MAX = 340 slots
    and bgv_latency_max() = 16,384 pairs (bgv_device.h), so bgv_launch_prep takes the wide branch
    and pk_bits_one runs; were those thresholds lowered below this call, the size here has to
    follow.  95 %: 6 absentees per attestation, 25 of the sync committee (teams of 16 lanes);
    50 %: 64 and 256 terms (the whole wave, from BGV_PK_ONE_WAVE_MIN = 49 terms)."""
    assert world.ctx.verify_jobs(_block_import(world, participation), world.native.MODE_WORKER) == [1]
    assert world.ctx.verify_jobs(_block_import(world, participation, flip=True), world.native.MODE_WORKER) == [0]


def test_block_import_split_over_devices():
    """The same call on a context over two device entries with the split threshold at 64 sets:
    the job's runs carry their bitfields to each device, same code."""
    w = World([0, 0])
    try:
        w.ctx.set_split(64)
        assert w.ctx.verify_jobs(_block_import(w, 95), w.native.MODE_WORKER) == [1]
        assert w.ctx.verify_jobs(_block_import(w, 95, flip=True), w.native.MODE_WORKER) == [0]
    finally:
        w.close()


def test_bulk_path_and_uniform_group(world):
    """20,000 one-set batchable jobs over 16-member committees: the bulk kernels (k_pk_agg_bits
    before k_prep), 64 of the sets sharing one signing root (a uniform group).  All valid, then
    one set with a wrong bit: exactly its job fails.
    Sizes against the thresholds: 20,032 slots + 313 groups exceed bgv_latency_max() = 16,384
    pairs, so the batch takes bgv_launch_prep's bulk branch; 20,000 one-set batchable jobs are
    above BGV_UNIFORM_MIN_JOBS = 1024, the shared root recurs after other roots (every other job
    of 5000..5127) and has 64 >= kUniformAlignMin = 32 jobs, so layout_call gives it a group of
    its own, which run_pass1 flags BGV_GROUP_UNIFORM on a bulk batch (bgv_host_layout.h).  The
    stats carry no path field; the retry of job 5010 below is resolved by the weighted test only
    a uniform group gets, and the verdicts hold on any path."""
    w, native = world, world.native
    N = 20000
    coms = [[(11 * c + 3 * i) % 520 for i in range(16)] for c in range(32)]
    ids = [w.put(m) for m in coms]
    shared = hashlib.sha256(b"shared root").digest()
    msgs, pos, sk = [], [], []
    for j in range(N):
        # every other job of 5000..5127 signs the shared root: the layout gathers them into one group
        msgs.append(shared if 5000 <= j < 5128 and j % 2 == 0 else hashlib.sha256(b"bulk %d" % j).digest())
        k = 1 + (j * 7) % 16  # 1..16 participants: both modes, the empty complement included
        p = sorted((j + 5 * q) % 16 for q in range(k))
        pos.append(p)
        sk.append(w.sum_sk(coms[j % 32], p))
    sigs = w.ctx.sign(b"".join(_sk_bytes(s) for s in sk), b"".join(msgs))

    def jobs(wrong=None):
        out = []
        for j in range(N):
            p = pos[j]
            if j == wrong:
                p = p[1:] if len(p) > 1 else sorted(p + [(p[0] + 1) % 16])
            out.append(([com_set(w, msgs[j], sigs[96 * j:96 * j + 96], ids[j % 32], p, 16)], True))
        return out

    assert w.ctx.verify_jobs(jobs(), native.MODE_WORKER) == [1] * N
    for wrong in (5010, 12345):  # inside the uniform group, and elsewhere
        got = w.ctx.verify_jobs(jobs(wrong), native.MODE_WORKER)
        assert [j for j in range(N) if got[j] != 1] == [wrong] and got[wrong] == 0


def test_lifecycle(world):
    w, native = world, world.native
    msg = hashlib.sha256(b"lifecycle").digest()
    a, b = [1, 2, 3, 4, 5], [6, 7, 8]
    cid = w.put(a)
    with pytest.raises(native.BlsGpuError) as e:  # a put on a live id
        w.ctx.committee_put(cid, b)
    assert e.value.code == native.BGV_E_ARG
    with pytest.raises(native.BlsGpuError) as e:  # an index past the cache
        w.ctx.committee_put(cid + 5000, [1, 521])
    assert e.value.code == native.BGV_E_BAD_INDEX
    sig_a = w.ctx.sign(_sk_bytes(w.sum_sk(a, [0, 1, 2, 3])), msg)
    sig_b = w.ctx.sign(_sk_bytes(w.sum_sk(b, [0, 2])), msg)
    set_a = com_set(w, msg, sig_a, cid, [0, 1, 2, 3], 5)
    assert w.ctx.verify_jobs([([set_a], False)]) == [1]
    # the argument errors, per job
    stray = native.SetSpec(msg, sig_a, committee=cid, bits=bytes([0x2F]), n_bits=5)
    got = w.ctx.verify_jobs([([com_set(w, msg, sig_a, cid, [0, 1], 4)], False), ([stray], False),
                             ([com_set(w, msg, sig_a, cid, [], 5)], False), ([set_a], False)])
    assert got == [-native.BGV_E_ARG, -native.BGV_E_ARG, -native.BGV_E_EMPTY_AGGREGATE, 1]
    # drop: the id is unknown at once, and free for other members
    w.ctx.committee_drop(cid)
    assert w.ctx.verify_jobs([([set_a], False)]) == [-native.BGV_E_BAD_INDEX]
    with pytest.raises(native.BlsGpuError):
        w.ctx.committee_drop(cid)
    w.ctx.committee_put(cid, b)
    assert w.ctx.verify_jobs([([com_set(w, msg, sig_b, cid, [0, 2], 3)], False)]) == [1]
    assert w.ctx.verify_jobs([([com_set(w, msg, sig_a, cid, [0, 2], 3)], False)]) == [0]


def test_pubkey_overwrite_recomputes_totals():
    """bgv_pubkeys_put over a member of a live committee: sets that subtract from the total see
    the new keys; an undecodable record makes the committee's sets reject."""
    from lodestar_amd import native
    o = _o()
    fx, sks = cs.fixture(), _sks()
    c = native.Context()
    try:
        c.pubkeys_put(0, b"".join(bytes.fromhex(k) for k in fx["keys"][:8]))
        c.committee_put(3, [0, 1, 2, 3, 4])
        c.committee_put(4, [5, 6])
        c.pubkeys_put(2, bytes.fromhex(fx["keys"][300]))  # index 2 now holds key 300
        new = [sks[0], sks[1], sks[300], sks[3], sks[4]]
        want = o.g1_serialize(o.g1_mul(o.G1, sum(new) % o.R))
        assert c.aggregate_committee_bits(3, bytes([0x1F]), 5) == want  # complement over the new total
        msg = hashlib.sha256(b"overwrite").digest()
        sig = c.sign(_sk_bytes((sum(new) - sks[0]) % o.R), msg)
        s = native.SetSpec(msg, sig, committee=3, bits=bytes([0x1E]), n_bits=5)  # all but member 0
        assert c.verify_jobs([([s], False)]) == [1]
        with pytest.raises(native.BlsGpuError):
            c.pubkeys_put(1, bytes(48))  # undecodable: index 1 is marked
        other = native.SetSpec(msg, sig, committee=4, bits=bytes([0x03]), n_bits=2)
        assert c.verify_jobs([([s], False), ([other], False)]) == [-native.BGV_E_BAD_INDEX, 0]
    finally:
        c.close()
