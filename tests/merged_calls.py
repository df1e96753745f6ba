"""Calls of unlike kind, size, keys, roots and failing positions, forced into one device
super-batch (bgv_sched.cpp dispatcher_loop -> run_pass1), and what each caller must get back.
Test infrastructure only; nothing at module level needs a GPU.

force_merge sets both coalescing windows to W_US, so a dispatcher that has taken the first queued
call waits W_US for the others; run_merged submits every call back to back (the asynchronous entry
points from one thread, so the queue order is the submission order; bgv_verify_partial, which has
no asynchronous form, from threads started beforehand that go in at their place in the order) and
reads from the profile counters how many first passes ran.  Expected codes are by construction:
every signature is bgv_sign's under the (summed) secret key, and an invalid part is a set that
names another key, another root, or carries a signature with its compression flag cleared.
"""
import hashlib
import os
import re
import threading
import time

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")
WAVE = 64  # slots per device group; every group starts on a 64-slot boundary
N_KEYS = 700
# The coalescing window of a forced merge: at least 20 times the submission span of the largest
# case (measured 0.56 ms on an MI355X host, docstring of tests/test_gpu_merged_calls.py, which
# asserts every span against W_US / 4), within 200 ms .. 1 s.
W_US = 200_000
# bgv_set_batching's defaults (include/blsgpu.h)
DEFAULT_MAX_SLOTS, DEFAULT_COALESCE_US, DEFAULT_IDLE_US = 131072, 500, 50


def define(header, name):
    """The integer a header of lodestar_amd/csrc gives `#define name`."""
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"^#\s*define\s+%s\s+(\d+)\s*$" % re.escape(name), text, re.M).group(1))


def thresholds():
    return {
        "PREP_WIDE_MAX": define("bgv_device.h", "BGV_PREP_WIDE_MAX"),
        "MILLER_WIDE_MAX": define("bgv_device.h", "BGV_MILLER_WIDE_MAX"),
        "PK_TREE_MIN": define("bgv_device.h", "BGV_PK_TREE_MIN"),
        "PK_TEAM_MAX": define("bgv_pk_bits.h", "BGV_PK_TEAM_MAX"),
        "LATENCY_MAX": 16384,  # bgv_latency_max() without BGV_LATENCY_MAX in the environment
    }


def rotations(items, step=2):
    """The submission orders of a case: as listed, and rotated by `step`."""
    items = list(items)
    k = step % len(items) if items else 0
    return [items, items[k:] + items[:k]]


def all_rotations(items):
    """Every rotation of items: each item is first exactly once."""
    items = list(items)
    return [items[k:] + items[:k] for k in range(len(items))]


class MergedCall:
    """One caller's call.  kind "jobs": verify_jobs(jobs, mode); "aggregate":
    verify_aggregate(jobs, tags, naggs); "partial": verify_partial(sets).  want: the comparable
    result (vector()) by construction, one entry per label.  retry: True when stats.batch_retries
    must be >= 1, False when it must be 0, None when the call reports no stats."""

    def __init__(self, name, kind, want, labels=None, jobs=None, mode=0, sets=None, tags=None, naggs=0, retry=None,
                 groups=1, accepted=None):
        self.name, self.kind, self.want = name, kind, list(want)
        self.labels = list(labels) if labels is not None else [str(j) for j in range(len(self.want))]
        assert len(self.labels) == len(self.want)
        self.jobs, self.mode, self.sets, self.tags, self.naggs = jobs, mode, sets, tags, naggs
        self.retry, self.groups = retry, groups
        self.accepted = accepted  # aggregate: per aggregate, the signatures by construction accepted
        self.packed = None

    @property
    def slots(self):
        return WAVE * self.groups

    @property
    def clean(self):
        """Entirely valid by construction."""
        return self.want == [0, 0, 1] if self.kind == "partial" else all(w == 1 for w in self.want)

    def pack(self, native):
        """The call's C arrays, built once (not inside the submission span)."""
        if self.packed is None:
            self.packed = native.PackedCall(self.jobs if self.kind != "partial" else [(list(self.sets), False)])
        return self.packed


def vector(ctx, call, raw):
    """A call's raw result as the list of integers that want holds: the job codes; for a partial
    call its two codes and bgv_final_verify's verdict over its 576 bytes."""
    if call.kind == "jobs":
        return list(raw[0])
    if call.kind == "aggregate":
        return list(raw[0])
    return [raw[1], raw[2], 1 if ctx.final_verify([raw[0]]) else 0]


def mismatches(cases, got):
    """The names call:label whose result differs from the call's want.  got: {call name: vector}
    (a missing or short vector names every label it lacks)."""
    bad = []
    for call in cases:
        g = got.get(call.name)
        for j, (label, w) in enumerate(zip(call.labels, call.want)):
            if g is None or j >= len(g) or g[j] != w:
                bad.append("%s:%s" % (call.name, label))
        if g is not None and len(g) > len(call.want):
            bad.append("%s:+%d" % (call.name, len(g) - len(call.want)))
    return bad


def force_merge(ctx, window_us=W_US, max_slots=0):
    """Both windows: an idle dispatcher takes the smaller of the two."""
    ctx.set_batching(max_slots, window_us, window_us)


def default_batching(ctx):
    ctx.set_batching(DEFAULT_MAX_SLOTS, DEFAULT_COALESCE_US, DEFAULT_IDLE_US)


class _PartialThread(threading.Thread):
    """bgv_verify_partial from a thread of its own: started before the submission span, it goes
    in when `go` is set and says so through `entering` just before the library call."""

    def __init__(self, ctx, call, native):
        super().__init__(daemon=True)
        self.ctx, self.packed = ctx, call.pack(native)
        self.go, self.entering = threading.Event(), threading.Event()
        self.t_enter, self.raw, self.error = None, None, None

    def run(self):
        self.go.wait()
        try:
            self.t_enter = time.perf_counter()
            self.entering.set()
            self.raw = _partial(self.ctx, self.packed)
        except Exception as e:  # reported by run_merged
            self.error = e
            self.entering.set()


def _partial(ctx, packed):
    import ctypes

    from lodestar_amd.native import _check
    out = ctypes.create_string_buffer(576)
    codes = (ctypes.c_int32 * 2)()
    _check(ctx.lib.bgv_verify_partial(ctx.handle, packed.sets, packed.nsets, out, codes))
    return out.raw, codes[0], codes[1]


def run_merged(ctx, calls, timeout=60.0):
    """Submits every call back to back and waits for all of them.  Returns ({name: raw result},
    first-pass launches, submission span in seconds, {name: stats dict}).  The span runs from before
    the first submit to after the last; a partial call's thread counts from the moment it enters
    the library."""
    from lodestar_amd import native
    for call in calls:
        call.pack(native)
    threads = {}
    for call in calls:
        if call.kind == "partial":
            threads[call.name] = _PartialThread(ctx, call, native)
            threads[call.name].start()
    ctx.profile(1)
    pending = {}
    t0 = time.perf_counter()
    for call in calls:
        if call.kind == "partial":
            th = threads[call.name]
            th.go.set()
            th.entering.wait(timeout)
        elif call.kind == "aggregate":
            pending[call.name] = ctx.verify_aggregate_async(call.packed, call.tags, call.naggs, call.mode)
        else:
            pending[call.name] = ctx.verify_jobs_async(call.packed, call.mode)
    t1 = time.perf_counter()
    raw, stats = {}, {}
    for call in calls:
        if call.kind == "partial":
            th = threads[call.name]
            th.join(timeout)
            if th.is_alive():
                raise TimeoutError("bgv_verify_partial has not returned: " + call.name)
            if th.error is not None:
                raise th.error
            t1 = max(t1, th.t_enter)
            raw[call.name] = th.raw
        elif call.kind == "aggregate":
            raw[call.name] = pending[call.name].wait(timeout)
            stats[call.name] = pending[call.name].stats.as_dict()
        else:
            raw[call.name] = (pending[call.name].wait(timeout),)
            stats[call.name] = pending[call.name].stats.as_dict()
    launches = ctx.profile(0)[1]
    return raw, launches, t1 - t0, stats


def run_alone(ctx, call):
    """The same call through the synchronous entry point, on its own: (raw result, stats dict)."""
    from lodestar_amd import native
    packed = call.pack(native)
    if call.kind == "partial":
        return _partial(ctx, packed), None
    st = native.BgvStats()
    if call.kind == "aggregate":
        return ctx.verify_aggregate(packed, call.tags, call.naggs, call.mode, st), st.as_dict()
    return (ctx.verify_jobs(packed, call.mode, st),), st.as_dict()


def _sk(i):
    return int.from_bytes(hashlib.sha256(b"merged-calls sk %d" % i).digest(), "little") % R


def _root(tag, i=0):
    return hashlib.sha256(b"merged-calls root %s %d" % (tag.encode(), i)).digest()


def clear_flag(sig):
    """The signature with its compression flag cleared: BLST_BAD_ENCODING (-1) for its job."""
    return bytes([sig[0] & 0x7F]) + sig[1:]


def pack_bits(positions, n):
    b = bytearray((n + 7) // 8)
    for p in positions:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


class Scenario:
    """One context with N_KEYS keys (keygen over hash-derived secret keys, key i at cache index
    i) and the builders of the calls; every builder takes its own keys and roots."""

    # committees of the bits and spans calls: (id, first key, members)
    COM_WAVE, COM_TEAM, COM_A, COM_B = (7001, 60, 600), (7002, 660, 40), (7003, 300, 9), (7004, 320, 12)

    def __init__(self, ctx=None):
        from lodestar_amd import native
        self.native = native
        self.th = thresholds()
        self.own_ctx = ctx is None
        self.ctx = ctx if ctx is not None else native.Context([0])
        self.sks = [_sk(i) for i in range(N_KEYS)]
        self.keys48 = self.ctx.keygen(b"".join(s.to_bytes(32, "big") for s in self.sks), cache_first=0)
        self.keys48 = [self.keys48[48 * i:48 * i + 48] for i in range(N_KEYS)]
        for cid, first, n in (self.COM_WAVE, self.COM_TEAM, self.COM_A, self.COM_B):
            self.ctx.committee_put(cid, list(range(first, first + n)))

    def close(self):
        if self.own_ctx:
            self.ctx.close()

    def sign(self, signers, msgs):
        """signers: per signature the list of key indices whose secret keys are summed."""
        sk = [sum(self.sks[k] for k in ks) % R for ks in signers]
        raw = self.ctx.sign(b"".join(s.to_bytes(32, "big") for s in sk), b"".join(msgs))
        return [raw[96 * i:96 * i + 96] for i in range(len(sk))]

    def _one_set_jobs(self, sets):
        return [([s], True) for s in sets]

    # --- the calls --------------------------------------------------------------------------
    def singles(self, name="singles", n=3, first_key=0, wrong=(1,), tag=None):
        """n batchable one-set jobs, one cached key each, distinct roots; the jobs of `wrong` name
        the next key."""
        S = self.native.SetSpec
        tag = tag or name
        keys = [(first_key + j) % N_KEYS for j in range(n)]
        msgs = [_root(tag, j) for j in range(n)]
        sigs = self.sign([[k] for k in keys], msgs)
        sets = [S(msgs[j], sigs[j], pk_indices=[(keys[j] + 1) % N_KEYS if j in wrong else keys[j]]) for j in range(n)]
        return MergedCall(name, "jobs", [0 if j in wrong else 1 for j in range(n)], jobs=self._one_set_jobs(sets),
                          retry=bool(wrong), groups=(n + WAVE - 1) // WAVE)

    def multikey(self):
        """Sets of 2, 3, 15, 16, 17 and 128 cached keys (16 = BGV_PK_TREE_MIN: from there on the
        sums come from k_pk_agg16 through pk_off + ib); the 16-key set names one wrong key."""
        S = self.native.SetSpec
        t = self.th["PK_TREE_MIN"]
        sizes = [2, 3, t - 1, t, t + 1, 128]
        first, lists = 10, []
        for n in sizes:
            lists.append(list(range(first, first + n)))
            first += n
        msgs = [_root("multikey", j) for j in range(len(sizes))]
        sigs = self.sign(lists, msgs)
        named = [list(x) for x in lists]
        named[3][5] = lists[4][0]  # the 16-key set: a key of the next set in place of its sixth
        sets = [S(msgs[j], sigs[j], pk_indices=named[j]) for j in range(len(sizes))]
        return MergedCall("multikey", "jobs", [1, 1, 1, 0, 1, 1], labels=["%dkeys" % n for n in sizes],
                          jobs=self._one_set_jobs(sets), retry=True)

    def records(self):
        """pk_bytes sets of 1 and 3 records (pubkeys_validate's 96-byte output): the pb base.
        Entirely valid: the clean call of its cases."""
        S = self.native.SetSpec
        codes, k96 = self.ctx.pubkeys_validate(self.keys48[200:204])
        assert codes == [0, 0, 0, 0]
        lists = [[200], [201, 202, 203]]
        msgs = [_root("records", j) for j in range(2)]
        sigs = self.sign(lists, msgs)
        sets = [S(msgs[j], sigs[j], pk_bytes=[k96[k - 200] for k in lists[j]]) for j in range(2)]
        return MergedCall("records", "jobs", [1, 1], labels=["1rec", "3rec"], jobs=self._one_set_jobs(sets),
                          retry=False)

    def com_side(self, n, k):
        """(complement side, terms) as bgv_pk_bits.h pkb_use_complement / pkb_terms choose."""
        comp = n - k + 1 < k
        return comp, (n - k if comp else k)

    def bits(self):
        """bgv_verify_bits sets: a 600-member committee with 300 bits set (direct side, 300 terms
        above BGV_PK_TEAM_MAX: the wave list) and a 40-member one with 35 set (complement side, 5
        terms: the team list); the second set is signed over another root."""
        S = self.native.SetSpec
        (wid, wfirst, wn), (tid, tfirst, tn) = self.COM_WAVE, self.COM_TEAM
        wpos = list(range(0, wn, 2))
        tpos = [p for p in range(tn) if p % 8 != 3]
        assert self.com_side(wn, len(wpos)) == (False, 300) and 300 > self.th["PK_TEAM_MAX"]
        assert self.com_side(tn, len(tpos)) == (True, 5) and 5 <= self.th["PK_TEAM_MAX"]
        msgs = [_root("bits", 0), _root("bits", 1)]
        sigs = self.sign([[wfirst + p for p in wpos], [tfirst + p for p in tpos]], [msgs[0], _root("bits", 2)])
        sets = [S(msgs[0], sigs[0], committee=wid, bits=pack_bits(wpos, wn), n_bits=wn),
                S(msgs[1], sigs[1], committee=tid, bits=pack_bits(tpos, tn), n_bits=tn)]
        call = MergedCall("bits", "jobs", [1, 0], labels=["wave", "team"], jobs=self._one_set_jobs(sets), retry=True)
        assert call.pack(self.native).pkbits is not None and call.packed.spans is None
        return call

    def spans(self):
        """A set over two committees (9 and 12 members, one bitfield of 21 bits) beside a plain
        set whose signature has its compression flag cleared: the slot is not live, its group
        passes, no retry."""
        S = self.native.SetSpec
        (aid, afirst, an), (bid, bfirst, bn) = self.COM_A, self.COM_B
        pos = [0, 2, 3, 8, 9, 10, 15, 20]
        members = list(range(afirst, afirst + an)) + list(range(bfirst, bfirst + bn))
        msgs = [_root("spans", 0), _root("spans", 1)]
        sigs = self.sign([[340], [members[p] for p in pos]], msgs)
        sets = [S(msgs[0], clear_flag(sigs[0]), pk_indices=[340]),
                S(msgs[1], sigs[1], committees=[aid, bid], bits=pack_bits(pos, an + bn), n_bits=an + bn)]
        call = MergedCall("spans", "jobs", [-self.native.BLST_BAD_ENCODING, 1], labels=["plain", "span"],
                          jobs=self._one_set_jobs(sets), retry=False)
        assert call.pack(self.native).spans is not None
        return call

    def perjob(self):
        """A MODE_PER_JOB call of three jobs (a group each) among the worker-mode calls; the third
        names another root."""
        S = self.native.SetSpec
        keys = [350, 351, 352]
        msgs = [_root("perjob", j) for j in range(3)]
        sigs = self.sign([[k] for k in keys], msgs)
        sets = [S(msgs[0], sigs[0], pk_indices=[350]), S(msgs[1], sigs[1], pk_indices=[351]),
                S(_root("perjob", 9), sigs[2], pk_indices=[352])]
        return MergedCall("perjob", "jobs", [1, 1, 0], jobs=self._one_set_jobs(sets), mode=self.native.MODE_PER_JOB,
                          groups=3)

    def widejob(self):
        """One batchable job of 70 sets (two groups), one non-batchable job of 3 sets (a group of
        its own, laid out first) and one more batchable one-set job, which makes the 70-set job's
        second group a shared one: with set 66 over another root that group fails and its two jobs
        go to a fanout retry, the 70-set job as two runs of slots."""
        S = self.native.SetSpec
        n = 70
        keys = [360 + j for j in range(n + 4)]
        msgs = [_root("widejob", j) for j in range(n + 4)]
        sigs = self.sign([[k] for k in keys], msgs)
        sets = [S(_root("widejob", 999) if j == 66 else msgs[j], sigs[j], pk_indices=[keys[j]]) for j in range(n + 4)]
        jobs = [(sets[:n], True), (sets[n:n + 3], False), (sets[n + 3:], True)]
        return MergedCall("widejob", "jobs", [0, 1, 1], labels=["70sets", "3sets", "tail"], jobs=jobs, retry=True,
                          groups=3)

    def hostmix(self):
        """Device jobs beside an empty job and a job naming an index past the cache (todo is
        shorter than the job list); the third device job names a wrong key."""
        S = self.native.SetSpec
        nat = self.native
        keys = [440, 441, 442]
        msgs = [_root("hostmix", j) for j in range(3)]
        sigs = self.sign([[k] for k in keys], msgs)
        good = [S(msgs[j], sigs[j], pk_indices=[keys[j]]) for j in range(3)]
        good[2] = S(msgs[2], sigs[2], pk_indices=[443])
        past = S(msgs[0], sigs[0], pk_indices=[N_KEYS + 5])
        jobs = [([good[0]], True), ([], True), ([good[1]], True), ([past], True), ([good[2]], True)]
        return MergedCall("hostmix", "jobs", [1, -nat.BGV_E_EMPTY_SET, 1, -nat.BGV_E_BAD_INDEX, 0],
                          labels=["dev0", "empty", "dev1", "past", "dev2"], jobs=jobs, retry=True)

    def aggregate(self):
        """verify_aggregate_async: 12 tagged one-set jobs over two aggregates (even jobs 0, odd
        jobs 1); job 4 names a wrong key, so aggregate 0 sums five signatures and aggregate 1 six."""
        S = self.native.SetSpec
        keys = [450 + j for j in range(12)]
        msgs = [_root("aggregate", j % 3) for j in range(12)]
        sigs = self.sign([[k] for k in keys], msgs)
        sets = [S(msgs[j], sigs[j], pk_indices=[keys[j] + 20 if j == 4 else keys[j]]) for j in range(12)]
        want = [0 if j == 4 else 1 for j in range(12)]
        tags = [j % 2 for j in range(12)]
        accepted = [[sigs[j] for j in range(12) if tags[j] == a and want[j] == 1] for a in range(2)]
        return MergedCall("aggregate", "aggregate", want, jobs=self._one_set_jobs(sets), tags=tags, naggs=2,
                          retry=True, accepted=accepted)

    def partial(self, name="partial", wrong_message=False):
        """verify_partial over 5 sets (2, 1, 3, 1 and 17 keys); wrong_message: the same shard with
        its third set over another root.  want: the two codes and the verdict of its product."""
        S = self.native.SetSpec
        lists = [[480, 481], [482], [483, 484, 485], [486], list(range(487, 504))]
        msgs = [_root("partial", j) for j in range(5)]
        sigs = self.sign(lists, msgs)
        sets = [S(_root("partial", 77) if wrong_message and j == 2 else msgs[j], sigs[j], pk_indices=lists[j])
                for j in range(5)]
        return MergedCall(name, "partial", [0, 0, 0 if wrong_message else 1], labels=["sig_code", "pk_code", "verdict"],
                          sets=sets)

    # --- the cases ---------------------------------------------------------------------------
    def five(self):
        return [self.singles(), self.records(), self.bits(), self.spans(), self.multikey()]

    def team(self):
        return self.five() + [self.widejob(), self.aggregate(), self.perjob(), self.hostmix(), self.partial(),
                              self.partial("partial_bad", wrong_message=True)]

    def ten_singles(self):
        """Ten calls of 64 jobs; call k names a wrong key at job 7k mod 64."""
        return [self.singles("singles64_%d" % k, n=64, first_key=61 * k + 5, wrong=((7 * k) % 64,)) for k in range(10)]

    def cap_calls(self):
        """Five 64-slot calls of 2..6 jobs, the third of them clean."""
        return [self.singles("cap%d" % k, n=2 + k, first_key=100 * k + 7, wrong=() if k == 2 else (k % (2 + k),))
                for k in range(5)]

    def bulk_calls(self):
        """The calls A, B and C of the bulk case (all batchable one-set jobs)."""
        S = self.native.SetSpec

        def call(name, n, key_of, root_of, wrong_key=(), wrong_msg=(), undecodable=()):
            keys = [key_of(j) for j in range(n)]
            assert len(set(keys)) == n and max(keys) + 1 < N_KEYS
            msgs = [root_of(j) for j in range(n)]
            sigs = self.sign([[k] for k in keys], msgs)
            sets, want = [], []
            for j in range(n):
                sig = clear_flag(sigs[j]) if j in undecodable else sigs[j]
                msg = _root(name + " other", j) if j in wrong_msg else msgs[j]
                key = (keys[j] + 1) % N_KEYS if j in wrong_key else keys[j]
                sets.append(S(msg, sig, pk_indices=[key]))
                want.append(-self.native.BLST_BAD_ENCODING if j in undecodable else
                            0 if j in wrong_key or j in wrong_msg else 1)
            return MergedCall(name, "jobs", want, jobs=self._one_set_jobs(sets), retry=True,
                              groups=(n + WAVE - 1) // WAVE)

        a = call("A", 130, lambda j: 3 * j + 11, lambda j: _root("A", j // 64), wrong_key=(5,))
        b = call("B", 70, lambda j: 5 * j + 2, lambda j: _root("B", j), wrong_msg=(67,), undecodable=(9,))
        c = call("C", 100, lambda j: 6 * j + 100, lambda j: _root("C", j // 50), wrong_key=(70, 90))
        return [a, b, c]


def sizes(calls):
    """(slots, groups, pairs) of the calls merged: a call's slot count is 64 x its group count."""
    groups = sum(c.groups for c in calls)
    return WAVE * groups, groups, WAVE * groups + groups
