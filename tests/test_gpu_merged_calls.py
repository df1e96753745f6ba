"""Merged super-batches of unlike calls, checked call by call (tests/merged_calls.py).

libblsgpu.so merges whatever calls are queued into one device super-batch (bgv_sched.cpp
dispatcher_loop -> run_pass1) and hands every caller its part: the slots of a later call are
rebased (bgv_host_layout.h rebase_slot: hsrc, group, pk_off by the index base or the record base),
the uniq / com_team / com_wave / span_team / span_wave lists are concatenated kind by kind, statuses
and verdicts come back at slot_base and the call's first group, a partial call multiplies its own
run of group products, the retry rounds of all calls share one list of tests, and the kernels are
chosen by the merged size.  Elsewhere in tests/ calls merge only by accident (the idle window is
50 us), and the benchmarks merge identical calls, where a result read from the neighbour's region
is the same result.  Here both coalescing windows are set to W, calls that differ in kind, size,
keys, roots and failing positions are submitted back to back, and every caller's result must equal
the constructed truth and the same call submitted alone.

  case         merged size                                     what only the merge reaches
  wide         5 one-group calls, 320 slots <= PREP_WIDE_MAX   k_prep_wide, per-slot signature pairs,
                                                               k_final_fold over rebased lists
  team         960 slots, 975 pairs <= MILLER_WIDE_MAX         k_prep_a / k_prep_team, group sums,
                                                               k_miller_wide; every call alone is wide
  miller_team  1,600 slots, 1,625 pairs > MILLER_WIDE_MAX      k_miller_team; ten failing calls' units
                                                               in one retry round
  cap          five 64-slot calls under max_batch_slots 128    slots + n > cap splits the queue (2 + 2 + 1
                                                               launches), slots + n == cap still joins
  bulk         child process, BGV_LATENCY_MAX=0                a uniform batch of uniform and mixed
                                                               groups of different calls, the weighted
                                                               test, pattern tests whose reference is a
                                                               first-pass group at gb > 0,
                                                               bgv_launch_partial at gb > 0

That the merge happened is read from the profile counters: bgv_profile counts one launch per first
pass.  A case whose launch count is not the stated one fails; before that the submission span is
asserted against W / 4, so a miss explains itself.

The window W (merged_calls.W_US) is measured, not guessed.  On an MI355X host the submission span of
the largest case (miller_team: 21 calls, two of them bgv_verify_partial threads) measured 0.56 ms
(0.08 to 0.61 ms over all cases here); 20 times that is 12 ms, so W = 200 ms, the lower end of the
200 ms .. 1 s range, about 350 times the span.  Every case costs about W plus a few milliseconds of
kernels; the file ran in 11 s.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import merged_calls as mc  # noqa: E402

pytestmark = pytest.mark.gpu

TH = mc.thresholds()
_oracle_aggregates = {}


def _o():
    from oracle import bls12381 as o  # expected aggregates and final exponentiations; never the code under test
    return o


def execute(sc, calls, max_slots=0):
    """Runs the calls merged, then each alone under the default windows.  Everything a verdict on
    the case needs, as JSON-able values (the bulk case prints it from a child process)."""
    ctx = sc.ctx
    mc.force_merge(ctx, mc.W_US, max_slots)
    try:
        raw, launches, span, stats = mc.run_merged(ctx, calls)
    finally:
        mc.default_batching(ctx)
    res = {"launches": launches, "span": span, "stats": stats, "got": {}, "alone": {}, "alone_stats": {},
           "aggregates": {}, "partials": {}}
    for call in calls:
        res["got"][call.name] = mc.vector(ctx, call, raw[call.name])
        if call.kind == "aggregate":
            res["aggregates"][call.name] = [[s, n, b.hex()] for s, n, b in raw[call.name][1]]
        if call.kind == "partial":
            res["partials"][call.name] = raw[call.name][0].hex()
    for call in calls:
        a, st = mc.run_alone(ctx, call)
        res["alone"][call.name] = mc.vector(ctx, call, a)
        res["alone_stats"][call.name] = st
    return res


def judge(calls, res, want_launches):
    names = [c.name for c in calls]
    print("merged case %s: span %.3f ms, window %d ms, launches %d" %
          (names, 1e3 * res["span"], mc.W_US // 1000, res["launches"]))
    # no two alike: the property the benchmarks' super-batches lack
    vectors = [tuple(c.want) for c in calls]
    assert len(set(vectors)) == len(vectors), "two calls of the case expect the same vector"
    assert any(c.clean for c in calls), "no entirely valid call in the case"
    assert sum(1 for c in calls[1:] if c.retry) >= 2  # retry rounds run with gb > 0
    assert res["span"] < mc.W_US * 1e-6 / 4, "submission took %.1f ms of a %d ms window" % (
        1e3 * res["span"], mc.W_US // 1000)
    assert res["launches"] == want_launches
    assert mc.mismatches(calls, res["got"]) == []
    assert mc.mismatches(calls, res["alone"]) == []
    assert res["got"] == res["alone"]
    for call in calls:
        if call.retry is None:
            continue
        for where in ("stats", "alone_stats"):
            r = res[where][call.name]["batch_retries"]
            assert (r >= 1) if call.retry else (r == 0), (call.name, where, r)
        assert res["stats"][call.name]["sets_verified"] == res["alone_stats"][call.name]["sets_verified"], call.name
    o = _o()
    for call in calls:
        if call.kind == "aggregate":
            for a, sub in enumerate(call.accepted):
                status, count, got = res["aggregates"][call.name][a]
                key = hashlib.sha256(b"".join(sub)).digest()
                if key not in _oracle_aggregates:
                    _oracle_aggregates[key] = o.signatures_aggregate(list(sub))
                code, want = _oracle_aggregates[key]
                assert code == 0 and count == len(sub) and status == 0, (call.name, a, status, count)
                assert bytes.fromhex(got) == want, (call.name, a)
        if call.kind == "partial":
            from tests.test_pairing_golden import f12_from_bytes
            one = o.final_exp(f12_from_bytes(bytes.fromhex(res["partials"][call.name]))) == o.F12_ONE
            assert one == (call.want[2] == 1), call.name  # the oracle's verdict on the 576 bytes
            assert res["got"][call.name][2] == (1 if one else 0), call.name  # bgv_final_verify agrees


@pytest.fixture(scope="module")
def world():
    sc = mc.Scenario()
    yield sc
    sc.close()


@pytest.mark.parametrize("first", range(5))
def test_wide(world, first):
    """Five one-group calls, every kind first (unrebased) once: rotation 0 is the listed order,
    rotation 2 the one rotated by two."""
    calls = mc.all_rotations(world.five())[first]
    slots, groups, pairs = mc.sizes(calls)
    assert (slots, groups) == (320, 5) and slots <= TH["PREP_WIDE_MAX"] and pairs <= TH["LATENCY_MAX"]
    judge(calls, execute(world, calls), 1)


@pytest.mark.parametrize("order", [0, 1], ids=["listed", "rotated2"])
def test_team(world, order):
    calls = mc.rotations(world.team(), 2)[order]
    slots, groups, pairs = mc.sizes(calls)
    assert all(c.slots <= TH["PREP_WIDE_MAX"] for c in calls)  # every call alone is wide
    assert slots > TH["PREP_WIDE_MAX"] and pairs <= TH["MILLER_WIDE_MAX"]
    judge(calls, execute(world, calls), 1)


def test_miller_team(world):
    calls = world.team() + world.ten_singles()
    slots, groups, pairs = mc.sizes(calls)
    assert TH["MILLER_WIDE_MAX"] < pairs < TH["LATENCY_MAX"] // 8
    assert [c.want.index(0) for c in calls[-10:]] == [(7 * k) % 64 for k in range(10)]
    judge(calls, execute(world, calls), 1)


def test_cap(world):
    """max_batch_slots = 128: the dispatcher takes a queue of five 64-slot calls as 2 + 2 + 1."""
    calls = world.cap_calls()
    assert [c.slots for c in calls] == [64] * 5
    judge(calls, execute(world, calls, max_slots=128), 3)


def test_profiled_small_call_on_a_fresh_context():
    """The launch count above comes from bgv_profile, so profiling must not disturb the calls.  On a
    fresh context the first profiled call takes the smallest calls' route (bgv_sig_pairs: one
    k_miller_wide launch).  That route recorded only the closing event of the k_miller pair, so
    prof_add's hipEventElapsedTime failed on the never-recorded opening event: k_miller read 0 ms,
    and the failure stayed the dispatcher thread's last HIP error, with which the launch check of
    the next call on that thread failed (BGV_E_DEVICE for a valid call).  This file's first case
    showed it."""
    from lodestar_amd import native
    ctx = native.Context([0])
    try:
        sks = [(k + 1).to_bytes(32, "big") for k in range(3)]
        ctx.keygen(b"".join(sks), cache_first=0, want_pubkeys=False)
        msgs = [hashlib.sha256(b"profiled %d" % k).digest() for k in range(3)]
        sigs = ctx.sign(b"".join(sks), b"".join(msgs))
        jobs = [([native.SetSpec(msgs[k], sigs[96 * k:96 * k + 96], pk_indices=[k])], True) for k in range(3)]
        ctx.profile(1)
        assert ctx.verify_jobs(jobs) == [1, 1, 1]
        ms, launches = ctx.profile(0)
        assert launches == 1
        assert sorted(ms) == ["k_final", "k_miller", "k_prep"] and all(v > 0 for v in ms.values()), ms
        for _ in range(8):  # later calls, whichever dispatcher thread takes them
            assert ctx.verify_jobs(jobs) == [1, 1, 1]
    finally:
        ctx.close()


BULK_RUNS = {
    "default": ("ABC", {}),
    "final12": ("ABC", {"BGV_RETRY_FOLD_MAX": "0"}),  # k_final12 multiplies the tests' pubkey-sum pairs
    "reversed": ("CBA", {}),
}


def _bulk_calls(sc, order):
    abc = {c.name: c for c in sc.bulk_calls()}
    # a partial call between the verify calls and one behind them: at most one call is first
    return [abc[order[0]], sc.partial(), abc[order[1]], sc.aggregate(), abc[order[2]],
            sc.partial("partial_bad", wrong_message=True)]


def _child(order):
    assert os.environ.get("BGV_LATENCY_MAX") == "0"
    sc = mc.Scenario()
    try:
        print(json.dumps(execute(sc, _bulk_calls(sc, order))))
    finally:
        sc.close()


@pytest.mark.parametrize("run", sorted(BULK_RUNS))
def test_bulk(world, run):
    """BGV_LATENCY_MAX=0 (read once per process, hence the child): every batch is a bulk batch, so
    the merged one is uniform.  A: 130 jobs, one root per 64, a wrong key at job 5 (a uniform
    group: the weighted test).  B: 70 jobs over distinct roots (mixed groups), job 67 over another
    root, job 9 undecodable.  C: 100 jobs, one root per 50, wrong keys at jobs 70 and 90, both in
    its 36-slot same-root group (two invalid slots defeat the weighted test: pattern tests, whose
    reference is the group's first-pass value at the call's first group + 1)."""
    order, knobs = BULK_RUNS[run]
    env = dict(os.environ, BGV_LATENCY_MAX="0", **knobs)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), order], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    calls = _bulk_calls(world, order)
    abc = {c.name: c for c in calls}
    assert [abc["A"].want.index(0), abc["B"].want.index(0), abc["B"].want.index(-1)] == [5, 67, 9]
    assert [j for j, w in enumerate(abc["C"].want) if w == 0] == [70, 90]
    judge(calls, res, 1)


if __name__ == "__main__":
    _child(sys.argv[1])
