"""GPU: crafted G1 wire bytes (tests/golden/pk_edges.json, tools/gen_golden_pk_edges.py, oracle
only) through every place where the device decodes a pubkey, and what follows the decoding.

  route  kernel                                                      call here
  P1     k_pk_validate (g1_decompress + [r]P), bgv_k_util.hip        pubkeys_validate, with and without
                                                                     out96; first half of deposits_verify
  P2     k_cache_put_compressed                                      bgv_pubkeys_put(fmt 48)
  P3     k_cache_put_uncompressed (g1_deserialize)                   bgv_pubkeys_put(fmt 96)
  P4     pk_sum's record branch (bgv_k_tasks.h) in k_prep_wide       verify_jobs, 64 one-set jobs a call
  P5     the same branch in k_prep_a                                 verify_jobs, N_TEAM one-set jobs
  P6     the same branch in the bulk k_prep                          the N_TEAM call in a child process
                                                                     with BGV_LATENCY_MAX=0

The corpus: every flag combination, the infinity encodings with stray bits, x and y at and around
p, non-canonical x + p and y + p below 2^381, x = 0, off-curve points, compressed bytes inside a
record, sort flips, limb patterns, and the subgroup edges: pure torsion points of order 11, 10177,
859267, 52437899 and 11 * 10177, and valid keys with such a point added.  Cache entries and records
are taken on trust (no subgroup check), so a mixed-order key goes through the GLV multiplication,
the point programs of k_prep_wide and the Miller loop, and must verify the signature of its
underlying secret key, the torsion part dying in the final exponentiation; as a deposit key it is
rejected.  Multi-record sets carry a bad record first, in the middle and last, two bad records of
different codes, infinity records, pk and -pk, a record twice and three times (the doubling branch
of jac_add_aff), 17 and 65 records, mixed-order records and torsion parts that cancel.

Edge entries sit at slots 0, 63, 64 and the last of every decoding kernel's run, valid keys and
valid golden sets between them (tests/sig_edges.py place).  N_TEAM and the routing threshold come
from bgv_device.h as in tests/test_gpu_randomizer_edges.py.  Every expected value is the
fixture's; no pairing is computed here.  Integer work, bit-exact, no tolerance.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)  # the child process runs this file as a script

from tests import pk_edges as pe  # noqa: E402
from tests import sig_edges as se  # noqa: E402

WAVE = 64
BAD_INDEX = 22
ABSENTEE = 115  # a valid key beside the fixture's agg_keys: the one clear bit of the committee sets


def _serialize(pt):
    return pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def _items():
    """Everything the record routes verify: (name, records, root, sig, expected one-set code) for
    each entry with a 96-byte form, then for each multi-record set."""
    from oracle import bls12381 as o  # the encodings of the sets' record references only
    items = [(e["name"], [e["pk96"]], e["root"], e["sig"], pe.job_code(e)) for e in pe.with_form(pe.corpus(), 96)]
    sets, partner = pe.record_sets(o)
    items += [("set_" + s["name"], s["records"], s["root"], s["sig"], s["expect"]) for s in sets]
    return items, sets, partner


def _record_jobs(n, items, must):
    """n one-set batchable jobs: the items placed by se.place, valid golden sets (their key as a
    96-byte record) elsewhere.  Returns (jobs, [{"name", "want"}])."""
    from lodestar_amd import native
    _, pk96 = pe.keys()
    valid = se.golden_valid()
    slots = se.place(n, items, must)
    assert all(s in slots for s in must if s < n)
    assert all(any(i not in slots for i in range(g, min(g + WAVE, n))) for g in range(0, n, WAVE) if n - g > 1)
    jobs, want = [], []
    for i in range(n):
        if i in slots:
            name, records, root, sig, code = slots[i]
        else:
            key, root, sig = valid[i % len(valid)]
            name, records, code = "valid", [pk96[key]], 1
        jobs.append(([native.SetSpec(root, sig, pk_bytes=records)], True))
        want.append({"name": "%s@%d" % (name, i), "want": code})
    return jobs, want


def _run(ctx, jobs, mode):
    from lodestar_amd import native
    st = native.BgvStats()
    return ctx.verify_jobs(jobs, mode, st), st.batch_retries


def _team_call(n_team):
    items, _, _ = _items()
    return _record_jobs(n_team, items, (0, WAVE - 1, WAVE, n_team - 1))


def _child():
    from lodestar_amd import native
    from tests.test_gpu_randomizer_edges import N_TEAM
    jobs, _ = _team_call(N_TEAM)
    ctx = native.Context([0])
    got, retries = _run(ctx, jobs, native.MODE_WORKER)
    ctx.close()
    print(json.dumps({"worker": got, "retries": retries}))


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    from lodestar_amd import native
    from tests.test_gpu_randomizer_edges import N_TEAM, PREP_WIDE_MAX, _padded
    assert _padded(WAVE) <= PREP_WIDE_MAX < _padded(N_TEAM)  # 64 jobs: k_prep_wide; N_TEAM: k_prep_a
    items, sets, partner = _items()
    keys, pk96 = pe.keys()
    ctx = native.Context([0])
    yield {"ctx": ctx, "n_team": N_TEAM, "corpus": pe.corpus(), "items": items, "sets": sets, "partner": partner,
           "keys": keys, "pk48": [bytes.fromhex(k) for k in keys["pk_compressed"]], "pk96": pk96}
    ctx.close()


def _validate_run(world):
    """The compressed corpus between valid keys: (keys, [{"name", "code", "rec"}])."""
    edges = pe.with_form(world["corpus"], 48)
    n = 2 * WAVE
    slots = se.place(n, edges, (0, WAVE - 1, WAVE, n - 1))
    keys, want = [], []
    for i in range(n):
        if i in slots:
            e = slots[i]
            keys.append(e["pk48"])
            want.append({"name": "%s@%d" % (e["name"], i), "code": -e["validate"],
                         "rec": _serialize(pe.point(e)) if e["validate"] == 0 else pe.INF96})
        else:
            keys.append(world["pk48"][i])
            want.append({"name": "valid@%d" % i, "code": 0, "rec": world["pk96"][i]})
    assert len(slots) == len(edges)
    return keys, want


def test_p1_pubkeys_validate(world):
    """Codes of every compressed entry, and the 96-byte records: the key uncompressed where it is
    valid, the infinity record (0x40, zeros) where it is not."""
    keys, want = _validate_run(world)
    codes, recs = world["ctx"].pubkeys_validate(keys)
    assert se.mismatches(want, codes, lambda w: w["code"]) == []
    assert se.mismatches(want, recs, lambda w: w["rec"]) == []
    assert sum(1 for w in want if w["code"] == -3) >= 15  # x = 0, the limb, torsion and mixed-order points


def test_p1_pubkeys_validate_without_records(world):
    keys, want = _validate_run(world)
    ctx = world["ctx"]
    st = (ctypes.c_int32 * len(keys))(*([77] * len(keys)))
    buf = ctypes.create_string_buffer(b"".join(keys), 48 * len(keys))
    assert ctx.lib.bgv_pubkeys_validate(ctx.handle, buf, len(keys), st, None) == 0
    assert se.mismatches(want, list(st), lambda w: w["code"]) == []


@pytest.mark.parametrize("form", [48, 96], ids=["p2-compressed", "p3-uncompressed"])
def test_pubkeys_put(world, form):
    """One put of the whole corpus between valid keys into a fresh context: the return code, the
    count, every committed entry read back, the marks and their clearing, and every decodable key
    as the key of a set (a mixed-order one also in a 16-key set and in a committee set)."""
    from lodestar_amd import native
    fx = pe.fixture()
    edges = pe.with_form(world["corpus"], form)
    n = 3 * WAVE
    slots = se.place(n, edges, (0, WAVE - 1, WAVE, n - 1))
    order = fx["agg_keys"] + [ABSENTEE] + [k for k in range(128) if k not in fx["agg_keys"] and k != ABSENTEE]
    valid_form = world["pk48"] if form == 48 else world["pk96"]
    raw, where, fill = [], {}, 0
    for i in range(n):
        if i in slots:
            raw.append(slots[i]["pk%d" % form])
        else:
            k = order[fill % len(order)]
            fill += 1
            where.setdefault(k, i)
            raw.append(valid_form[k])
    assert all(k in where for k in fx["agg_keys"] + [ABSENTEE])
    ctx = native.Context([0])
    try:
        buf = ctypes.create_string_buffer(b"".join(raw), form * n)
        rc = ctx.lib.bgv_pubkeys_put(ctx.handle, 0, buf, n, form)
        bad = [i for i in sorted(slots) if pe.put_status(slots[i], form)]
        good = [i for i in sorted(slots) if not pe.put_status(slots[i], form)]
        assert len(bad) >= 15 and len(good) >= 20 and 0 in slots and n - 1 in slots
        assert rc == -pe.put_status(slots[bad[0]], form)
        assert ctx.pubkeys_count() == n
        # committed entries, off-subgroup ones included
        named = [{"name": "%s@%d" % (slots[i]["name"], i), "rec": _serialize(pe.point(slots[i]))} for i in good]
        assert se.mismatches(named, [ctx.aggregate_pubkeys([i]) for i in good], lambda w: w["rec"]) == []
        assert ctx.aggregate_pubkeys([where[5]]) == world["pk96"][5]
        # the marks
        any_root, any_sig = slots[good[0]]["root"], slots[good[0]]["sig"]
        got = ctx.verify_jobs([([native.SetSpec(any_root, any_sig, pk_indices=[i])], True) for i in bad])
        assert se.mismatches([{"name": "%s@%d" % (slots[i]["name"], i)} for i in bad], got, lambda w: -BAD_INDEX) == []
        with pytest.raises(native.BlsGpuError) as err:
            ctx.aggregate_pubkeys([where[5], bad[-1]])
        assert err.value.code == BAD_INDEX
        # every decodable key alone
        alone = [([native.SetSpec(slots[i]["root"], slots[i]["sig"], pk_indices=[i])], True) for i in good]
        want = [{"name": "%s@%d" % (slots[i]["name"], i), "want": slots[i]["verdict"]} for i in good]
        for mode in (native.MODE_WORKER, native.MODE_PER_JOB):
            assert se.mismatches(want, ctx.verify_jobs(alone, mode), lambda w: w["want"]) == [], mode
        # a mixed-order key in a 16-key set (the k_pk_agg tree) and in a committee set with one
        # absentee (the complement side of k_pk_agg_bits)
        mixed = [i for i in good if "agg_sig" in slots[i]]
        assert len(mixed) >= 6 and all(slots[i]["agg_verdict"] == 1 and slots[i]["verdict"] == 1 for i in mixed)
        others = [where[k] for k in fx["agg_keys"]]
        jobs, names = [], []
        for c, i in enumerate(mixed):
            e = slots[i]
            members = others[:c + 1] + [i] + others[c + 1:]  # the mixed key at another place each time
            jobs.append(([native.SetSpec(e["root"], e["agg_sig"], pk_indices=members)], True))
            com = members[:c] + [where[ABSENTEE]] + members[c:]
            bits = bytearray(b"\xff\xff\x01")
            bits[c >> 3] &= ~(1 << (c & 7))
            ctx.committee_put(c, com)
            jobs.append(([native.SetSpec(e["root"], e["agg_sig"], committee=c, bits=bytes(bits), n_bits=17)], True))
            names += [{"name": e["name"] + " in 16 keys"}, {"name": e["name"] + " in a committee"}]
        for mode in (native.MODE_WORKER, native.MODE_PER_JOB):
            assert se.mismatches(names, ctx.verify_jobs(jobs, mode), lambda w: 1) == [], mode
        # a valid key over a marked index clears the mark
        e8 = next(e for e in world["corpus"] if e["name"] == "valid_key8")
        one = ctypes.create_string_buffer(valid_form[8], form)
        assert ctx.lib.bgv_pubkeys_put(ctx.handle, bad[0], one, 1, form) == 0
        assert ctx.pubkeys_count() == n
        assert ctx.aggregate_pubkeys([bad[0]]) == world["pk96"][8]
        assert ctx.verify_jobs([([native.SetSpec(e8["root"], e8["sig"], pk_indices=[bad[0]])], True),
                                ([native.SetSpec(any_root, any_sig, pk_indices=[bad[1]])], True)]) == [1, -BAD_INDEX]
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["worker", "per_job"])
def test_p4_records_latency_small(world, mode):
    """k_prep_wide: 64 one-set jobs a call, so the items take three calls; an item at slots 0 and
    63 of each."""
    from lodestar_amd import native
    items = world["items"]
    per = WAVE // 2  # the most se.place spreads over 64 slots
    done = retries = 0
    for lo in range(0, len(items), per):
        jobs, want = _record_jobs(WAVE, items[lo:lo + per], (0, WAVE - 1))
        got, r = _run(world["ctx"], jobs, native.MODE_WORKER if mode == "worker" else native.MODE_PER_JOB)
        assert se.mismatches(want, got, lambda w: w["want"]) == []
        done += len(items[lo:lo + per])
        retries += r
    assert done == len(items)
    if mode == "worker":
        assert retries >= 1


@pytest.mark.parametrize("mode", ["worker", "per_job"])
def test_p5_records_latency_team(world, mode):
    from lodestar_amd import native
    jobs, want = _team_call(world["n_team"])
    assert sum(1 for w in want if not w["name"].startswith("valid@")) == len(world["items"])
    got, retries = _run(world["ctx"], jobs, native.MODE_WORKER if mode == "worker" else native.MODE_PER_JOB)
    assert se.mismatches(want, got, lambda w: w["want"]) == []
    codes = {w["name"].split("@")[0]: w["want"] for w in want}
    assert all(codes[e["name"]] == 1 for e in world["corpus"] if e["kind"] == "mixed" and e["verdict"])
    assert all(codes[e["name"]] == 0 for e in world["corpus"] if e["kind"] in ("torsion", "flip"))
    if mode == "worker":
        assert retries >= 1


def test_p6_records_bulk_path(world):
    """The N_TEAM worker-mode call again in a child process whose BGV_LATENCY_MAX=0 sends it down
    the bulk path (as tests/test_gpu_prep_bulk.py does)."""
    _, want = _team_call(world["n_team"])
    env = dict(os.environ, BGV_LATENCY_MAX="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert se.mismatches(want, res["worker"], lambda w: w["want"]) == []
    assert res["retries"] >= 1


def test_two_set_jobs(world):
    """Each multi-record set behind a valid set in a non-batchable job: the blst batch semantics
    (an infinity sum rejects with BLST_PK_IS_INFINITY, a bad record with its code)."""
    from lodestar_amd import native
    p = world["partner"]
    first = native.SetSpec(p["root"], p["sig"], pk_bytes=p["records"])
    jobs = [([first, native.SetSpec(s["root"], s["sig"], pk_bytes=s["records"])], False) for s in world["sets"]]
    assert {s["pair_expect"] for s in world["sets"]} >= {1, 0, -1, -2, -3, -6}
    for mode in (native.MODE_WORKER, native.MODE_PER_JOB):
        got = world["ctx"].verify_jobs(jobs, mode)
        assert se.mismatches(world["sets"], got, lambda s: s["pair_expect"]) == [], mode


def test_shared_root_with_mixed_record(world):
    """Eight sets over one signing root (one uniform group), one of them a mixed-order record."""
    from lodestar_amd import native
    e = next(e for e in world["corpus"] if e["name"] == "mixed_10177")
    assert e["verdict"] == 1
    ctx, signers = world["ctx"], [30, 31, 32, 33, 34, 35, 36]
    sks = b"".join(int(world["keys"]["sk"][k], 16).to_bytes(32, "big") for k in signers)
    sigs = ctx.sign(sks, e["root"] * len(signers))
    sets = [native.SetSpec(e["root"], sigs[96 * j:96 * j + 96], pk_bytes=[world["pk96"][k]])
            for j, k in enumerate(signers)]
    sets.insert(3, native.SetSpec(e["root"], e["sig"], pk_bytes=[e["pk96"]]))
    for mode in (native.MODE_WORKER, native.MODE_PER_JOB):
        assert ctx.verify_jobs([([s], True) for s in sets], mode) == [1] * 8, mode
    assert ctx.verify_jobs([(sets, False)]) == [1]


def test_torsion_key_meets_exceptional_addition(world):
    """k_prep_wide multiplies the key sum on generic-case addition programs (bgv_tg1.h).  A trusted
    key of order 11 meets an exceptional addition for about a third of the randomizers (0x55555555
    is one: tests/test_pk_edges_cpu.py); the kernel then repeats the task with the complete
    formulas.  Before it did, the degenerate point made the group's Miller product 0 and every
    retry test of the group pass, so that each job of the call came back valid.  Every odd job
    carries that key under a valid set's root and signature (verdict 0: e(T, H) = 1), the seed
    puts the word into slot 1, and the other odd slots draw theirs from the same fixed stream."""
    from lodestar_amd import native
    from tests.randomizer_edges import seed_for
    t11 = next(e for e in world["corpus"] if e["name"] == "torsion_11")
    valid = se.golden_valid()
    jobs, want = [], []
    for i in range(WAVE):
        key, root, sig = valid[i % len(valid)]
        rec = t11["pk96"] if i & 1 else world["pk96"][key]
        jobs.append(([native.SetSpec(root, sig, pk_bytes=[rec])], True))
        want.append({"name": "%s@%d" % ("torsion_11" if i & 1 else "valid", i), "want": 0 if i & 1 else 1})
    ctx = world["ctx"]
    ctx.set_rng_seed(seed_for(0x55555555, 1))
    try:
        got, retries = _run(ctx, jobs, native.MODE_WORKER)
    finally:
        ctx.set_rng_seed(0)
    assert se.mismatches(want, got, lambda w: w["want"]) == []
    assert retries >= 1


def test_deposits_verify(world):
    """Every compressed entry as a deposit key with its stored root and signature: valid only where
    o.deposit_valid says so; a mixed-order key with a correct signature is not."""
    edges = pe.with_form(world["corpus"], 48)
    got = world["ctx"].deposits_verify([e["pk48"] for e in edges], [e["root"] for e in edges],
                                       [e["sig"] for e in edges])
    assert se.mismatches(edges, got, lambda e: e["deposit"]) == []
    assert sum(got) >= 3
    assert sum(1 for e in edges if e["kind"] == "mixed" and e["verdict"] == 1 and e["deposit"] == 0) >= 6


def test_comparison_can_fail(world):
    """Negative control: with one item's expected code swapped for its neighbour's, the helper
    names that item alone."""
    from lodestar_amd import native
    jobs, want = _record_jobs(WAVE, world["items"][:WAVE // 2], (0, WAVE - 1))
    got, _ = _run(world["ctx"], jobs, native.MODE_PER_JOB)
    assert se.mismatches(want, got, lambda w: w["want"]) == []
    j = next(k for k in range(len(want) - 1) if want[k]["want"] != want[k + 1]["want"])
    swapped = [dict(w) for w in want]
    swapped[j]["want"] = want[j + 1]["want"]
    bad = se.mismatches(swapped, got, lambda w: w["want"])
    assert len(bad) == 1 and bad[0].startswith(want[j]["name"] + ":")


if __name__ == "__main__":
    _child()
