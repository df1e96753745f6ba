"""GPU: crafted G2 wire bytes (tests/golden/sig_edges.json, tools/gen_golden_sig_edges.py, oracle
only) through the four places where the device decodes a signature, and through the public calls.

  route  kernels                                                          call here
  A      k_sig_decode + k_sig_sum (bgv_k_util.hip)                        aggregate_signatures
  B      bulk k_prep task_sig (bgv_k_tasks.h)                             debug_prepare(PATH_BULK)
  C      task_sig_decode_t<bgv_pow_wave>, k_prep_wide plane 2 (team       debug_prepare(PATH_LATENCY),
         subgroup check, one-lane fallback on an exceptional addition)    64 sets a call
  D      k_prep_a (lane decode), k_prep_team plane 2                      debug_prepare(PATH_LATENCY),
                                                                          N_TEAM sets

The corpus: points of small order on the twist (three of order 13, whose |x| chain meets -P and
infinity, so that route C takes its fallback), a valid signature plus such a point, x chosen so that
y^2 lies in Fp (every arm of fp2_sqrt_t and fp2_lex_largest), x = 0, the field-boundary and flag
encodings, valid signatures with the sort bit flipped (status 0, verdict false) and the wrong
lengths.  Every set names a cached golden key and a real root; valid golden signatures sit between
the edge entries, edge entries at slots 0, 63, 64 and the last.  N_TEAM and the routing threshold
come from bgv_device.h as in tests/test_gpu_randomizer_edges.py.  The sums of route A (more than
64 signatures, equal signatures, a signature and its negative, infinity mid-stride, an empty list
between full ones) are compared with the fixture's aggregates, which the generator took from
o.signatures_aggregate.  Integer work, bit-exact, no tolerance.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)  # the child process runs this file as a script

from tests import sig_edges as se  # noqa: E402

WAVE = 64


def _world_inputs():
    """Everything the calls need but the context, also for the child process: the corpus, the valid
    golden signatures and the one-set jobs of the public calls (an edge entry, then a valid one)."""
    corpus = se.corpus()
    valid = se.golden_valid()
    jobs = []  # (key, root, sig, expected code, name)
    for j, e in enumerate(corpus):
        key, root = se.owner(e, j, valid)
        jobs.append((key, root, e["sig"], -e["expect"], e["name"]))  # 0: a flipped signature, infinity
        jobs.append(valid[j % len(valid)] + (1, "valid_after_" + e["name"]))
    return corpus, valid, jobs


def _context():
    from lodestar_amd import native
    keys = se.load("keys.json")
    c = native.Context([0])
    c.pubkeys_put(0, b"".join(bytes.fromhex(k) for k in keys["pk_compressed"]), native.PK_COMPRESSED)
    return c, keys


def _verify(ctx, jobs, mode):
    from lodestar_amd import native
    st = native.BgvStats()
    got = ctx.verify_jobs([([native.SetSpec(root, sig, pk_indices=[key])], True) for key, root, sig, _, _ in jobs],
                          mode, st)
    return got, st.batch_retries


def _child():
    from lodestar_amd import native
    _, _, jobs = _world_inputs()
    ctx, _ = _context()
    got, retries = _verify(ctx, jobs, native.MODE_WORKER)
    ctx.close()
    print(json.dumps({"worker": got, "retries": retries}))


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    from oracle import bls12381 as o  # checker only
    from tests.test_gpu_randomizer_edges import N_TEAM, PREP_WIDE_MAX, _padded
    corpus, valid, jobs = _world_inputs()
    ctx, keys = _context()
    assert _padded(WAVE) <= PREP_WIDE_MAX < _padded(N_TEAM)  # 64 sets: k_prep_wide; N_TEAM: k_prep_a + k_prep_team
    h192 = {root: o.g2_serialize(o.hash_to_g2(root)) for _, root, _ in valid}  # H(m) of every root used
    yield {"ctx": ctx, "keys": keys, "n_team": N_TEAM, "corpus": corpus, "valid": valid, "jobs": jobs, "h192": h192}
    ctx.close()


def _prepare(world, n, edges, must, path):
    """One debug_prepare call of n sets, the edge entries placed by se.place: the names of the sets
    whose statuses or H(m) are wrong."""
    from lodestar_amd import native
    valid = world["valid"]
    slots = se.place(n, edges, must)
    assert all(s in slots for s in must if s < n)
    # no 64-slot group is all bad (at N_TEAM = 64 k + 1 sets the last set, an edge entry, is a group alone)
    assert all(any(i not in slots for i in range(g, min(g + WAVE, n))) for g in range(0, n, WAVE) if n - g > 1)
    sets, want = [], []
    for i in range(n):
        if i in slots:
            key, root = se.owner(slots[i], i, valid)
            sig, st, name = slots[i]["sig"], se.decode_status(slots[i]), slots[i]["name"]
        else:
            (key, root, sig), st, name = valid[i % len(valid)], 0, "valid"
        sets.append(native.SetSpec(root, sig, pk_indices=[key]))
        want.append({"name": "%s@%d" % (name, i), "status": (st, 0), "h": world["h192"][root]})
    res = world["ctx"].debug_prepare(sets, path, seed=0x51CED6E5 + n)
    bad = se.mismatches(want, [(ss, ps) for _, _, ss, ps in res], lambda w: w["status"])
    bad += se.mismatches(want, [h for h, _, _, _ in res], lambda w: w["h"])
    return bad, len(slots)


def test_route_b_bulk(world):
    from lodestar_amd import native
    edges = world["corpus"]
    bad, n = _prepare(world, 2 * len(edges) + 2, edges, (0, WAVE - 1, WAVE, 2 * len(edges) + 1), native.PATH_BULK)
    assert bad == [] and n == len(edges)


def test_route_c_latency_small(world):
    """k_prep_wide: at most 64 sets a call, so the corpus takes two calls; edge entries at slots
    0 and 63 (the last) of each.  The order-13 entries run the subgroup check's one-lane fallback."""
    from lodestar_amd import native
    edges = world["corpus"]
    half = (len(edges) + 1) // 2
    assert half <= WAVE // 2 + 1
    done = 0
    for part in (edges[:half], edges[half:]):
        bad, n = _prepare(world, WAVE, part, (0, WAVE - 1), native.PATH_LATENCY)
        assert bad == []
        done += n
    assert done == len(edges)
    assert sum(1 for e in edges if e.get("hits_exceptional")) >= 2


def test_route_d_latency_team(world):
    from lodestar_amd import native
    edges, n_team = world["corpus"], world["n_team"]
    bad, n = _prepare(world, n_team, edges, (0, WAVE - 1, WAVE, n_team - 1), native.PATH_LATENCY)
    assert bad == [] and n == len(edges)


def test_route_a_aggregate(world):
    """One aggregation call: every entry alone and between two valid signatures, valid aggregates
    among them, then the sums.  A failing list gives the first failing code and a zeroed output."""
    lists = se.aggregate_lists()
    names = [name for name, _, _, _ in lists]
    for e in world["corpus"]:
        assert "alone_" + e["name"] in names and "between_" + e["name"] in names
    assert max(len(sigs) for _, sigs, _, _ in lists) > 2 * WAVE
    got = world["ctx"].aggregate_signatures([sigs for _, sigs, _, _ in lists])
    want = [{"name": name, "want": (-code, agg if code == 0 else bytes(96))} for name, _, code, agg in lists]
    assert se.mismatches(want, got, lambda w: w["want"]) == []
    by = dict(zip(names, got))
    assert by["cancel"] == (0, bytes([0xC0]) + bytes(95))
    assert by["empty_between_full_runs"][0] == -20


def _want_codes(jobs):
    return [{"name": name, "want": code} for _, _, _, code, name in jobs]


@pytest.mark.parametrize("mode", ["worker", "per_job"])
def test_public_verdicts(world, mode):
    """Every entry as a batchable one-set job between valid ones: -code for what the decoding
    rejects (a mixed-order or small-order point: -3), 0 for a sort-flipped signature."""
    from lodestar_amd import native
    jobs = world["jobs"]
    assert len(jobs) <= 130
    got, retries = _verify(world["ctx"], jobs, native.MODE_WORKER if mode == "worker" else native.MODE_PER_JOB)
    assert se.mismatches(_want_codes(jobs), got, lambda w: w["want"]) == []
    codes = {e["name"]: -e["expect"] for e in world["corpus"]}
    assert all(codes[e["name"]] == 0 for e in world["corpus"] if e["kind"] == "flip")
    assert all(codes[e["name"]] == -3 for e in world["corpus"] if e["kind"] in ("mixed", "small"))
    if mode == "worker":
        assert retries >= 1


def test_deposits_verify(world):
    jobs = [j for j in world["jobs"] if len(j[2]) == 96]
    pk = world["keys"]["pk_compressed"]
    got = world["ctx"].deposits_verify([bytes.fromhex(pk[j[0]]) for j in jobs], [j[1] for j in jobs],
                                       [j[2] for j in jobs])
    want = [{"name": j[4], "want": int(j[3] == 1)} for j in jobs]
    assert se.mismatches(want, got, lambda w: w["want"]) == []
    assert sum(got) == len(world["corpus"])  # the valid ones, one per entry


def test_public_verdicts_bulk_path():
    """The worker-mode call again in a child process whose BGV_LATENCY_MAX=0 sends it down the
    bulk path (as tests/test_gpu_prep_bulk.py does)."""
    _, _, jobs = _world_inputs()
    assert len(jobs) <= 130
    env = dict(os.environ, BGV_LATENCY_MAX="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert se.mismatches(_want_codes(jobs), res["worker"], lambda w: w["want"]) == []
    assert res["retries"] >= 1


def test_comparison_can_fail(world):
    """Negative control: with one entry's expected code swapped for its neighbour's, the helper
    reports that entry and no other."""
    from lodestar_amd import native
    wire = [e for e in world["corpus"] if len(e["sig"]) == 96][:WAVE // 2]
    slots = se.place(WAVE, wire, (0, WAVE - 1))
    order = sorted(slots)
    valid = world["valid"]
    sets = []
    for i in range(WAVE):
        key, root = se.owner(slots[i], i, valid) if i in slots else valid[i % len(valid)][:2]
        sets.append(native.SetSpec(root, slots[i]["sig"] if i in slots else valid[i % len(valid)][2], pk_indices=[key]))
    res = world["ctx"].debug_prepare(sets, native.PATH_LATENCY, seed=7)
    got = [res[i][2] for i in order]
    entries = [slots[i] for i in order]
    assert se.mismatches(entries, got) == []
    j = next(k for k in range(len(entries) - 1) if se.decode_status(entries[k]) != se.decode_status(entries[k + 1]))
    swapped = [dict(e) for e in entries]
    swapped[j]["expect"], swapped[j]["infinity"] = entries[j + 1]["expect"], entries[j + 1].get("infinity")
    bad = se.mismatches(swapped, got)
    assert len(bad) == 1 and bad[0].startswith(entries[j]["name"] + ":")


if __name__ == "__main__":
    _child()
