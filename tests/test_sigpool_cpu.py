"""CPU checks of the signature pools' host side: the tag check and the plan
(lodestar_amd/csrc/bgv_sigpool_plan.h, run through tests/native/sigpoolsim.cpp, a program of its
own, also built under -fsanitize=address,undefined) against the Python model of the contract
(tests/sigpoolsim.py), and the header and binding.  The kernels are checked on the GPU
(tests/test_gpu_sigpool.py)."""
import ctypes
import os
import random
import re

import pytest

from tests import sigpoolsim as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = sim.NO_AGG
KINDS = ["O2", "san"]
SYMBOLS = ("bgv_sigpool_open", "bgv_sigpool_drop_range", "bgv_sigpool_get", "bgv_verify_accumulate",
           "bgv_verify_accumulate_async", "bgv_debug_sigpool_launches")


def _one_set_jobs(codes):
    return [(i, 1, c) for i, c in enumerate(codes)]


def edge_cases(wave_max, max_pool):
    w, top = wave_max, max_pool - 1
    return {
        "tag_equals_max_sigpool": (_one_set_jobs([1, 1]), [0, max_pool], {0: 1}, {}, w),
        "tag_just_below_no_agg": (_one_set_jobs([1]), [NO - 1], {0: 1}, {}, w),
        "tag_on_a_not_live_id": (_one_set_jobs([1, 1]), [0, 5], {0: 1}, {}, w),
        "bad_tag_on_a_rejected_set": (_one_set_jobs([0, 1]), [max_pool + 9, 0], {0: 1}, {}, w),
        "not_live_tag_on_a_rejected_set": (_one_set_jobs([0, 1]), [3, 0], {0: 1}, {}, w),
        "bad_tag_beats_not_live_tag": (_one_set_jobs([1, 1]), [5, max_pool], {0: 1}, {}, w),
        "sparse_ids_ascend": (_one_set_jobs([1] * 5), [top, 0, 7, top, 0], {top: 3, 0: 1, 7: 2}, {}, w),
        "multi_set_job_splits": ([(0, 3, 1), (3, 3, 0), (6, 1, 1)], [4, 9, 4, 4, 9, 9, 9], {4: 1, 9: 1}, {}, w),
        "set_in_no_job": ([(1, 1, 1)], [2, 2, 2], {2: 1}, {}, w),
        "code_2_is_not_accepted": (_one_set_jobs([2, 1]), [0, 0], {0: 1}, {}, w),
        "negative_codes": (_one_set_jobs([1, -8, -3, 1, -30]), [1] * 5, {1: 6}, {}, w),
        "all_untagged": (_one_set_jobs([1, 1, 1]), [NO, NO, NO], {}, {}, w),
        "all_rejected": (_one_set_jobs([0, 0]), [0, 1], {0: 1, 1: 1}, {}, w),
        "no_sets": ([], [], {3: 1}, {}, w),
        "dropped_since_submit": (_one_set_jobs([1] * 4), [1, 2, 1, 2], {1: 1, 2: 1}, {2: (0, 1)}, w),
        "reopened_since_submit": (_one_set_jobs([1] * 4), [1, 2, 1, 2], {1: 4, 2: 9}, {1: (1, 5)}, w),
        "all_entries_gone": (_one_set_jobs([1, 1]), [1, 2], {1: 1, 2: 1}, {1: (0, 1), 2: (1, 2)}, w),
        "opened_since_submit_is_no_help": (_one_set_jobs([1, 1]), [1, NO], {1: 1}, {8: (1, 1)}, w),
        "count_wave_max_minus_1": (_one_set_jobs([1] * (w - 1)), [0] * (w - 1), {0: 1}, {}, w),
        "count_wave_max": (_one_set_jobs([1] * w + [0]), [0] * (w + 1), {0: 1}, {}, w),
        "count_wave_max_plus_1": (_one_set_jobs([1] * (w + 1)), [i % 2 for i in range(w + 1)], {0: 1, 1: 1}, {}, w),
        "dropped_sets_do_not_count_for_the_form": (_one_set_jobs([1] * (w + 1)), [0] * w + [1], {0: 1, 1: 1},
                                                   {1: (0, 1)}, w),
        "wave_max_0_is_always_bulk": (_one_set_jobs([1]), [0], {0: 1}, {}, 0),
    }


def random_cases(seed, n, max_pool):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        nsets, wave_max = rnd.randrange(0, 40), rnd.choice([0, 1, 4, 16, 64])
        pool = rnd.sample([0, 1, 2, 7, 100, 4095, max_pool - 2, max_pool - 1], rnd.randrange(1, 6))
        live = {i: rnd.randrange(1, 5) for i in pool}
        jobs, at = [], 0
        while at < nsets:
            k = min(nsets - at, rnd.choice([1, 1, 1, 2, 3, 7]))
            if rnd.random() < 0.1:  # a gap: sets no job holds
                at += k
                continue
            jobs.append((at, k, rnd.choice([1, 1, 1, 0, -8, -3, 2])))
            at += k
        rnd.shuffle(jobs)
        tags = [NO if rnd.random() < 0.2 else rnd.choice(pool) for _ in range(nsets)]
        if nsets and rnd.random() < 0.08:
            tags[rnd.randrange(nsets)] = rnd.choice([max_pool, NO - 1, 1 << 20])
        if nsets and rnd.random() < 0.08:
            tags[rnd.randrange(nsets)] = 5000  # never live
        changed = {}
        for i in pool:
            r = rnd.random()
            if r < 0.15:
                changed[i] = (0, live[i])  # dropped
            elif r < 0.3:
                changed[i] = (1, live[i] + 1)  # dropped and opened again
        out.append((jobs, tags, live, changed, wave_max))
    return out


def test_constants_agree():
    """BGV_MAX_SIGPOOL: the header, the plan's driver and the binding; the threshold between the
    decoding forms is bgv_verify_aggregate's, not a second one."""
    from lodestar_amd import native
    no_agg, wave_max, max_pool = sim.consts()
    assert (no_agg, max_pool) == (NO, 16384)
    assert (native.NO_AGG, native.SIGAGG_WAVE_MAX, native.MAX_SIGPOOL) == (no_agg, wave_max, max_pool)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    assert re.search(r"#define BGV_MAX_SIGPOOL %d\b" % max_pool, src)
    plan = open(os.path.join(ROOT, "lodestar_amd", "csrc", "bgv_sigpool_plan.h")).read()
    assert "sigagg_form(" in plan and "#define" not in plan


@pytest.mark.parametrize("kind", KINDS)
def test_plan_edge_cases(kind):
    _, w, max_pool = sim.consts()
    cases = edge_cases(w, max_pool)
    got = sim.run(list(cases.values()), kind)
    bad = [name for (name, c), g in zip(cases.items(), got) if g != sim.model(*c, max_pool=max_pool)]
    assert not bad, bad
    # and what the model itself must say about a few of them
    by = dict(zip(cases, got))
    top = max_pool - 1
    for name in ("tag_equals_max_sigpool", "tag_just_below_no_agg", "bad_tag_on_a_rejected_set",
                 "bad_tag_beats_not_live_tag"):
        assert by[name] == -sim.E_ARG, name
    for name in ("tag_on_a_not_live_id", "not_live_tag_on_a_rejected_set"):
        assert by[name] == -sim.E_BAD_INDEX, name
    assert by["sparse_ids_ascend"] == (sim.FORM_WAVE, [0, 7, top], [0, 2, 3], [2, 1, 2], [1, 4, 2, 0, 3],
                                       [3, 1, 2, 3, 1])
    assert by["multi_set_job_splits"][1:5] == ([4, 9], [0, 2], [2, 2], [0, 2, 1, 6])
    assert by["set_in_no_job"][1:5] == ([2], [0], [1], [1])
    assert by["code_2_is_not_accepted"][4] == [1]
    assert by["negative_codes"][3:5] == ([2], [0, 3])
    assert by["all_untagged"][:5] == (sim.FORM_NONE, [], [], [], [])
    assert by["all_rejected"][:5] == (sim.FORM_NONE, [], [], [], [])
    assert by["dropped_since_submit"][1:5] == ([1], [0], [2], [0, 2])
    assert by["reopened_since_submit"][1:5] == ([2], [0], [2], [1, 3])
    assert by["all_entries_gone"][:5] == (sim.FORM_NONE, [], [], [], [])
    assert by["opened_since_submit_is_no_help"][1:5] == ([1], [0], [1], [0])
    assert by["count_wave_max_minus_1"][0] == sim.FORM_WAVE
    assert by["count_wave_max"][0] == sim.FORM_WAVE and by["count_wave_max"][3] == [w]
    assert by["count_wave_max_plus_1"][0] == sim.FORM_BULK and by["count_wave_max_plus_1"][1] == [0, 1]
    assert by["dropped_sets_do_not_count_for_the_form"][0] == sim.FORM_WAVE
    assert by["wave_max_0_is_always_bulk"][0] == sim.FORM_BULK


@pytest.mark.parametrize("kind", KINDS)
def test_plan_random_tables(kind):
    max_pool = sim.consts()[2]
    cases = random_cases(0x5169001 if kind == "O2" else 0x5169002, 400, max_pool)
    got = sim.run(cases, kind)
    bad = [i for i, (c, g) in enumerate(zip(cases, got)) if g != sim.model(*c, max_pool=max_pool)]
    assert not bad, (bad[:5], cases[bad[0]], got[bad[0]])
    assert any(g == -sim.E_ARG for g in got) and any(g == -sim.E_BAD_INDEX for g in got)
    plans = [g for g in got if not isinstance(g, int)]
    assert any(g[0] == sim.FORM_BULK for g in plans) and any(g[0] == sim.FORM_WAVE for g in plans)
    # some case lost an entry between submit and step and kept another
    assert any(g[1] and any(t in c[3] for t in c[1]) and not any(i in c[3] for i in g[1])
               for c, g in zip(cases, got) if not isinstance(g, int))


def test_symbols_declared_exported_and_bound():
    from lodestar_amd import build, native
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    lib = ctypes.CDLL(build.build(verbose=False))
    L = native.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None
    for method in ("sigpool_open", "sigpool_drop_range", "sigpool_get", "verify_accumulate",
                   "verify_accumulate_async", "sigpool_launches"):
        assert callable(getattr(native.Context, method)), method
    from lodestar_amd.verifier import BlsGpuVerifier
    assert callable(BlsGpuVerifier.verify_and_pool_same_message)
