"""CPU checks of bgv_verify_aggregate's host side: the plan (lodestar_amd/csrc/bgv_sigagg_plan.h,
run through tests/native/sigaggsim.cpp, a program of its own, also built under
-fsanitize=address,undefined) against the Python model of the contract (tests/sigaggsim.py), and
the header and binding.  The kernels are checked on the GPU (tests/test_gpu_verify_aggregate.py)."""
import ctypes
import os
import random
import re

import pytest

from tests import sigaggsim as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = sim.NO_AGG
KINDS = ["O2", "san"]


def _one_set_jobs(codes):
    return [(i, 1, c) for i, c in enumerate(codes)]


def edge_cases(wave_max):
    w = wave_max
    return {
        "naggs_0": (_one_set_jobs([1, 1, 0]), [0, NO, 7], 0, w),  # the tags are not read
        "naggs_1": (_one_set_jobs([1, 0, 1, 1]), [0, 0, NO, 0], 1, w),
        "all_untagged": (_one_set_jobs([1, 1, 1]), [NO, NO, NO], 2, w),
        "all_rejected": (_one_set_jobs([0, 0, 0, 0]), [0, 1, 0, 1], 2, w),
        "negative_codes": (_one_set_jobs([1, -8, -3, 1, -30]), [0, 0, 0, 0, 0], 1, w),
        "code_2_is_not_accepted": (_one_set_jobs([2, 1]), [0, 0], 1, w),
        "multi_set_job_splits": ([(0, 3, 1), (3, 3, 0), (6, 1, 1)], [0, 1, 0, 0, 1, 1, 1], 2, w),
        "interleaved": (_one_set_jobs([1] * 9), [2, 0, 1, 2, 0, 1, 2, 0, 1], 3, w),
        "empty_aggregates_between": (_one_set_jobs([1, 1, 1]), [4, 0, 4], 6, w),
        "jobs_out_of_order": ([(3, 2, 1), (0, 3, 1)], [1, 0, 1, 0, 1], 2, w),
        "set_in_no_job": ([(1, 1, 1)], [0, 0, 0], 1, w),
        "no_sets": ([], [], 3, w),
        "empty_job": ([(0, 0, -21), (0, 1, 1)], [0], 1, w),
        "count_wave_max": (_one_set_jobs([1] * w + [0]), [0] * (w + 1), 1, w),
        "count_wave_max_plus_1": (_one_set_jobs([1] * (w + 1)), [i % 2 for i in range(w + 1)], 2, w),
        "count_wave_max_minus_1": (_one_set_jobs([1] * (w - 1)), [0] * (w - 1), 1, w),
        "wave_max_0_is_always_bulk": (_one_set_jobs([1]), [0], 1, 0),
        "tag_equals_naggs": (_one_set_jobs([1, 1]), [0, 2], 2, w),
        "tag_just_below_no_agg": (_one_set_jobs([1]), [NO - 1], 1, w),
        "bad_tag_on_a_rejected_set": (_one_set_jobs([0, 1]), [9, 0], 1, w),
        "too_many_aggregates": (_one_set_jobs([1]), [0], (1 << 20) + 1, w),
        "most_aggregates": (_one_set_jobs([1, 1]), [(1 << 20) - 1, 0], 1 << 20, w),
    }


def random_cases(seed, n):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        nsets, naggs, wave_max = rnd.randrange(0, 40), rnd.randrange(0, 6), rnd.choice([0, 1, 4, 16, 64])
        jobs, at = [], 0
        while at < nsets:
            k = min(nsets - at, rnd.choice([1, 1, 1, 2, 3, 7]))
            if rnd.random() < 0.1:  # a gap: sets no job holds
                at += k
                continue
            jobs.append((at, k, rnd.choice([1, 1, 1, 0, -8, -3, 2])))
            at += k
        rnd.shuffle(jobs)
        bad = rnd.random() < 0.1
        tags = [NO if rnd.random() < 0.2 else rnd.randrange(0, max(1, naggs + (1 if bad else 0))) for _ in range(nsets)]
        out.append((jobs, tags, naggs, wave_max))
    return out


def test_constants_agree():
    """BGV_NO_AGG and BGV_SIGAGG_WAVE_MAX: the header, the plan's driver and the binding."""
    from lodestar_amd import native
    no_agg, wave_max, max_aggs = sim.consts()
    assert (no_agg, max_aggs) == (NO, 1 << 20)
    assert (native.NO_AGG, native.SIGAGG_WAVE_MAX) == (no_agg, wave_max)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    assert re.search(r"#define BGV_SIGAGG_WAVE_MAX %d\b" % wave_max, src)


@pytest.mark.parametrize("kind", KINDS)
def test_plan_edge_cases(kind):
    cases = edge_cases(sim.consts()[1])
    got = sim.run(list(cases.values()), kind)
    bad = [name for (name, c), g in zip(cases.items(), got) if g != sim.model(*c)]
    assert not bad, bad
    # and what the model itself must say about a few of them
    by = dict(zip(cases, got))
    w = sim.consts()[1]
    assert by["naggs_0"] == (sim.FORM_NONE, [], [], [])
    assert by["multi_set_job_splits"] == (sim.FORM_WAVE, [0, 2], [2, 2], [0, 2, 1, 6])
    assert by["interleaved"][3] == [1, 4, 7, 2, 5, 8, 0, 3, 6]
    assert by["negative_codes"][2:] == ([2], [0, 3])
    assert by["all_rejected"] == (sim.FORM_NONE, [0, 0], [0, 0], [])
    assert by["count_wave_max"][0] == sim.FORM_WAVE and by["count_wave_max"][2] == [w]
    assert by["count_wave_max_plus_1"][0] == sim.FORM_BULK
    assert by["count_wave_max_minus_1"][0] == sim.FORM_WAVE
    assert by["wave_max_0_is_always_bulk"][0] == sim.FORM_BULK
    for name in ("tag_equals_naggs", "tag_just_below_no_agg", "bad_tag_on_a_rejected_set", "too_many_aggregates"):
        assert by[name] == -sim.E_ARG, name
    assert by["most_aggregates"][3] == [1, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_plan_random_tables(kind):
    cases = random_cases(0x51A66 if kind == "O2" else 0x51A67, 400)
    got = sim.run(cases, kind)
    bad = [i for i, (c, g) in enumerate(zip(cases, got)) if g != sim.model(*c)]
    assert not bad, (bad[:5], cases[bad[0]], got[bad[0]])
    assert any(g == -sim.E_ARG for g in got) and any(g != -sim.E_ARG and g[0] == sim.FORM_BULK for g in got)


def test_symbols_declared_exported_and_bound():
    from lodestar_amd import build, native
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    lib = ctypes.CDLL(build.build(verbose=False))
    L = native.load()
    for name in ("bgv_verify_aggregate", "bgv_verify_aggregate_async", "bgv_debug_sigagg_launches"):
        assert re.search(r"\bint %s\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert callable(native.Context.verify_aggregate) and callable(native.Context.verify_aggregate_async)


def test_pkbits_call_converts_to_spans():
    """PackedCall.as_spans: a (committee, bitfield) set is the span over that one committee."""
    from lodestar_amd import native
    msg, sig = bytes(32), bytes(96)
    plain = native.SetSpec(msg, sig, pk_indices=[3])
    com = native.SetSpec(msg, sig, committee=9, bits=b"\x05", n_bits=3)
    assert native.PackedCall([([plain], True)]).as_spans() is None
    p = native.PackedCall([([plain, com], True)])
    assert p.spans is None and p.pkbits is not None
    spans = p.as_spans()
    assert spans[0].n_committees == 0
    assert (spans[1].n_committees, spans[1].n_bits) == (1, 3)
    assert ctypes.cast(spans[1].committees, ctypes.POINTER(ctypes.c_uint32))[0] == 9
    assert ctypes.string_at(spans[1].bits, 1) == b"\x05"
