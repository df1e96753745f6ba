"""CPU checks of pool entries with participation bits: the bits check at submit, the step's plan,
its commit and bgv_sigpool_sum's bit concatenation (lodestar_amd/csrc/bgv_sigpool_bits_plan.h, run
through tests/native/sigpoolbitssim.cpp, a program of its own, also built under
-fsanitize=address,undefined) against the Python model of the contract (tests/sigpoolbitssim.py),
and the header and binding.  The kernel and the calls are checked on the GPU
(tests/test_gpu_sigpool_bits.py)."""
import ctypes
import os
import random
import re

import pytest

from tests import sigpoolbitssim as sim
from tests.sigpoolbitssim import ADDED, KNOWN, NOT_ADDED, OVERLAP, Entry, Member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = sim.NO_AGG
KINDS = ["O2", "san"]
SYMBOLS = ("bgv_sigpool_open_bits", "bgv_verify_accumulate_bits", "bgv_verify_accumulate_bits_async",
           "bgv_sigpool_get_bits", "bgv_sigpool_sum")
NBITS = (1, 7, 8, 9, 130, 2048)


def _jobs(codes):
    return [(i, 1, c) for i, c in enumerate(codes)]


def _singles(n_bits, positions):
    return [Member(n_bits, bit=b) for b in positions]


def edge_cases(w):
    c = {}
    for n in NBITS:
        e = {3: Entry(n_bits=n)}
        c["single_first_and_last_%d" % n] = (_jobs([1, 1]), [3, 3], _singles(n, [0, n - 1]), e, {}, {}, w)
        c["single_at_n_bits_%d" % n] = (_jobs([1]), [3], _singles(n, [n]), e, {}, {}, w)
        c["field_full_%d" % n] = (_jobs([1]), [3], [Member(n, field=range(n))], e, {}, {}, w)
        c["field_last_position_%d" % n] = (_jobs([1, 1]), [3, 3],
                                           [Member(n, field=[n - 1]), Member(n, field=[0, n - 1])], e, {}, {}, w)
        c["field_empty_%d" % n] = (_jobs([1]), [3], [Member(n, field=[])], e, {}, {}, w)
        c["n_bits_mismatch_%d" % n] = (_jobs([1]), [3], [Member(n + 1, bit=0)], e, {}, {}, w)
        if n % 8:
            c["stray_bit_%d" % n] = (_jobs([1]), [3], [Member(n, field=[0, n])], e, {}, {}, w)
            c["stray_top_bit_%d" % n] = (_jobs([1]), [3], [Member(n, field=[0, 8 * ((n + 7) // 8) - 1])], e, {}, {}, w)
    e = {1: Entry(n_bits=130), 2: Entry(gen=4)}
    c["error_on_a_rejected_set"] = (_jobs([0, 1]), [1, 1], _singles(130, [130, 0]), e, {}, {}, w)
    c["null_with_a_bits_entry"] = (_jobs([1, 1]), [2, 1], None, e, {}, {}, w)
    c["null_without_a_bits_entry"] = (_jobs([1, 1, 0]), [2, NO, 2], None, e, {}, {}, w)
    c["plain_entry_ignores_its_member"] = (_jobs([1, 1, 1]), [2, 1, 2],
                                           [Member(77, bit=99), Member(130, bit=5), Member(0, field=[])], e, {}, {}, w)
    c["untagged_set_ignores_its_member"] = (_jobs([1, 1]), [NO, 1], [Member(5, bit=9), Member(130, bit=129)], e, {}, {},
                                            w)
    c["tag_errors_come_first"] = (_jobs([1, 1]), [1, 9], _singles(130, [500, 0]), e, {}, {}, w)
    e4 = {0: Entry(n_bits=4)}
    A, B, C = Member(4, field=[0, 1]), Member(4, field=[1, 2]), Member(4, field=[2, 3])
    c["order_a_b_c"] = (_jobs([1, 1, 1]), [0, 0, 0], [A, B, C], e4, {}, {}, w)
    c["order_a_a"] = (_jobs([1, 1]), [0, 0], [A, A], e4, {}, {}, w)
    c["order_a_superset_of_b"] = (_jobs([1, 1]), [0, 0], [B, Member(4, field=[0, 1, 2])], e4, {}, {}, w)
    c["order_rejected_a_frees_b"] = (_jobs([0, 1, 1]), [0, 0, 0], [A, B, C], e4, {}, {}, w)
    c["order_against_stored_bits"] = (_jobs([1, 1, 1]), [0, 0, 0], [A, B, Member(4, bit=3)],
                                      {0: Entry(count=2, n_bits=4, bits=[0, 1])}, {}, {}, w)
    c["order_two_entries_interleaved"] = (_jobs([1] * 4), [0, 5, 0, 5], [A, A, B, C],
                                          {0: Entry(n_bits=4), 5: Entry(n_bits=4)}, {}, {}, w)
    c["multi_set_job"] = ([(0, 2, 1), (2, 2, 0)], [0, 0, 0, 0], [A, C, A, C], e4, {}, {}, w)
    e2 = {1: Entry(gen=2, n_bits=8), 2: Entry(gen=3, n_bits=8)}
    m = _singles(8, [0, 1, 0, 1])
    c["dropped_since_submit"] = (_jobs([1] * 4), [1, 2, 1, 2], m, e2, {2: Entry(gen=3, live=0)}, {}, w)
    c["reopened_with_other_n_bits"] = (_jobs([1] * 4), [1, 2, 1, 2], m, e2, {1: Entry(gen=3, n_bits=16)}, {}, w)
    c["reopened_as_plain"] = (_jobs([1] * 4), [1, 2, 1, 2], m, e2, {1: Entry(gen=3)}, {}, w)
    c["filled_since_submit"] = (_jobs([1] * 4), [1, 2, 1, 2], m, e2,
                                {1: Entry(gen=2, count=1, n_bits=8, bits=[0])}, {}, w)
    c["flagged_entry"] = (_jobs([1] * 5), [1, 2, 1, 2, 1], _singles(8, [0, 1, 0, 2, 3]),
                          {1: Entry(gen=2, count=1, n_bits=8, bits=[7]), 2: Entry(gen=3, n_bits=8)}, {}, {1: -3}, w)
    c["flag_on_an_untouched_entry"] = (_jobs([1, 1]), [1, 2], _singles(8, [7, 1]),
                                       {1: Entry(gen=2, count=1, n_bits=8, bits=[7]), 2: Entry(gen=3, n_bits=8)}, {},
                                       {1: -3}, w)
    # n_add distinct (entry, position) pairs over two entries, then 40 of them again: the form
    # follows the n_add members to add, not the n_add + 40 tagged sets
    big = {0: Entry(n_bits=2048), 1: Entry(n_bits=2048)}
    for wm in (16, w):
        for n_add in (wm, wm + 1):
            k = list(range(n_add)) + [v % n_add for v in range(40)]
            c["added_%d_at_wave_max_%d" % (n_add, wm)] = (_jobs([1] * len(k)), [v % 2 for v in k],
                                                          _singles(2048, [v // 2 for v in k]), big, {}, {}, wm)
    c["all_known"] = (_jobs([1, 1]), [0, 0], _singles(4, [0, 1]), {0: Entry(count=2, n_bits=4, bits=[0, 1])}, {}, {}, w)
    c["no_sets"] = ([], [], [], e4, {}, {}, w)
    return c


def random_cases(seed, n):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        nsets, wave_max = rnd.randrange(0, 40), rnd.choice([0, 1, 4, 16, 64])
        pool = rnd.sample([0, 1, 2, 7, 100, 4095, 16382, 16383], rnd.randrange(1, 6))
        entries = {}
        for i in pool:
            nb = rnd.choice([0, 1, 5, 8, 9, 16, 130])
            bits = [k for k in range(nb) if rnd.random() < 0.25]
            entries[i] = Entry(gen=rnd.randrange(1, 5), count=len(bits), n_bits=nb, bits=bits)
        jobs, at = [], 0
        while at < nsets:
            k = min(nsets - at, rnd.choice([1, 1, 1, 2, 3, 7]))
            if rnd.random() < 0.1:
                at += k
                continue
            jobs.append((at, k, rnd.choice([1, 1, 1, 1, 0, -8, 2])))
            at += k
        rnd.shuffle(jobs)
        tags = [NO if rnd.random() < 0.15 else rnd.choice(pool) for _ in range(nsets)]
        if nsets and rnd.random() < 0.04:
            tags[rnd.randrange(nsets)] = rnd.choice([16384, NO - 1])
        if nsets and rnd.random() < 0.04:
            tags[rnd.randrange(nsets)] = 5000  # never live
        members = []
        for t in tags:
            nb = entries[t].n_bits if t in entries else 0
            if nb == 0:
                members.append(Member(rnd.randrange(0, 9), bit=rnd.randrange(0, 9)))
            elif rnd.random() < 0.5:
                members.append(Member(nb, bit=rnd.randrange(nb)))
            else:
                members.append(Member(nb, field=rnd.sample(range(nb), rnd.randrange(1, min(nb, 4) + 1))))
            r = rnd.random()
            if nb and r < 0.01:
                members[-1] = Member(nb + rnd.choice([-1, 1, 8]), bit=0)
            elif nb and r < 0.02:
                members[-1] = Member(nb, bit=nb + rnd.randrange(3))
            elif nb % 8 and r < 0.03:
                members[-1] = Member(nb, field=[0, nb])
            elif nb and r < 0.04:
                members[-1] = Member(nb, field=[])
        use = None if rnd.random() < 0.05 else members
        changed, flags = {}, {}
        for i in pool:
            r, e = rnd.random(), entries[i]
            if r < 0.1:
                changed[i] = Entry(gen=e.gen, live=0)
            elif r < 0.2:
                changed[i] = Entry(gen=e.gen + 1, n_bits=rnd.choice([0, e.n_bits, 12]))
            elif r < 0.3 and e.n_bits:
                more = set(e.bits) | {rnd.randrange(e.n_bits)}
                changed[i] = Entry(gen=e.gen, count=e.count + len(more) - len(e.bits), n_bits=e.n_bits, bits=more)
            elif r < 0.4:
                flags[i] = -rnd.choice([1, 2, 3])
        out.append((jobs, tags, use, entries, changed, flags, wave_max))
    return out


def test_constants_agree():
    from lodestar_amd import native
    c = sim.consts()
    assert c[:3] == (NO, native.SIGAGG_WAVE_MAX, native.MAX_SIGPOOL)
    assert c[3:6] == (2048, 256, 64)
    assert c[3:6] == (native.SIGPOOL_MAX_BITS, native.SIGPOOL_BITS_BYTES, native.MAX_SUM_ENTRIES)
    assert c[6:] == (NOT_ADDED, ADDED, KNOWN, OVERLAP) == (0, 1, 2, 3)
    assert c[6:] == (native.POOL_NOT_ADDED, native.POOL_ADDED, native.POOL_KNOWN, native.POOL_OVERLAP)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    for name, v in (("BGV_SIGPOOL_MAX_BITS", 2048), ("BGV_SIGPOOL_BITS_BYTES", 256), ("BGV_MAX_SUM_ENTRIES", 64)):
        assert re.search(r"#define %s %d\b" % (name, v), src), name
    m = re.search(r"#define BGV_MAX_SET_COMMITTEES (\d+)", src)
    assert m and int(m.group(1)) == 64


@pytest.mark.parametrize("kind", KINDS)
def test_plan_edge_cases(kind):
    w = sim.consts()[1]
    cases = edge_cases(w)
    got = sim.run(list(cases.values()), kind)
    bad = [name for (name, c), g in zip(cases.items(), got) if g != sim.model(*c)]
    assert not bad, bad
    # and what the contract itself says about them, whatever the model does
    by = dict(zip(cases, got))
    for n in NBITS:
        g = by["single_first_and_last_%d" % n]
        assert g[5] == ([ADDED, KNOWN] if n == 1 else [ADDED, ADDED]), n
        assert g[6][3] == ((1, 1, {0}) if n == 1 else (2, n, {0, n - 1})), n
        assert by["field_full_%d" % n][6][3] == (1, n, set(range(n))), n
        g = by["field_last_position_%d" % n]
        assert g[5] == [ADDED, KNOWN if n == 1 else OVERLAP] and g[6][3] == (1, n, {n - 1}), n
        for name in ("single_at_n_bits_%d", "field_empty_%d", "n_bits_mismatch_%d"):
            assert by[name % n] == -sim.E_ARG, name % n
        if n % 8:
            assert by["stray_bit_%d" % n] == by["stray_top_bit_%d" % n] == -sim.E_ARG, n
    assert by["error_on_a_rejected_set"] == by["null_with_a_bits_entry"] == -sim.E_ARG
    assert by["tag_errors_come_first"] == -sim.E_BAD_INDEX
    g = by["null_without_a_bits_entry"]
    assert g[1:6] == ([2], [0], [1], [0], [ADDED, NOT_ADDED, NOT_ADDED]) and g[6][2][0] == 1
    g = by["plain_entry_ignores_its_member"]
    assert g[1:6] == ([1, 2], [0, 1], [1, 2], [1, 0, 2], [ADDED] * 3)
    assert g[6] == {1: (1, 130, {5}), 2: (2, 0, set())}
    assert by["untagged_set_ignores_its_member"][5] == [NOT_ADDED, ADDED]
    g = by["order_a_b_c"]
    assert g[4:6] == ([0, 2], [ADDED, OVERLAP, ADDED]) and g[6][0] == (2, 4, {0, 1, 2, 3})
    g = by["order_a_a"]
    assert g[4:6] == ([0], [ADDED, KNOWN]) and g[6][0] == (1, 4, {0, 1})
    g = by["order_a_superset_of_b"]
    assert g[4:6] == ([0], [ADDED, OVERLAP]) and g[6][0] == (1, 4, {1, 2})
    g = by["order_rejected_a_frees_b"]
    assert g[4:6] == ([1], [NOT_ADDED, ADDED, OVERLAP]) and g[6][0] == (1, 4, {1, 2})
    g = by["order_against_stored_bits"]
    assert g[4:6] == ([2], [KNOWN, OVERLAP, ADDED]) and g[6][0] == (3, 4, {0, 1, 3})
    g = by["order_two_entries_interleaved"]
    assert g[1:6] == ([0, 5], [0, 1], [1, 2], [0, 1, 3], [ADDED, ADDED, OVERLAP, ADDED])
    assert g[6] == {0: (1, 4, {0, 1}), 5: (2, 4, {0, 1, 2, 3})}
    assert by["multi_set_job"][4:6] == ([0, 1], [ADDED, ADDED, NOT_ADDED, NOT_ADDED])
    g = by["dropped_since_submit"]
    assert g[4:6] == ([0], [ADDED, NOT_ADDED, KNOWN, NOT_ADDED]) and g[6] == {1: (1, 8, {0})}
    for name in ("reopened_with_other_n_bits", "reopened_as_plain"):
        g = by[name]
        assert g[1] == [2] and g[5] == [NOT_ADDED, ADDED, NOT_ADDED, KNOWN], name
        assert g[6][1][0] == 0 and g[6][1][2] == set() and g[6][2] == (1, 8, {1}), name
    g = by["filled_since_submit"]
    assert g[5] == [KNOWN, ADDED, KNOWN, KNOWN] and g[6][1] == (1, 8, {0})
    g = by["flagged_entry"]  # entry 1: nothing committed and all of its sets 0, the known one too
    assert g[1:5] == ([1, 2], [0, 2], [2, 2], [0, 4, 1, 3])
    assert g[5] == [NOT_ADDED, ADDED, NOT_ADDED, ADDED, NOT_ADDED]
    assert g[6] == {1: (1, 8, {7}), 2: (2, 8, {1, 2})}
    g = by["flag_on_an_untouched_entry"]  # nothing of entry 1 went to the device: nothing to flag
    assert g[1] == [2] and g[5] == [KNOWN, ADDED] and g[6][1] == (1, 8, {7})
    for wm in (16, w):
        for n_add, form in ((wm, sim.FORM_WAVE), (wm + 1, sim.FORM_BULK)):
            g = by["added_%d_at_wave_max_%d" % (n_add, wm)]
            assert g[0] == form and len(g[4]) == n_add and g[5].count(KNOWN) == 40, (n_add, wm)
            assert g[5].count(ADDED) == n_add and g[6][0][0] + g[6][1][0] == n_add, (n_add, wm)
    g = by["all_known"]
    assert g[:6] == (sim.FORM_NONE, [], [], [], [], [KNOWN, KNOWN]) and g[6][0] == (2, 4, {0, 1})
    assert by["no_sets"][:6] == (sim.FORM_NONE, [], [], [], [], [])


@pytest.mark.parametrize("kind,seed", [("O2", 0xB175001), ("O2", 0xB175002), ("san", 0xB175003)])
def test_plan_random_tables(kind, seed):
    cases = random_cases(seed, 300)
    got = sim.run(cases, kind)
    bad = [i for i, (c, g) in enumerate(zip(cases, got)) if g != sim.model(*c)]
    assert not bad, (bad[:5], got[bad[0]], sim.model(*cases[bad[0]]))
    assert any(g == -sim.E_ARG for g in got) and any(g == -sim.E_BAD_INDEX for g in got)
    plans = [g for g in got if not isinstance(g, int)]
    for v in (NOT_ADDED, ADDED, KNOWN, OVERLAP):
        assert any(v in g[5] for g in plans), v
    assert any(g[0] == sim.FORM_BULK for g in plans) and any(g[0] == sim.FORM_WAVE for g in plans)
    # some flagged entry had members to add, and some plan found nothing to add among accepted sets
    assert any(any(i in c[5] for i in g[1]) for c, g in zip(cases, got) if not isinstance(g, int))
    assert any(g[0] == sim.FORM_NONE and KNOWN in g[5] for g in plans)


def concat_lists():
    rnd = random.Random(0xC0CA7)
    some = lambda n: [k for k in range(n) if rnd.random() < 0.5]
    lists = {
        "130_5_128": [(130, some(130)), (5, some(5)), (128, some(128))],
        "130_5_128_full": [(130, range(130)), (5, range(5)), (128, range(128))],
        "64_of_1": [(1, [0] if k % 3 else []) for k in range(64)],
        "64_of_2048": [(2048, some(2048)) for _ in range(64)],
        "plain_in_the_middle": [(130, some(130)), (0, []), (5, range(5)), (0, []), (128, some(128))],
        "empty_entry": [(7, range(7)), (9, []), (7, range(7))],
        "four_subnets": [(128, some(128)), (128, []), (128, range(128)), (128, some(128))],
        "last_position_only": [(3, [2]), (2047, [2046]), (1, [0])],
        "one": [(9, [0, 8])],
    }
    for k in range(40):
        lists["random_%d" % k] = [(n, some(n)) for n in (rnd.choice([0, 1, 3, 8, 13, 64, 130, 2048])
                                                        for _ in range(rnd.randrange(1, 9)))]
    return lists


@pytest.mark.parametrize("kind", KINDS)
def test_concatenation(kind):
    lists = concat_lists()
    got = sim.run_concat(list(lists.values()), kind)
    bad = [name for (name, items), g in zip(lists.items(), got) if g != sim.model_concat(items)]
    assert not bad, bad
    by = dict(zip(lists, got))
    assert by["130_5_128_full"] == (263, b"\xff" * 32 + b"\x7f")
    assert by["64_of_1"][0] == 64 and by["64_of_2048"][0] == 131072 and len(by["64_of_2048"][1]) == 16384
    assert by["empty_entry"] == (23, bytes([0x7F, 0x00, 0x7F]))
    assert by["four_subnets"][0] == 512 and by["four_subnets"][1][16:48] == b"\x00" * 16 + b"\xff" * 16


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
    for method in ("sigpool_open", "verify_accumulate_bits", "verify_accumulate_bits_async", "sigpool_get_bits",
                   "sigpool_sum"):
        assert callable(getattr(native.Context, method)), method
    import inspect
    assert inspect.signature(native.Context.sigpool_open).parameters["n_bits"].default == 0
    from lodestar_amd.verifier import BlsGpuVerifier
    assert callable(BlsGpuVerifier.verify_and_pool_bits_same_message)
