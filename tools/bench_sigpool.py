"""Times bgv_verify_accumulate, bgv_sigpool_get, bgv_sigpool_sum and bgv_verify_accumulate_bits on the
device ("Signature pools" and "Participation bits and entry sums").

    python tools/bench_sigpool.py step|sum|bits [--calls 100] [--warmup 60] [--out FILE]

step   The pool's accumulation step beside the fused call's aggregation step, at 128 and 512
       one-set jobs on one root and 8,192 on 64 roots (one entry / aggregate per root), clean and
       with 1 % wrong signers.  Three variants alternate call by call on the same jobs:
       bgv_verify_spans, bgv_verify_aggregate and bgv_verify_accumulate; median and p25-p75 of the
       host wall time of each (every call ends in a device synchronise), and the two steps as
       differences of the medians from the plain call.  Then bgv_sigpool_get of the touched
       entries, timed on its own.  The entries keep growing over the calls: the accumulator is one
       Jacobian point whatever its count.

sum    bgv_sigpool_sum over 1 x 4, 1 x 64 and 64 x 64 entries of one signature each beside the path
       it replaces on the same entries: bgv_sigpool_get of the ids, then bgv_aggregate_signatures
       over the returned bytes.  The two alternate call by call; the bytes must agree.

bits   bgv_verify_accumulate beside bgv_verify_accumulate_bits on the 128-on-1 and 8,192-on-64
       rows of `step`, every set at a position of its own in a 2,048-position entry, and a third
       variant in which the second half of an entry's sets repeat the positions of the first half
       (known: half as many signatures decoded).  The entries are dropped and opened again before
       every call, outside the timed part, for all variants alike (a position can be taken once).

Every line of output is one JSON record.  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_verify_aggregate import FUSED_SHAPES, Bench, quartiles  # noqa: E402


class PoolBench(Bench):
    def spans(self, s):
        p = s["packed"]
        t = time.perf_counter()
        rc = self.lib.bgv_verify_spans(self.h, p.jobs, s["n"], p.sets, s["n"], None, 0, s["codes"], None)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return 1e3 * dt

    def accumulate(self, s):
        p = s["packed"]
        t = time.perf_counter()
        rc = self.lib.bgv_verify_accumulate(self.h, p.jobs, s["n"], p.sets, s["n"], None, 0, s["tags"], s["codes"],
                                            s["added"], None)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return 1e3 * dt

    def get(self, s):
        na = s["naggs"]
        t = time.perf_counter()
        rc = self.lib.bgv_sigpool_get(self.h, s["ids"], na, s["got"], s["gcnt"], s["gst"])
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return 1e3 * dt


def run_step(args, emit):
    b = PoolBench(8192)
    for n, nroots in FUSED_SHAPES:
        for wrong_every in (0, 100):
            s = b.shape(n, nroots, wrong_every)
            s.update(added=(ctypes.c_uint8 * n)(), ids=(ctypes.c_uint32 * nroots)(*range(nroots)),
                     got=ctypes.create_string_buffer(96 * nroots), gcnt=(ctypes.c_uint32 * nroots)(),
                     gst=(ctypes.c_int32 * nroots)())
            assert b.ctx.sigpool_drop_range(0, b.native.MAX_SIGPOOL) >= 0
            for i in range(nroots):
                b.ctx.sigpool_open(i)
            variants = [lambda: b.spans(s), lambda: b.fused(s), lambda: b.accumulate(s)]
            for _ in range(args.warmup):
                for v in variants:
                    v()
            times = [[], [], []]
            for _ in range(args.calls):
                for k, v in enumerate(variants):
                    times[k].append(v())
            # the codes are the expected ones, every accepted set was added every time, and one
            # more call into fresh entries gives the fused call's bytes
            assert [k for k in range(n) if s["codes"][k] != 1] == sorted(s["wrong"])
            assert [k for k in range(n) if not s["added"][k]] == sorted(s["wrong"])
            calls = args.warmup + args.calls
            b.get(s)
            assert all(v == 0 for v in s["gst"]) and sum(s["gcnt"]) == calls * (n - len(s["wrong"]))
            b.ctx.sigpool_drop_range(0, nroots)
            for i in range(nroots):
                b.ctx.sigpool_open(i)
            b.accumulate(s)
            b.fused(s)
            b.get(s)
            assert s["got"].raw == s["agg"].raw and list(s["gcnt"]) == list(s["cnt"])
            for _ in range(args.warmup):
                b.get(s)
            gets = [b.get(s) for _ in range(args.calls)]
            med = [statistics.median(t) for t in times]
            emit({"part": "step", "jobs": n, "roots": nroots, "wrong_signers": len(s["wrong"]),
                  "verify_spans": quartiles(times[0]), "verify_aggregate": quartiles(times[1]),
                  "verify_accumulate": quartiles(times[2]),
                  "aggregate_step_ms": round(med[1] - med[0], 4), "accumulate_step_ms": round(med[2] - med[0], 4),
                  "sigpool_get": quartiles(gets), "entries": nroots})


def run_sum(args, emit):
    b = PoolBench(4096)
    n = 4096
    s = b.shape(n, 1)
    s["tags"] = (ctypes.c_uint32 * n)(*range(n))
    s["added"] = (ctypes.c_uint8 * n)()
    for i in range(n):
        b.ctx.sigpool_open(i)
    b.accumulate(s)
    assert all(s["added"])
    for ngroups, per in ((1, 4), (1, 64), (64, 64)):
        m = ngroups * per
        ids = (ctypes.c_uint32 * m)(*range(m))
        groups = (b.native.BgvPoolGroup * ngroups)()
        for g in range(ngroups):
            groups[g].ids = ctypes.addressof(ids) + 4 * per * g
            groups[g].n_ids = per
        out = ctypes.create_string_buffer(96 * ngroups)
        cnt, st, nb = (ctypes.c_uint32 * ngroups)(), (ctypes.c_int32 * ngroups)(), (ctypes.c_uint32 * ngroups)()
        got = ctypes.create_string_buffer(96 * m)
        gcnt, gst = (ctypes.c_uint32 * m)(), (ctypes.c_int32 * m)()
        lens = (ctypes.c_uint32 * m)(*([96] * m))
        counts = (ctypes.c_uint32 * ngroups)(*([per] * ngroups))
        out2 = ctypes.create_string_buffer(96 * ngroups)
        st2 = (ctypes.c_int32 * ngroups)()

        def summed():
            t = time.perf_counter()
            rc = b.lib.bgv_sigpool_sum(b.h, groups, ngroups, out, cnt, st, None, 0, nb)
            dt = time.perf_counter() - t
            assert rc == 0, rc
            return 1e3 * dt

        def replaced():
            t = time.perf_counter()
            rc = b.lib.bgv_sigpool_get(b.h, ids, m, got, gcnt, gst)
            rc2 = b.lib.bgv_aggregate_signatures(b.h, got, lens, counts, ngroups, out2, st2)
            dt = time.perf_counter() - t
            assert rc == 0 and rc2 == 0, (rc, rc2)
            return 1e3 * dt

        variants = [summed, replaced]
        for _ in range(args.warmup):
            for v in variants:
                v()
        times = [[], []]
        for _ in range(args.calls):
            for k, v in enumerate(variants):
                times[k].append(v())
        assert out.raw == out2.raw and list(st) == list(st2) == [0] * ngroups and list(cnt) == [per] * ngroups
        emit({"part": "sum", "groups": ngroups, "entries_per_group": per, "sigpool_sum": quartiles(times[0]),
              "get_then_aggregate": quartiles(times[1])})


def run_bits(args, emit):
    b = PoolBench(8192)
    nbits = b.native.SIGPOOL_MAX_BITS
    for n, nroots in ((128, 1), (8192, 64)):
        s = b.shape(n, nroots)
        per = n // nroots
        s["added"] = (ctypes.c_uint8 * n)()
        s["outcome"] = (ctypes.c_uint8 * n)()
        s["tags_bits"] = (ctypes.c_uint32 * n)(*[nroots + k % nroots for k in range(n)])
        own, half = (b.native.BgvPoolBits * n)(), (b.native.BgvPoolBits * n)()
        for k in range(n):
            own[k].n_bits = half[k].n_bits = nbits
            own[k].bit = k // nroots
            half[k].bit = (k // nroots) % (per // 2)

        def reopen():
            b.ctx.sigpool_drop_range(0, 2 * nroots)
            for i in range(nroots):
                b.ctx.sigpool_open(i)
                b.ctx.sigpool_open(nroots + i, nbits)

        def with_bits(members):
            p = s["packed"]
            t = time.perf_counter()
            rc = b.lib.bgv_verify_accumulate_bits(b.h, p.jobs, n, p.sets, n, None, 0, s["tags_bits"], members,
                                                  s["codes"], s["outcome"], None)
            dt = time.perf_counter() - t
            assert rc == 0, rc
            return 1e3 * dt

        variants = [lambda: b.spans(s), lambda: b.accumulate(s), lambda: with_bits(own), lambda: with_bits(half)]
        want = [None, None, [1] * n, [1 if k // nroots < per // 2 else 2 for k in range(n)]]
        times = [[], [], [], []]
        for it in range(args.warmup + args.calls):
            for k, v in enumerate(variants):
                reopen()
                dt = v()
                if it >= args.warmup:
                    times[k].append(dt)
                if want[k] is not None:
                    assert list(s["outcome"]) == want[k]
        assert all(s["added"]) and all(c == 1 for c in s["codes"])
        med = [statistics.median(t) for t in times]
        emit({"part": "bits", "jobs": n, "roots": nroots, "verify_spans": quartiles(times[0]),
              "verify_accumulate": quartiles(times[1]), "verify_accumulate_bits": quartiles(times[2]),
              "verify_accumulate_bits_half_known": quartiles(times[3]),
              "accumulate_step_ms": round(med[1] - med[0], 4), "bits_step_ms": round(med[2] - med[0], 4),
              "bits_half_known_step_ms": round(med[3] - med[0], 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["step", "sum", "bits"])
    ap.add_argument("--calls", type=int, default=100, help="timed calls per variant")
    ap.add_argument("--warmup", type=int, default=60,
                    help="untimed calls of each variant before the window (at least half a second of load "
                         "at the smallest shape, so the window runs at the settled clock)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec, sort_keys=True)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    {"step": run_step, "sum": run_sum, "bits": run_bits}[args.part](args, emit)


if __name__ == "__main__":
    main()
