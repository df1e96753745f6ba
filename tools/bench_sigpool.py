"""Times bgv_verify_accumulate and bgv_sigpool_get on the device ("Signature pools").

    python tools/bench_sigpool.py step [--calls 100] [--warmup 60] [--out FILE]

step   The pool's accumulation step beside the fused call's aggregation step, at 128 and 512
       one-set jobs on one root and 8,192 on 64 roots (one entry / aggregate per root), clean and
       with 1 % wrong signers.  Three variants alternate call by call on the same jobs:
       bgv_verify_spans, bgv_verify_aggregate and bgv_verify_accumulate; median and p25-p75 of the
       host wall time of each (every call ends in a device synchronise), and the two steps as
       differences of the medians from the plain call.  Then bgv_sigpool_get of the touched
       entries, timed on its own.  The entries keep growing over the calls: the accumulator is one
       Jacobian point whatever its count.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["step"])
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

    {"step": run_step}[args.part](args, emit)


if __name__ == "__main__":
    main()
