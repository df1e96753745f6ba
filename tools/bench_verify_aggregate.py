"""Times bgv_verify_aggregate on the device ("Verify and aggregate").

    python tools/bench_verify_aggregate.py fused [--calls 100] [--warmup 60] [--out FILE]
    python tools/bench_verify_aggregate.py crossover [--calls 100] [--warmup 60] [--out FILE]

fused      The fused call against the sequence it replaces, bgv_verify then
           bgv_aggregate_signatures over the accepted sets, at 128 and 512 one-set jobs on one root
           and 8,192 on 64 roots (one aggregate per root), clean and with 1 % wrong signers.  The
           two variants alternate call by call; median and p25-p75 of the host wall time of each
           (every call ends in a device synchronise).  The sequence's second call reads buffers
           packed before the timed window (the accepted sets are the same every time), which a
           real caller would have to gather after the verdicts: the comparison leans towards the
           sequence.
crossover  The two decoding forms of the aggregation step at 1 .. 4,096 accepted signatures.  The
           form is fixed per process (BGV_SIGAGG_WAVE_MAX in the environment), so each form runs in
           child processes of its own, alternating; inside a process the fused call alternates with
           the plain verify call of the same jobs, and the step's time is the difference of the
           two medians.

Every line of output is one JSON record.  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROSS_SIZES = [1, 16, 64, 128, 256, 512, 1024, 2048, 4096]
FUSED_SHAPES = [(128, 1), (512, 1), (8192, 64)]


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": round(statistics.median(xs), 4), "p25_ms": round(q[0], 4), "p75_ms": round(q[2], 4),
            "calls": len(xs)}


class Bench:
    def __init__(self, nkeys):
        from lodestar_amd import native
        self.native = native
        self.ctx = native.Context()
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        # any nonzero scalars below r serve as secret keys
        self.sks = [int.from_bytes(hashlib.sha256(b"bench sk %d" % k).digest(), "big") >> 2 for k in range(nkeys)]
        self.skb = [int(s).to_bytes(32, "big") for s in self.sks]
        self.ctx.keygen(b"".join(self.skb), cache_first=0, want_pubkeys=False)

    def shape(self, n, nroots, wrong_every=0):
        """n one-set batchable jobs, job k by key k over root k % nroots with aggregate k % nroots;
        every wrong_every-th signature is another key's over the same root."""
        native = self.native
        roots = [hashlib.sha256(b"bench root %d" % r).digest() for r in range(nroots)]
        msgs = b"".join(roots[k % nroots] for k in range(n))
        raw = self.ctx.sign(b"".join(self.skb[:n]), msgs)
        sigs = [raw[96 * k:96 * k + 96] for k in range(n)]
        wrong = set(range(wrong_every // 2, n, wrong_every)) if wrong_every else set()
        used = [sigs[(k + nroots) % n] if k in wrong else sigs[k] for k in range(n)]
        packed = native.PackedCall([([native.SetSpec(roots[k % nroots], used[k], pk_indices=[k])], True)
                                    for k in range(n)])
        return {"n": n, "naggs": nroots, "packed": packed, "sigs": used, "wrong": wrong,
                "tags": (ctypes.c_uint32 * n)(*[k % nroots for k in range(n)]),
                "codes": (ctypes.c_int32 * n)(), "agg": ctypes.create_string_buffer(96 * nroots),
                "ast": (ctypes.c_int32 * nroots)(), "cnt": (ctypes.c_uint32 * nroots)()}

    def verify(self, s):
        p = s["packed"]
        t = time.perf_counter()
        rc = self.lib.bgv_verify(self.h, p.jobs, s["n"], p.sets, s["n"], 0, s["codes"], None)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return 1e3 * dt

    def fused(self, s):
        p = s["packed"]
        t = time.perf_counter()
        rc = self.lib.bgv_verify_aggregate(self.h, p.jobs, s["n"], p.sets, s["n"], None, 0, s["tags"], s["naggs"],
                                           s["codes"], s["agg"], s["ast"], s["cnt"], None)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return 1e3 * dt

    def pack_sequence(self, s):
        """The second call of the sequence, packed once: the accepted signatures by aggregate."""
        n, na = s["n"], s["naggs"]
        by = [[s["sigs"][k] for k in range(n) if k % na == a and k not in s["wrong"]] for a in range(na)]
        flat = [x for g in by for x in g]
        s["seq"] = (ctypes.create_string_buffer(b"".join(flat), 96 * len(flat)),
                    (ctypes.c_uint32 * len(flat))(*[96] * len(flat)), (ctypes.c_uint32 * na)(*[len(g) for g in by]),
                    ctypes.create_string_buffer(96 * na), (ctypes.c_int32 * na)())

    def sequence(self, s):
        p = s["packed"]
        sigs, lens, counts, out, st = s["seq"]
        t = time.perf_counter()
        rc = self.lib.bgv_verify(self.h, p.jobs, s["n"], p.sets, s["n"], 0, s["codes"], None)
        rc2 = self.lib.bgv_aggregate_signatures(self.h, sigs, lens, counts, s["naggs"], out, st)
        dt = time.perf_counter() - t
        assert rc == 0 and rc2 == 0, (rc, rc2)
        return 1e3 * dt, out.raw


def alternate(calls, warmup, a, b):
    for _ in range(warmup):
        a(), b()
    ta, tb = [], []
    for _ in range(calls):
        ta.append(a())
        tb.append(b())
    return ta, tb


def run_fused(args, emit):
    b = Bench(8192)
    for n, nroots in FUSED_SHAPES:
        for wrong_every in (0, 100):
            s = b.shape(n, nroots, wrong_every)
            b.pack_sequence(s)
            fused, seq = alternate(args.calls, args.warmup, lambda: b.fused(s), lambda: b.sequence(s)[0])
            # the two ways give the same bytes, and the codes are the expected ones
            assert b.sequence(s)[1] == s["agg"].raw and all(v == 0 for v in s["ast"])
            assert [k for k in range(n) if s["codes"][k] != 1] == sorted(s["wrong"])
            emit({"part": "fused", "jobs": n, "roots": nroots, "wrong_signers": len(s["wrong"]),
                  "fused": quartiles(fused), "sequence": quartiles(seq)})


def run_cross_child(args, emit):
    b = Bench(max(CROSS_SIZES))
    for n in CROSS_SIZES:
        s = b.shape(n, 1)
        fused, plain = alternate(args.calls, args.warmup, lambda: b.fused(s), lambda: b.verify(s))
        assert s["cnt"][0] == n and s["ast"][0] == 0
        emit({"part": "crossover", "form": args.form, "accepted": n, "fused": quartiles(fused),
              "verify": quartiles(plain),
              "step_ms": round(statistics.median(fused) - statistics.median(plain), 4)})


def run_cross(args, emit):
    for rep in range(2):
        for form, wave_max in (("wave", 1 << 30), ("lane", 0)):
            env = dict(os.environ, BGV_SIGAGG_WAVE_MAX=str(wave_max))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "crossover-child", "--form", form,
                                  "--calls", str(args.calls), "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=500)
            if out.returncode != 0:
                raise SystemExit("child (%s) exit %d: %s" % (form, out.returncode, out.stderr[-2000:]))
            for line in out.stdout.splitlines():
                emit(dict(json.loads(line), rep=rep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["fused", "crossover", "crossover-child"])
    ap.add_argument("--calls", type=int, default=100, help="timed calls per variant")
    ap.add_argument("--warmup", type=int, default=60,
                    help="untimed calls of each variant before the window (at least half a second of load "
                         "at the smallest shape, so the window runs at the settled clock)")
    ap.add_argument("--form", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec, sort_keys=True)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    {"fused": run_fused, "crossover": run_cross, "crossover-child": run_cross_child}[args.part](args, emit)


if __name__ == "__main__":
    main()
