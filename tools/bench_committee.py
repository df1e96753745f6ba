"""Committee-bitfield sets against index sets: the same sets in both forms, one process,
interleaved A/B (not part of bench.py).

    python tools/bench_committee.py [--runs 120] [--calls 1260] [--out profiles/r07/committee_bits.jsonl]

  block import   bench.py's config 3 (randao + 128 x 128-key attestations + the 512-key sync
                 aggregate + proposer, one non-batchable call of 131 sets) at 100 %, 95 % and 50 %
                 participation: one call of the index form, one of the committee form, in turn;
                 p10 / p50 / p90 of the wall latency of each over --runs calls.  The index form's
                 own p10..p90 is the noise floor a difference has to clear.
  config 2       1024 aggregate sets x 128 keys, 126 calls in flight (bench.py
                 aggregate_throughput's stream) at 100 % and 95 % participation: sets/s of each
                 form, the two streams run alternately, three times each.

One JSON line per measurement on stdout and appended to --out.  Every verdict is checked.  The
index path's code is the parent's; the committee path uploads 16 bytes of bits per 128-member set
and gathers the shorter side (bgv_pk_bits.h).
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (interop_sk, R_ORDER, default_batching)

NKEYS = 131072


def pack(positions, n):
    b = bytearray((n + 7) // 8)
    for p in positions:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


def present(j, n, participation):
    """The members of committee j that take part: all but n (100 - p) / 100 scattered ones."""
    absent = {(j * 7 + 13 * q) % n for q in range(n * (100 - participation) // 100)}
    return [p for p in range(n) if p not in absent]


def both_forms(ctx, native, groups, ids, sk_int, participation, tag):
    """groups: [(members, committee id or None)]; returns (index-form sets, committee-form sets)."""
    msgs = [hashlib.sha256(b"bench-committee" + tag + i.to_bytes(4, "little")).digest() for i in range(len(groups))]
    pos = [present(i, len(m), participation) if ids[i] is not None else [0] for i, m in enumerate(groups)]
    sks = [(sum(sk_int[m[p]] for p in pos[i]) % bench.R_ORDER).to_bytes(32, "big") for i, m in enumerate(groups)]
    sigs = ctx.sign(b"".join(sks), b"".join(msgs))
    idx_sets, com_sets = [], []
    for i, m in enumerate(groups):
        sig = sigs[96 * i:96 * i + 96]
        s = native.SetSpec(msgs[i], sig, pk_indices=[m[p] for p in pos[i]])
        idx_sets.append(s)
        com_sets.append(s if ids[i] is None else
                        native.SetSpec(msgs[i], sig, committee=ids[i], bits=pack(pos[i], len(m)), n_bits=len(m)))
    return idx_sets, com_sets


def caller(ctx, native, jobs):
    packed = native.PackedCall(jobs)
    n = len(jobs)

    def call(stats=None):
        out = (native.ctypes.c_int32 * n)()
        st = native.ctypes.byref(stats) if stats is not None else None
        if packed.pkbits is not None:
            rc = ctx.lib.bgv_verify_bits(ctx.handle, packed.jobs, n, packed.sets, packed.nsets, packed.pkbits,
                                         native.MODE_WORKER, out, st)
        else:
            rc = ctx.lib.bgv_verify(ctx.handle, packed.jobs, n, packed.sets, packed.nsets, native.MODE_WORKER, out, st)
        if rc != 0:
            raise native.DeviceError(native.strerror(rc))
        assert list(out) == [1] * n, "verdict mismatch"
    call.keep = packed
    return call


def lone_device_ms(native, call, runs=20):
    """Median HIP-event time of the kernels of one call on an otherwise idle device."""
    ms = []
    for _ in range(runs):
        st = native.BgvStats()
        call(st)
        ms.append(st.device_ms)
    return statistics.median(ms)


def pct(lat):
    s = sorted(lat)
    return {"p10_ms": 1e3 * s[len(s) // 10], "p50_ms": 1e3 * statistics.median(s), "p90_ms": 1e3 * s[9 * len(s) // 10]}


def block_import(ctx, native, sk_int, runs, emit):
    groups = [[0]] + [list(range(128 * a, 128 * a + 128)) for a in range(128)] + [list(range(16384, 16896)), [1]]
    ids = [None] + list(range(128)) + [128, None]
    for i, m in enumerate(groups):
        if ids[i] is not None:
            ctx.committee_put(ids[i], m)
    for p in (100, 95, 50):
        idx_sets, com_sets = both_forms(ctx, native, groups, ids, sk_int, p, b"block%d" % p)
        a, b = caller(ctx, native, [(idx_sets, False)]), caller(ctx, native, [(com_sets, False)])
        for _ in range(5):
            a()
            b()
        la, lb = [], []
        for _ in range(runs):
            for fn, lat in ((a, la), (b, lb)):
                t = time.perf_counter()
                fn()
                lat.append(time.perf_counter() - t)
        npk = sum(len(s.pk_indices) for s in idx_sets)
        bits_bytes = sum(4 * (1 + (len(m) + 31) // 32) for i, m in enumerate(groups) if ids[i] is not None)
        emit({"shape": "block_import", "participation": p, "runs": runs, "pubkeys_in_index_form": npk,
              "index_upload_bytes": 4 * npk, "bits_upload_bytes": bits_bytes,
              "lone_call_device_ms": {"index": lone_device_ms(native, a), "committee": lone_device_ms(native, b)},
              "index": pct(la), "committee": pct(lb)})
    for i in ids:
        if i is not None:
            ctx.committee_drop(i)


def stream(ctx, native, call, nsets, calls, inflight, settle_s=0.6):
    from concurrent.futures import ThreadPoolExecutor
    done, lock = [], threading.Lock()

    def one(_):
        call()
        with lock:
            done.append(time.perf_counter())

    ctx.set_batching(inflight * nsets, 20000, 20000)
    t0 = time.perf_counter()
    try:
        with ThreadPoolExecutor(max_workers=inflight) as pool:
            list(pool.map(one, range(calls)))
    finally:
        ctx.set_batching(*bench.default_batching())
    done.sort()
    b, a = len(done) - 1, 2 * inflight - 1
    while a + inflight < b and done[a] - t0 < settle_s:
        a += inflight
    return nsets * (b - a) / (done[b] - done[a])


def config2(ctx, native, sk_int, calls, emit):
    nsets, per, inflight = 1024, 128, 126
    groups = [list(range(per * a, per * a + per)) for a in range(nsets)]
    ids = list(range(1000, 1000 + nsets))
    for i, m in zip(ids, groups):
        ctx.committee_put(i, m)
    for p in (100, 95):
        idx_sets, com_sets = both_forms(ctx, native, groups, ids, sk_int, p, b"agg%d" % p)
        jobs = lambda sets: [(sets[j:j + 128], True) for j in range(0, nsets, 128)]
        a, b = caller(ctx, native, jobs(idx_sets)), caller(ctx, native, jobs(com_sets))
        a()
        b()
        ra, rb = [], []
        for _ in range(3):
            ra.append(stream(ctx, native, a, nsets, calls, inflight))
            rb.append(stream(ctx, native, b, nsets, calls, inflight))
        emit({"shape": "config2", "participation": p, "calls": calls, "inflight": inflight, "unit": "sets/s",
              "lone_call_device_ms": {"index": lone_device_ms(native, a), "committee": lone_device_ms(native, b)},
              "index": ra, "committee": rb, "index_median": statistics.median(ra),
              "committee_median": statistics.median(rb)})
    for i in ids:
        ctx.committee_drop(i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=120)
    ap.add_argument("--calls", type=int, default=1260)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "committee_bits.jsonl"))
    ap.add_argument("--no-config2", action="store_true")
    args = ap.parse_args()
    from lodestar_amd import native
    ctx = native.Context([0])
    ctx.keygen(b"".join(bench.interop_sk(i) for i in range(NKEYS)), cache_first=0, want_pubkeys=False)
    sk_int = [int.from_bytes(bench.interop_sk(i), "big") for i in range(NKEYS)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    block_import(ctx, native, sk_int, args.runs, emit)
    if not args.no_config2:
        config2(ctx, native, sk_int, args.calls, emit)
    ctx.close()


if __name__ == "__main__":
    main()
