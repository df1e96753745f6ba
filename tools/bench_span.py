"""Span sets (one bitfield over several committees, bgv_verify_spans) against index sets: the
same block-import call in both forms, one process, interleaved A/B (not part of bench.py;
tools/bench_committee.py is the one-committee sibling).

    python tools/bench_span.py [--runs 60] [--members 128,512] [--out profiles/span_sets/span_sets.jsonl]

  block import   randao + 8 attestation sets, each ONE bitfield over 64 committees of --members
                 members (a full slot's aggregate since EIP-7549: 8,192 keys per set at 128 members,
                 32,768 at 512) + the 512-key sync aggregate + proposer: one non-batchable call of
                 11 sets, at 99 %, 95 % and 50 % participation.  One call of the index form, one of
                 the span form, in turn; p10 / p50 / p90 of the wall latency of each over --runs
                 calls.  The index form's own p10..p90 is the noise floor a difference has to clear.

The cache holds 131,072 keys; at 512 members the 8 x 64 committees need 262,144 places, so the
committees of attestations 4..7 repeat the keys of 0..3 (the same work for both forms).
One JSON line per measurement on stdout and appended to --out.  Every verdict is checked.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (interop_sk, R_ORDER)
from tools.bench_committee import NKEYS, lone_device_ms, pack, pct, present  # noqa: E402

NATT, NCOM, SYNC_ID = 8, 64, 15000


def caller(ctx, native, jobs):
    packed = native.PackedCall(jobs)
    n = len(jobs)

    def call(stats=None):
        out = (native.ctypes.c_int32 * n)()
        st = native.ctypes.byref(stats) if stats is not None else None
        if packed.spans is not None:
            rc = ctx.lib.bgv_verify_spans(ctx.handle, packed.jobs, n, packed.sets, packed.nsets, packed.spans,
                                          native.MODE_WORKER, out, st)
        else:
            rc = ctx.lib.bgv_verify(ctx.handle, packed.jobs, n, packed.sets, packed.nsets, native.MODE_WORKER, out, st)
        if rc != 0:
            raise native.DeviceError(native.strerror(rc))
        assert list(out) == [1] * n, "verdict mismatch"
    call.keep = packed
    return call


def block_import(ctx, native, sk_int, members, runs, emit):
    coms = [[[(a * NCOM * members + c * members + i) % NKEYS for i in range(members)] for c in range(NCOM)]
            for a in range(NATT)]
    ids = [[1000 + a * NCOM + c for c in range(NCOM)] for a in range(NATT)]
    for a in range(NATT):
        for c in range(NCOM):
            ctx.committee_put(ids[a][c], coms[a][c])
    sync = list(range(16384, 16896))
    ctx.committee_put(SYNC_ID, sync)
    for p in (99, 95, 50):
        msgs = [hashlib.sha256(b"bench-span%d-%d-%d" % (members, p, i)).digest() for i in range(NATT + 3)]
        per = [[present(a * NCOM + c, members, p) for c in range(NCOM)] for a in range(NATT)]
        att_idx = [[coms[a][c][q] for c in range(NCOM) for q in per[a][c]] for a in range(NATT)]
        sync_pos = present(1, 512, p)
        sks = [sk_int[0]] + [sum(sk_int[v] for v in idx) % bench.R_ORDER for idx in att_idx] + \
              [sum(sk_int[sync[q]] for q in sync_pos) % bench.R_ORDER, sk_int[1]]
        sigs = ctx.sign(b"".join(s.to_bytes(32, "big") for s in sks), b"".join(msgs))
        sg = lambda j: sigs[96 * j:96 * j + 96]  # noqa: E731
        first, last = native.SetSpec(msgs[0], sg(0), pk_indices=[0]), native.SetSpec(msgs[-1], sg(NATT + 2), pk_indices=[1])
        idx_sets = [first] + [native.SetSpec(msgs[1 + a], sg(1 + a), pk_indices=att_idx[a]) for a in range(NATT)] + \
                   [native.SetSpec(msgs[NATT + 1], sg(NATT + 1), pk_indices=[sync[q] for q in sync_pos]), last]
        span_sets = [first]
        for a in range(NATT):
            pos = [c * members + q for c in range(NCOM) for q in per[a][c]]
            span_sets.append(native.SetSpec(msgs[1 + a], sg(1 + a), committees=ids[a],
                                            bits=pack(pos, NCOM * members), n_bits=NCOM * members))
        span_sets += [native.SetSpec(msgs[NATT + 1], sg(NATT + 1), committee=SYNC_ID, bits=pack(sync_pos, 512),
                                     n_bits=512), last]
        fa, fb = caller(ctx, native, [(idx_sets, False)]), caller(ctx, native, [(span_sets, False)])
        for _ in range(5):
            fa()
            fb()
        la, lb = [], []
        for _ in range(runs):
            for fn, lat in ((fa, la), (fb, lb)):
                t = time.perf_counter()
                fn()
                lat.append(time.perf_counter() - t)
        npk = sum(len(s.pk_indices) for s in idx_sets)
        # per committee the shorter side, plus its total on the complement side (bgv_pk_bits.h)
        terms = [sum(min(len(q), members - len(q) + 1) for q in per[a]) for a in range(NATT)]
        emit({"shape": "block_import_spans", "members": members, "committees_per_set": NCOM, "participation": p,
              "runs": runs, "pubkeys_in_index_form": npk, "index_upload_bytes": 4 * npk,
              "span_bits_bytes": NATT * NCOM * members // 8 + 64, "span_terms_per_set": terms,
              "lone_call_device_ms": {"index": lone_device_ms(native, fa), "span": lone_device_ms(native, fb)},
              "index": pct(la), "span": pct(lb)})
    ctx.committee_drop_range(1000, NATT * NCOM)
    ctx.committee_drop(SYNC_ID)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=60)
    ap.add_argument("--members", default="128,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "span_sets", "span_sets.jsonl"))
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

    for m in args.members.split(","):
        block_import(ctx, native, sk_int, int(m), args.runs, emit)
    ctx.close()


if __name__ == "__main__":
    main()
