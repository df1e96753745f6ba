"""Filling an epoch's committees: one bgv_shuffling_put against the per-committee path, one
process, interleaved A/B (not part of bench.py).

    python tools/bench_shuffling.py [--runs 20] [--n 1048576] [--out profiles/r08/shuffling.jsonl]

  A  committee_put   the device part of the per-committee path: slots * committees_per_slot
                     (32 * 64 = 2,048) bgv_committee_put calls with member lists shuffled
                     beforehand.  A lower bound of that path: the host's unshuffleList is not in it.
  B  shuffling_put   one bgv_shuffling_put over the same active indices with the shuffling read
                     back (swap-or-not on the device, directory entries, the same pubkey sums).

Both forms go through the C-ABI with arrays prepared beforehand, each run fills the same ids and
is followed by an untimed bgv_committee_drop_range.  The n active indices are drawn from the --keys cached keys: the
entry points take repeated indices, and the pubkey gathers of both forms read the same cache.
One JSON line on stdout and appended to --out: median and p10 / p90 of the wall time of each
form over --runs runs, the same for B with rounds = 0 (no digest table and a walk without rounds:
what is left is the copies, the directory, the 2,048 sums and the host's mirror, so the difference
to B is what the swap-or-not rounds cost).  B's shuffling is checked against a hashlib / numpy
model at full size, and A and B must produce the same aggregates.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (interop_sk)


def pct(lat):
    s = sorted(lat)
    return {"p10_ms": 1e3 * s[len(s) // 10], "p50_ms": 1e3 * statistics.median(s), "p90_ms": 1e3 * s[9 * len(s) // 10],
            "min_ms": 1e3 * s[0]}


def model_shuffle(seed, rounds, active):
    """compute_shuffled_index for every position at once: hashlib digests, numpy for the walk
    (independent of bgv_shuffle.h; checks the device's shuffling at the benchmark's size)."""
    import hashlib

    import numpy as np
    n = len(active)
    idx = np.arange(n, dtype=np.int64)
    for r in range(rounds):
        rb = bytes([r])
        pivot = int.from_bytes(hashlib.sha256(seed + rb).digest()[:8], "little") % n
        src = np.frombuffer(b"".join(hashlib.sha256(seed + rb + b.to_bytes(4, "little")).digest()
                                     for b in range((n + 255) // 256)), dtype=np.uint8)
        flip = (pivot + n - idx) % n
        pos = np.maximum(idx, flip)
        bit = (src[pos >> 3] >> (pos & 7).astype(np.uint8)) & 1
        idx = np.where(bit == 1, flip, idx)
    return np.asarray(active)[idx]


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=131072)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--committees-per-slot", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "shuffling.jsonl"))
    args = ap.parse_args()
    assert args.runs >= 20, "medians of fewer than 20 runs are not reported"
    from lodestar_amd import native
    ctx = native.Context([0])
    ctx.keygen(b"".join(bench.interop_sk(i) for i in range(args.keys)), cache_first=0, want_pubkeys=False)
    lib, h, ct = ctx.lib, ctx.handle, native.ctypes
    n, count = args.n, args.slots * args.committees_per_slot
    active = (np.arange(n, dtype=np.uint64) * 2654435761 % args.keys).astype(np.uint32)
    seed = ct.create_string_buffer(bytes(range(32)), 32)
    out = np.empty(n, dtype=np.uint32)

    def form_b(rounds=args.rounds):
        rc = lib.bgv_shuffling_put(h, 0, seed, active.ctypes.data, n, args.slots, args.committees_per_slot, rounds,
                                   out.ctypes.data)
        assert rc == 0, native.strerror(rc)

    def drop():
        assert lib.bgv_committee_drop_range(h, 0, count) == count

    # the member lists of form A: the shuffling itself, computed once (by form B) and cut as the
    # reference cuts it
    form_b()
    shuffling = out.copy()
    assert np.array_equal(shuffling, model_shuffle(bytes(range(32)), args.rounds, active)), "shuffling differs from the model"
    bounds = [n * k // count for k in range(count + 1)]
    lists = [np.ascontiguousarray(shuffling[bounds[k]:bounds[k + 1]]) for k in range(count)]
    ptrs = [(a.ctypes.data, a.size) for a in lists]
    probe = [0, count // 2, count - 1]
    all_bits = lambda k: (bytes([0xFF]) * ((lists[k].size + 7) // 8 - 1) +
                          bytes([(1 << ((lists[k].size - 1) % 8 + 1)) - 1]), int(lists[k].size))
    agg_b = [ctx.aggregate_committee_bits(k, *all_bits(k)) for k in probe]
    drop()

    def form_a():
        for k, (p, m) in enumerate(ptrs):
            rc = lib.bgv_committee_put(h, k, p, m)
            assert rc == 0, native.strerror(rc)

    form_a()
    agg_a = [ctx.aggregate_committee_bits(k, *all_bits(k)) for k in probe]
    drop()
    assert agg_a == agg_b, "the two forms disagree"
    la, lb, lb0 = [], [], []
    for _ in range(args.runs):
        for fn, lat in ((form_a, la), (lambda: form_b(0), lb0), (form_b, lb)):
            t = time.perf_counter()
            fn()
            lat.append(time.perf_counter() - t)
            drop()
        assert np.array_equal(out, shuffling)
    rec = {"shape": "epoch_fill", "n_active": n, "committees": count, "rounds": args.rounds, "runs": args.runs,
           "keys": args.keys, "shuffling_matches_model": True, "same_aggregates": True, "committee_put_x%d" % count: pct(la), "shuffling_put": pct(lb),
           "shuffling_put_rounds0": pct(lb0)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
