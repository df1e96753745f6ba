"""An epoch's proposers and the next sync committee on the device (not part of bench.py).

    python tools/bench_sampling.py [--runs 20] [--n 1048576] [--rules phase0,electra]
                                   [--out profiles/r10/sampling.jsonl]

Mainnet numbers: 32 slot seeds, a committee of 512, 90 rounds, over --n active indices drawn from
the --keys cached keys.  Under the byte rule (`phase0`: bgv_proposers, bgv_sync_committee_put,
max_incr --max-incr = 32) two balance profiles: `full` (32 everywhere: every candidate is accepted)
and `half` (16 everywhere: a candidate is accepted on a random byte below 128, about half of
them).  Under the 16-bit rule (`electra`: bgv_proposers_electra, bgv_sync_committee_put_electra,
max_incr --max-incr-electra = 2048) `full` (2048 everywhere) and `min` (32 everywhere, the mainnet
shape of a set without consolidations: a candidate is accepted about once in 64).  One JSON line
per rule and profile on stdout and appended to --out:

  proposers           median and p10 / p90 of the wall time of one bgv_proposers over the 32 seeds
  sync_committee_put  the same for one bgv_sync_committee_put (indices and aggregate read back),
                      each run followed by an untimed bgv_committee_drop
  sim_*_ms            tests/native/samplesim.cpp built -O2 on the same inputs: the same windowed
                      algorithm in C++ on one core (its pass loop alone, input parsing not counted).
                      It is NOT Lodestar's time, and like the device it evaluates whole windows: a
                      sequential loop that stops at the first acceptance hashes `serial_digests`
                      digests where the windows hash `window_digests`.

Both results are checked against the hashlib model of tests/samplesim.py (byte rule) or
tests/samplesim_electra.py (16-bit rule) at the benchmark's size.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (interop_sk)
from tests import samplesim as M8  # noqa: E402  (the byte rule's model and simulator driver)
from tests import samplesim_electra as M16  # noqa: E402  (the 16-bit rule's)


def pct(lat):
    s = sorted(lat)
    return {"p10_ms": 1e3 * s[len(s) // 10], "p50_ms": 1e3 * statistics.median(s), "p90_ms": 1e3 * s[9 * len(s) // 10],
            "min_ms": 1e3 * s[0]}


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=131072)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=90)
    ap.add_argument("--max-incr", type=int, default=32)
    ap.add_argument("--max-incr-electra", type=int, default=2048)
    ap.add_argument("--rules", default="phase0,electra", help="comma-separated: phase0, electra")
    ap.add_argument("--no-sim", action="store_true", help="skip the CPU simulator's figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "sampling.jsonl"))
    args = ap.parse_args()
    assert args.runs >= 20, "medians of fewer than 20 runs are not reported"
    from lodestar_amd import native
    ctx = native.Context([0])
    ctx.keygen(b"".join(bench.interop_sk(i) for i in range(args.keys)), cache_first=0, want_pubkeys=False)
    lib, h, ct = ctx.lib, ctx.handle, native.ctypes
    n = args.n
    active = (np.arange(n, dtype=np.uint64) * 2654435761 % args.keys).astype(np.uint32)
    act_list = [int(v) for v in active]
    epoch_seed = hashlib.sha256(b"lodestar-amd sampling bench").digest()
    seeds = M8.slot_seeds(epoch_seed, args.slots)
    seeds_buf = ct.create_string_buffer(b"".join(seeds), 32 * args.slots)
    seed_buf = ct.create_string_buffer(epoch_seed, 32)
    out_p = np.empty(args.slots, dtype=np.uint32)
    out_i = np.empty(args.size, dtype=np.uint32)
    agg = ct.create_string_buffer(48)
    digests = 2 * args.rounds + 1  # per candidate: a pivot and a block digest per round, one digest of draws
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    # rule -> (model module, numpy type of the table, max_incr, the two C-ABI calls, per-digest candidates, profiles)
    rules = {
        "phase0": (M8, np.uint8, args.max_incr, lib.bgv_proposers, lib.bgv_sync_committee_put, 32,
                   (("full", args.max_incr), ("half", args.max_incr // 2))),
        "electra": (M16, np.uint16, args.max_incr_electra, lib.bgv_proposers_electra,
                    lib.bgv_sync_committee_put_electra, 16,
                    (("full", args.max_incr_electra), ("min", args.max_incr_electra // 64))),
    }
    for rule in args.rules.split(","):
        M, dtype, max_incr, c_proposers, c_sync_put, per_digest, profiles = rules[rule]
        for name, incr in profiles:
            eff = np.full(args.keys, incr, dtype=dtype)
            eff_m = eff.tobytes() if rule == "phase0" else eff.tolist()  # what the rule's model and simulator take

            def proposers():
                rc = c_proposers(h, seeds_buf, args.slots, active.ctypes.data, n, eff.ctypes.data, eff.size, max_incr,
                                 args.rounds, out_p.ctypes.data)
                assert rc == 0, native.strerror(rc)

            def sync_put():
                rc = c_sync_put(h, 0, seed_buf, active.ctypes.data, n, eff.ctypes.data, eff.size, max_incr, args.size,
                                args.rounds, out_i.ctypes.data, agg)
                assert rc == 0, native.strerror(rc)

            want_p = [M.proposer(s, act_list, eff_m, max_incr, args.rounds) for s in seeds]
            want_s, tries_s = M.sync_committee(epoch_seed, act_list, eff_m, args.size, max_incr, args.rounds)
            proposers()
            assert [int(v) for v in out_p] == [v for v, _ in want_p], "proposers differ from the model"
            sync_put()
            assert [int(v) for v in out_i] == want_s, "sync committee differs from the model"
            ctx.committee_drop(0)
            lp, ls = [], []
            for _ in range(args.runs):
                t = time.perf_counter()
                proposers()
                lp.append(time.perf_counter() - t)
                t = time.perf_counter()
                sync_put()
                ls.append(time.perf_counter() - t)
                ctx.committee_drop(0)
            rec = {"shape": "sampling", "rule": rule, "profile": name, "eff_incr": incr, "n_active": n,
                   "slots": args.slots, "size": args.size, "rounds": args.rounds, "max_incr": max_incr,
                   "runs": args.runs, "keys": args.keys, "matches_model": True, "proposers": pct(lp),
                   "sync_committee_put": pct(ls), "proposer_candidates": sum(t for _, t in want_p),
                   "sync_candidates": tries_s, "proposers_serial_digests": digests * sum(t for _, t in want_p),
                   "sync_serial_digests": digests * tries_s}
            if not args.no_sim:
                sp = M.sim_sample(seeds, act_list, eff_m, 1, True, max_incr, args.rounds)
                ss = M.sim_sample([epoch_seed], act_list, eff_m, args.size, False, max_incr, args.rounds)
                assert [(p[0] if hv else None) for hv, _, p in sp["seeds"]] == [v for v, _ in want_p]
                assert ss["seeds"][0][2] == want_s

                def window_digests(passes):
                    return sum(w * k // 256 * args.rounds + w * k * args.rounds + w * k // per_digest
                               for w, _, k in passes)

                rec.update({"sim_proposers_ms": sp["us"] / 1e3, "sim_sync_ms": ss["us"] / 1e3,
                            "sim_what": "the same windowed algorithm in C++ (-O2) on one core; not Lodestar's time",
                            "proposers_passes": sp["passes"], "sync_passes": ss["passes"],
                            "proposers_window_digests": window_digests(sp["passes"]),
                            "sync_window_digests": window_digests(ss["passes"])})
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
