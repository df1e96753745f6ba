"""bench.main() on the host, over a stub device context (no GPU, no kernels: the plumbing only).

The stub's bgv_verify answers every call with the expected verdicts, so main() runs to its JSON
line.  Checked: --steps N times exactly N calls, whatever the completion period; a plain run calls
none of the --full legs; --full calls each of them (stubbed: their own tests and the GPU run
them for real); --dump-outputs writes the last timed call's verdict codes as float32.
"""
import json
import random
import sys

import numpy as np
import pytest

import bench
from lodestar_amd import native

LEGS = ("roofline_isolated", "block_import_latency", "aggregate_throughput", "mainnet_shaped_throughput",
        "epoch_sweep", "node_shape", "cpu_baseline")
FULL_KEYS = ("roofline", "block_import", "aggregates_1024x128", "mainnet_shaped_roots", "epoch_sweep",
             "node_single_process", "cpu_baseline", "vs_host_pool")
LEG_RESULT = {"roofline_isolated": {"sets": bench.ROOF_SETS, "kernel_ms": {"k_prep": 12.0, "k_miller": 10.0}},
              "cpu_baseline": {"host_pool": {"value": 1.0, "cores": 1}}}


@pytest.fixture
def stub(monkeypatch):
    """Context stub, the legs replaced by recorders; returns (calls of bgv_verify, legs called)."""
    seen = {"verify": 0, "legs": [], "expect": None}
    real_batch = bench.make_gossip_batch

    def make_batch(*a, **k):
        jobs, expect, key_of = real_batch(*a, **k)
        seen["expect"] = expect
        return jobs, expect, key_of

    class Lib:
        def bgv_verify(self, handle, jobs, n, sets, nsets, mode, out, st):
            seen["verify"] += 1
            for i, v in enumerate(seen["expect"]):
                out[i] = v
            return 0

    class Context:
        def __init__(self, devices):
            self.lib, self.handle = Lib(), None

        def keygen(self, sks, cache_first=0, want_pubkeys=False):
            pass

        def sign(self, sks, msgs):
            return bytes(96 * (len(msgs) // 32))

        def set_batching(self, *a):
            pass

        def profile(self, on):
            return {"k_prep": 1.0, "k_miller": 2.0, "k_final": 0.5}, 1

        def close(self):
            pass

    monkeypatch.setattr(native, "Context", Context)
    monkeypatch.setattr(bench, "make_gossip_batch", make_batch)
    for leg in LEGS:
        monkeypatch.setattr(bench, leg, lambda *a, _leg=leg, **k: (seen["legs"].append(_leg),
                                                                  LEG_RESULT.get(_leg, {"value": 1.0}))[1])
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BGV_BENCH_DEVICE", "BGV_DISPATCHERS", "BGV_MAX_BATCH_SLOTS"):
        monkeypatch.delenv(var, raising=False)
    return seen


def run_main(monkeypatch, capsys, *args):
    # 256-set calls, 4 calls per super-batch: a completion period of 8 calls with 2 dispatchers
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--nsets", "256", "--calls-per-batch", "4",
                                      "--settle-s", "0"] + list(args))
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.parametrize("steps,warmup", [(1, 0), (5, 3), (8, 4), (21, 5)])
def test_steps_sets_the_number_of_timed_calls(stub, monkeypatch, capsys, steps, warmup):
    line = run_main(monkeypatch, capsys, "--steps", str(steps), "--warmup", str(warmup))
    assert line["steps"] == steps and line["timed_steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same window of `steps` 256-set calls
    assert line["value"] == pytest.approx(256 * 1e3 / line["ms_per_step"], rel=1e-9)
    # 3 single calls, the warmup rounded up to whole 4-call super-batches, the steps, and at most
    # the calls in flight (max(--inflight 32, 3 x 4)) draining after the window
    warm = -(-warmup // 4) * 4
    assert 3 + warm + steps <= stub["verify"] <= 3 + warm + steps + 32


def test_plain_run_skips_every_full_leg(stub, monkeypatch, capsys):
    line = run_main(monkeypatch, capsys, "--steps", "8", "--warmup", "4")
    assert stub["legs"] == []
    assert not [k for k in FULL_KEYS if k in line]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["unit"] == "sets/s" and line["higher_is_better"] is True


def test_full_runs_every_leg(stub, monkeypatch, capsys):
    line = run_main(monkeypatch, capsys, "--steps", "8", "--warmup", "4", "--full", "--node-shape", "on")
    assert sorted(stub["legs"]) == sorted(LEGS)
    assert not [k for k in FULL_KEYS if k not in line]
    assert line["roofline"]["kernel"] == "k_prep" and line["roofline"]["sets_per_launch"] == bench.ROOF_SETS


def test_full_options_select_among_the_legs(stub, monkeypatch, capsys):
    line = run_main(monkeypatch, capsys, "--steps", "8", "--warmup", "4", "--full", "--no-cpu-baseline",
                    "--no-block-import", "--no-epoch-sweep")
    assert stub["legs"] == ["roofline_isolated"]
    assert "roofline" in line and "cpu_baseline" not in line and "epoch_sweep" not in line


def test_dump_outputs_writes_the_last_verdicts(stub, monkeypatch, capsys, tmp_path):
    out = tmp_path / "dump"
    run_main(monkeypatch, capsys, "--steps", "8", "--warmup", "4", "--dump-outputs", str(out))
    assert [p.name for p in out.iterdir()] == ["verdicts.npy"]
    got = np.load(out / "verdicts.npy")
    assert got.dtype == np.float32 and got.shape == (256,)
    # make_gossip_batch: round(256 x 0.01) = 3 corrupted jobs at seeded positions: a wrong message
    # and a wrong key (false), a flipped compression flag (bad encoding, -1)
    want = np.ones(256, dtype=np.float32)
    bad = random.Random(0x8192).sample(range(256), 3)
    want[bad[0]], want[bad[1]], want[bad[2]] = 0, 0, -1
    assert (got == want).all()
