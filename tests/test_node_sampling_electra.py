"""Device-side balance-weighted sampling under Electra's rule through the Node layer
(lodestar_amd/node/): the addon's proposersElectra / syncCommitteePutElectra (napi_async_work) and
BlsGpuVerifier's computeProposers / syncCommitteePut with opts.rule = "electra".  CPU: the exports.
GPU: computeProposers on the `min` table over 257 indices equals a restatement of the spec's loop
written in the script with crypto, a Uint8Array table gives what its widened Uint16Array gives, and
a {type: "committee"} set on the sampled sync committee verifies while one with a cleared bit does
not."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "node", "sampling_electra.js")
NODE_API = os.path.join(os.environ.get("NODE_INCLUDE", "/usr/include/node"), "node_api.h")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(NODE_API),
                                reason="node or its headers not in image")


def _run(args, timeout):
    from lodestar_amd import build
    assert build.build_node(verbose=False), "Node headers missing"
    p = subprocess.run(["node", SCRIPT] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_addon_exports():
    assert _run(["cpu"], 60) == {"cpu": "ok"}


@pytest.mark.gpu
def test_sampling_through_verifier():
    out = _run([], 100)
    for k in ("proposers", "widened", "aggregate", "valid", "invalid", "rejects"):
        assert out[k] == "ok", out
