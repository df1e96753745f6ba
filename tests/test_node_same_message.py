"""verifySignatureSetsSameMessage, verifyAndAggregateSameMessage and canAcceptWork of the Node
layer's BlsGpuVerifier (lodestar_amd/node/; tests/node/same_message.js).  CPU, against a mock addon
installed under the addon's resolved path: two aggregating callers and a plain one in one run get
their own results from one addon.verifyAggregate call, a run with no tagged set still calls
addon.verify, canAcceptWork flips at its bound.  GPU: five signers of one root with one wrong
signer, and the aggregate of the other four against aggregateSignatures of them."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "node", "same_message.js")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu.node")
NODE_API = os.path.join(os.environ.get("NODE_INCLUDE", "/usr/include/node"), "node_api.h")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(NODE_API),
                                reason="node or its headers not in image")


def _run(args, timeout):
    from lodestar_amd import build
    assert build.build_node(verbose=False), "Node headers missing"  # rebuilt when the addon's source is newer
    p = subprocess.run(["node", SCRIPT] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_same_message_against_mock_addon():
    assert _run(["cpu"], 60) == {"cpu": "ok"}


def test_addon_exports_verify_aggregate():
    src = open(os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.c")).read()
    assert '{"verifyAggregate", NULL, js_verify_aggregate' in src and "bgv_verify_aggregate_async(" in src
    dts = open(os.path.join(ROOT, "lodestar_amd", "node", "index.d.ts")).read()
    for name in ("verifySignatureSetsSameMessage", "verifyAndAggregateSameMessage", "canAcceptWork", "maxInflightSigs"):
        assert name in dts, name


@pytest.mark.gpu
def test_same_message_on_the_device():
    out = _run([], 100)
    for k in ("results", "aggregate", "errors", "closed"):
        assert out[k] == "ok", out
