"""Span sets through the Node layer (lodestar_amd/node/): the {type: "committees"} set of
BlsGpuVerifier (one bitfield over several stored committees) and its producer in
signatureSets.js.  CPU: the native set form and the producer against the expanded-index form.
GPU: a valid and an invalid set through BlsGpuVerifier.verifySignatureSets."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "node", "multi_committee.js")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu.node")
NODE_API = os.path.join(os.environ.get("NODE_INCLUDE", "/usr/include/node"), "node_api.h")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(NODE_API),
                                reason="node or its headers not in image")


def _run(args, timeout):
    from lodestar_amd import build
    if not os.path.exists(ADDON):
        assert build.build_node(verbose=False), "Node headers missing"
    p = subprocess.run(["node", SCRIPT] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_committees_set_form_and_producer():
    assert _run(["cpu"], 60) == {"cpu": "ok"}


@pytest.mark.gpu
def test_committees_sets_through_verifier():
    out = _run([], 100)
    for k in ("valid", "invalid", "mixed", "dropped"):
        assert out[k] == "ok", out
