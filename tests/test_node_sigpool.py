"""poolOpen, poolDropRange, poolGet and verifyAndPoolSameMessage of the Node layer's BlsGpuVerifier
(lodestar_amd/node/; tests/node/sigpool.js).  CPU, against a mock addon installed under the addon's
resolved path: a buffered run holds one kind of caller (a pool caller after aggregating callers
starts a new run, and the reverse), a pool caller's sets carry its entry, `added` comes back per
set, a run with neither kind still calls addon.verify.  GPU: two calls into one entry with a wrong
signer and an undecodable signature in the second, poolGet against aggregateSignatures of the
accepted sets; a pool caller and an aggregating caller issued together."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "node", "sigpool.js")
NODE_API = os.path.join(os.environ.get("NODE_INCLUDE", "/usr/include/node"), "node_api.h")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(NODE_API),
                                reason="node or its headers not in image")


def _run(args, timeout):
    from lodestar_amd import build
    assert build.build_node(verbose=False), "Node headers missing"  # rebuilt when the addon's source is newer
    p = subprocess.run(["node", SCRIPT] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_pool_callers_against_mock_addon():
    assert _run(["cpu"], 60) == {"cpu": "ok"}


def test_addon_exports_the_pool():
    src = open(os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.c")).read()
    for name, fn in (("sigpoolOpen", "bgv_sigpool_open("), ("sigpoolDropRange", "bgv_sigpool_drop_range("),
                     ("sigpoolGet", "bgv_sigpool_get("), ("verifyAccumulate", "bgv_verify_accumulate_async(")):
        assert '{"%s", NULL, js_' % name in src and fn in src, name
    dts = open(os.path.join(ROOT, "lodestar_amd", "node", "index.d.ts")).read()
    for name in ("verifyAndPoolSameMessage", "poolOpen", "poolDropRange", "poolGet"):
        assert name in dts, name


@pytest.mark.gpu
def test_pool_on_the_device():
    out = _run([], 100)
    for k in ("pool", "together", "drop", "closed"):
        assert out[k] == "ok", out
