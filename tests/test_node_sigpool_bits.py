"""poolOpen(id, {nBits}), verifyAndPoolBitsSameMessage, poolGetBits and poolSum of the Node layer's
BlsGpuVerifier (lodestar_amd/node/; tests/node/sigpool_bits.js).  CPU, against a mock addon
installed under the addon's resolved path: a bits caller's sets carry the entry, its size and their
position or field, outcomes come back per set beside the verdict, a buffered run holds one kind of
caller, poolSum flattens its groups; and the addon exports the new surface.  GPU: a duplicate within
one call and one across calls, poolGetBits, and poolSum of four 128-position entries, one of them
empty, against aggregateSignatures over the same signatures and the 512-position field."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "node", "sigpool_bits.js")
NODE_API = os.path.join(os.environ.get("NODE_INCLUDE", "/usr/include/node"), "node_api.h")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(NODE_API),
                                reason="node or its headers not in image")


def _run(args, timeout):
    from lodestar_amd import build
    assert build.build_node(verbose=False), "Node headers missing"  # rebuilt when the addon's source is newer
    p = subprocess.run(["node", SCRIPT] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_bits_callers_against_mock_addon():
    assert _run(["cpu"], 60) == {"cpu": "ok"}


def test_addon_exports_the_new_surface():
    src = open(os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.c")).read()
    for name, fn in (("sigpoolOpenBits", "bgv_sigpool_open_bits("), ("sigpoolGetBits", "bgv_sigpool_get_bits("),
                     ("sigpoolSum", "bgv_sigpool_sum("), ("verifyAccumulateBits", "bgv_verify_accumulate_bits_async(")):
        assert '{"%s", NULL, js_' % name in src and fn in src, name
    from lodestar_amd import build
    assert build.build_node(verbose=False), "Node headers missing"
    p = subprocess.run(["node", "-e", "const a = require('./lodestar_amd/node/blsgpu.node'); console.log(JSON.stringify("
                        "['sigpoolOpenBits', 'sigpoolGetBits', 'sigpoolSum', 'verifyAccumulateBits'].map((k) => typeof a[k])))"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and json.loads(p.stdout) == ["function"] * 4, p.stdout + p.stderr
    dts = open(os.path.join(ROOT, "lodestar_amd", "node", "index.d.ts")).read()
    for name in ("verifyAndPoolBitsSameMessage", "poolGetBits", "poolSum", "PoolRecord", "nBits"):
        assert name in dts, name


@pytest.mark.gpu
def test_pool_bits_on_the_device():
    out = _run([], 100)
    for k in ("bits", "sum", "closed"):
        assert out[k] == "ok", out
