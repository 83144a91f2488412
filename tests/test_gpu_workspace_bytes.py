"""-m gpu: the per-instance workspace of the swarm solve kernels is as large as it was before its layout had one definition.

Handles only, no solve: nmpc_workspace_bytes of every configuration of tests/golden/gen_workspace_bytes.GRID (team sizes 1 .. 10, heading
bounded or free, no / two obstacles, horizons on the steps of the checkpoint slot count, an LDS-resident kernel's stride and the HBM-resident
kernel's, one and three instances) against tests/golden/workspace_bytes.json, which that script recorded on the build before WsLayout.  The
arrays inside the workspace are pinned by the bit-identity of the workspace contents (tools/ab_outputs.py); this pins the total."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_workspace_bytes_as_recorded(built):
    spec = importlib.util.spec_from_file_location("gen_workspace_bytes", os.path.join(GOLD, "gen_workspace_bytes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.PATH) as f:
        want = json.load(f)
    assert sorted(want) == sorted(gen.key(r) for r in gen.GRID) and len(want) == 800
    got = gen.measure()
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, "nmpc_workspace_bytes (got, recorded): %s" % sorted(bad.items())[:8]
