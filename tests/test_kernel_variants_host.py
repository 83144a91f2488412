"""CPU: the table of solve-kernel instantiations (tests/kernel_variants.py) is exactly the set of solve kernels in the built gfx950 code object,
the launch-variant descriptor is declared, exported and bound, and the recipes' inputs are ones on which the oracle agrees with itself."""
import os
import re
import subprocess
from collections import Counter

import pytest

from tests import helpers as Hh
from tests import kernel_variants as KV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built_variants(tmp_path):
    """(kernel, m, thb, flags, threads) of every solve_kernel / solve_lds_kernel / solve_col_kernel symbol of lib/libnmpc_hip.so"""
    got = []
    for name in Hh.kernel_notes(tmp_path):
        m = re.search(r"^_ZN4nmpc16solve_col_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEE", name)
        if m:
            got.append((3,) + tuple(int(g) for g in m.groups()))
            continue
        m = re.search(r"^_ZN4nmpc16solve_lds_kernelILi(\d+)ELi(\d+)ELi(\d+)EEE", name)
        if m:
            got.append((2, int(m.group(1)), int(m.group(2)), 0, int(m.group(3))))
            continue
        m = re.search(r"^_ZN4nmpc12solve_kernelILi(\d+)ELi(\d+)EEE", name)
        if m:
            got.append((1, int(m.group(1)), 0, 0, int(m.group(2))))
            continue
        assert not re.search(r"^_ZN4nmpc\d+solve_\w*kernel", name), "solve kernel with an unknown template signature: " + name
    return got


def test_table_equals_the_solve_kernels_of_the_code_object(built, tmp_path):
    """One table row per instantiation and one instantiation per row: a new instantiation without a row fails here, and so does a row
    whose instantiation is gone.  The counts follow from the instantiation rules stated in tests/kernel_variants.py."""
    got = _built_variants(tmp_path)
    assert len(got) == len(set(got)), [v for v, n in Counter(got).items() if n > 1]
    rows = [r.row for r in KV.TABLE]
    assert len(rows) == len(set(rows)), [v for v, n in Counter(rows).items() if n > 1]
    missing_rows = sorted(set(got) - set(rows))
    missing_symbols = sorted(set(rows) - set(got))
    assert not missing_rows, "instantiations without a table row: %s" % missing_rows
    assert not missing_symbols, "table rows without an instantiation: %s" % missing_symbols
    per_kernel = Counter(v[0] for v in got)
    print("solve-kernel instantiations: column %d, element-per-lane %d, HBM-resident %d" % (per_kernel[3], per_kernel[2], per_kernel[1]))
    assert per_kernel[3] % 4 == 0      # every column variant exists per heading flag and per field flag
    for (k, m, thb, fl, tpb) in got:
        if k == 3:
            assert (k, m, thb ^ 1, fl, tpb) in got and (k, m, thb, fl ^ 4, tpb) in got, (k, m, thb, fl, tpb)


def test_variant_descriptor_declared_exported_and_bound(built):
    import ctypes as C
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc_debug.h")).read()
    assert re.search(r"\bnmpc_debug_variant\s*\(", hdr) and "nmpc_debug_variant_t" in hdr
    assert "nmpc_debug_variant" not in open(os.path.join(ROOT, "include", "nmpc.h")).read()      # a development aid, not product ABI
    assert "nmpc_debug_variant" in nmpc_amd._lib.DEBUG_EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert "nmpc_debug_variant" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    assert len(L.nmpc_debug_variant.argtypes) == 5
    # the struct of the header: five int32 then one int64 (8-aligned)
    V = nmpc_amd._lib.CDebugVariant
    assert [f[0] for f in V._fields_] == ["kernel", "m", "thb", "flags", "threads", "lds_bytes"]
    assert C.sizeof(V) == 32 and V.lds_bytes.offset == 24
    # a null handle or a null result is an argument error without touching a device
    v = V()
    assert L.nmpc_debug_variant(None, 1, 0, 0, C.byref(v)) == -1


def test_recipes_cover_what_the_layouts_move():
    """obstacles on at least one row per team size 1..6 of every kernel that has rows for it, pad_rows both ways for m > 1, field rows with
    S = 1 and with S = N, and every pin explained by the module's rules"""
    for kern in (1, 2, 3):
        rows = [r for r in KV.TABLE if r.row[0] == kern]
        for m in range(1, 7):
            assert any(r.cfg.get("obstacles") for r in rows if r.row[1] == m), (kern, m)
        for m in range(2, 11):
            pads = {r.cfg["pad_rows"] for r in KV.TABLE if r.row[1] == m}
            assert pads == {True, False}, m
    fields = {r.obs_field for r in KV.TABLE if r.row[0] == 3 and r.row[3] & 4}
    assert fields == {1, "N"}
    assert all((r.row[3] & 4 != 0) == bool(r.obs_field) for r in KV.TABLE)
    for r in KV.TABLE:
        k, m, thb, fl, tpb = r.row
        want = 2 if k == 2 else (4 if (k == 3 and tpb == 128 and m <= 3) else 0)
        assert r.pin == want, r.row
        assert (math_isfinite(r.cfg.get("th_max")) == bool(thb)) or k == 1, r.row


def math_isfinite(x):
    import math
    return x is not None and math.isfinite(x)


@pytest.mark.parametrize("r", KV.TABLE, ids=[KV.row_id(r) for r in KV.TABLE])
def test_oracle_holds_its_point_on_the_recipe_inputs(built, r):
    """The inputs of every recipe are screened: the oracle, run a second time with w0 and the goals perturbed at rounding level, converges on
    every instance to the same point (1e-6) in the same number of iterations.  So a GPU instance off the oracle's point is the GPU's doing.
    The solves are short cold starts."""
    conv, hold, iters = KV.screen(r)
    assert conv and hold, (r.row, r.seed, conv, hold)
    assert iters <= 100, (r.row, iters)
