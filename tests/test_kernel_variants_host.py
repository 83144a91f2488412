"""CPU: the table of solve-kernel instantiations (tests/kernel_variants.py) is exactly the set of solve kernels in the built gfx950 code object,
the launch-variant descriptor is declared, exported and bound, the library's choice of kernel, shape and instantiation (pure host arithmetic,
reached through the device-free descriptor with the 256 compute units of an MI355X) is what the table, the pinning tests and the built code
object say, and the recipes' inputs are ones on which the oracle agrees with itself."""
import json
import os
import re
import subprocess
from collections import Counter

import pytest

from oracle import nlp_ref as R
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


CUS = 256      # compute units of an MI355X


def test_every_row_is_named_by_its_recipe(built):
    """the device-free descriptor names each row of the table for the row's own recipe (pin, B, ordered, field), with exactly the LDS bytes
    recorded for the row in tests/golden/col_lds_bytes.json (the same call on the build before the LDS layout had one definition)"""
    with open(os.path.join(ROOT, "tests", "golden", "col_lds_bytes.json")) as f:
        lds_bytes = json.load(f)
    assert sorted(lds_bytes) == sorted(KV.row_id(r) for r in KV.TABLE)
    for r in KV.TABLE:
        rc, got, lds, code = KV.variant_of_config(KV.c_config(R.NLPConfig(**r.cfg), r.max_iter), r.pin, CUS, r.B, r.ordered, r.obs_field)
        assert rc == 0 and got == r.row and 0 <= lds <= 160 * 1024, (r.row, rc, got, lds)
        assert lds == lds_bytes[KV.row_id(r)], (r.row, lds, lds_bytes[KV.row_id(r)])
        assert code == (4 if (got[0] == 3 and got[4] > 64) else got[0]), (r.row, code)


def test_own_choice_never_launches_the_element_kernel_host(built):
    """The grid and the assertions of tests/test_gpu_kernel_variants.py::test_own_choice_never_launches_the_element_kernel, without a handle:
    for five to ten robots, both heading flags, 0 / 1 / 2 / 8 obstacles and every horizon up to the first one of the HBM-resident kernel, the
    unpinned library launches the column kernel (B = 1 satisfies every batch condition of the plan), then kernel 1."""
    seen = set()
    for m in range(5, 11):
        for thb in (0, 1):
            for K in (0, 1, 2, 8):
                d = KV._cfg(m, 2, thb, 2 if K else 0, True)
                if K:
                    d["obstacles"] = [(0.0, 0.0, 0.1)] * K
                for N in range(2, KV.KERNEL1[m] + 1):
                    d["N"] = N
                    rc, got, _, _ = KV.variant_of_config(KV.c_config(R.NLPConfig(**d), 10), 0, CUS, 1, 0, 0)
                    assert rc == 0 and got[0] in (1, 3), (m, thb, K, N, rc, got)
                    assert (got[0] == 1) == (N >= KV.KERNEL1[m]), (m, thb, K, N, got)
                    seen.add(got)
    assert {v[0] for v in seen} == {1, 3}


def test_kernel_selection_by_team_size_and_batch_host(built):
    """the literal expectations of tests/test_gpu_pinning.py::test_kernel_selection_by_team_size_and_batch (kernel codes as nmpc_query answers
    them), without a handle"""
    def choice(ocfg, B, kernel=0, ordered=False):
        cc = KV.c_config(ocfg, 2000)
        return [KV.variant_of_config(cc, kernel, CUS, b, ordered, 0)[3] for b in B]
    assert choice(R.cfg_two(20), [1, 512, 4096]) == [3, 3, 3]
    assert choice(R.cfg_six(20), [1, 512, 2048, 2049, 4096]) == [4, 4, 4, 3, 3]
    assert choice(R.cfg_ten(20), [256, 1024, 1025, 4096]) == [4, 4, 3, 3]
    c8 = R.cfg_six(25); c8.obstacles = [(0.3 * i, 0.0, 0.1) for i in range(8)]; c8.rob_dim = 0.2; c8.margin = 0.1
    assert choice(c8, [1024, 1025]) == [4, 3]                # eight obstacles: 63 KB of LDS per instance with its duals, 512 at once
    assert choice(R.cfg_six(20), [1, 4096], kernel=3) == [3, 3] and choice(R.cfg_six(20), [1, 4096], kernel=2) == [2, 2]
    assert choice(R.cfg_six(20), [1, 4096], kernel=4) == [4, 4]
    assert choice(R.cfg_six(20), [2048, 4096, 4097], ordered=True) == [4, 4, 3]      # with an order hint: up to four rounds
    assert choice(R.cfg_six(120), [1, 64]) == [3, 3]
    assert choice(R.cfg_six(240), [1, 64]) == [1, 1]          # beyond the LDS of either LDS kernel: HBM-resident fallback


# Batch sizes at and one above every threshold of the plan on 256 compute units: 256 and 512 (the element-per-lane kernel's shapes and its
# branches of the plan), two and four rounds of the latency shape's slots (256 x 1..4 instances) and two rounds of its four-wavefront slots
# (256 x 1..2): 512, 1024, 1536, 2048 and 1024, 2048, 3072, 4096; and the smallest batches
SWEEP_B = [0, 1] + [b for t in (256, 512, 1024, 1536, 2048, 3072, 4096) for b in (t, t + 1)]
SWEEP_N = [2, 3, 5, 8, 12, 16, 20, 24, 32, 48, 64, 96, 128, 192, 256, 512, 1024, 1200, 4096]      # coarse, to past the kernel-1 boundary of every team size


def test_every_plan_names_a_built_instantiation(built, tmp_path):
    """Over team sizes, heading flags, obstacle counts, pins, horizons (SWEEP_N plus the three around each team size's kernel-1 boundary),
    batch sizes (SWEEP_B), order hint and field: the plan answers unsupported — only to a field call, and only off the column kernel — or names
    an instantiation of the built code object with at most 160 KB of LDS, and a field plan is never kernel 1 or 2."""
    built_rows = set(_built_variants(tmp_path))
    assert len(built_rows) == len(KV.TABLE)
    points = unsupported = 0
    seen = set()
    for m in range(1, 11):
        for thb in (0, 1):
            for K in (0, 1, 2, 8):
                d = KV._cfg(m, 2, thb, 0, True)
                d["obstacles"] = [(0.0, 0.0, 0.1)] * K
                for N in sorted(set(SWEEP_N + [KV.KERNEL1[m] - 1, KV.KERNEL1[m], KV.KERNEL1[m] + 1])):
                    d["N"] = N
                    cc = KV.c_config(R.NLPConfig(**d), 10)
                    for pin in range(6):
                        for ordered in (0, 1):
                            for field in ((0, 1) if K else (0,)):      # a field call without obstacle rows is an argument error
                                for B in SWEEP_B:
                                    rc, got, lds, code = KV.variant_of_config(cc, pin, CUS, B, ordered, field)
                                    points += 1
                                    if rc != 0:
                                        assert rc == -2 and field, (m, thb, K, N, pin, ordered, field, B, rc)
                                        unsupported += 1
                                        continue
                                    assert got in built_rows and 0 <= lds <= 160 * 1024, (m, thb, K, N, pin, ordered, field, B, got, lds)
                                    assert code == (4 if (got[0] == 3 and got[4] > 64) else got[0]), (got, code)
                                    assert not field or (got[0] == 3 and got[3] & 4), (m, thb, K, N, pin, ordered, field, B, got)
                                    assert got[1] == m and (got[2] == thb or got[0] == 1), got
                                    seen.add(got)
    print("plan sweep: %d points, %d unsupported, %d of %d instantiations named" % (points, unsupported, len(seen), len(built_rows)))
    assert unsupported and {v[0] for v in seen} == {1, 2, 3}


def test_descriptor_of_config_argument_errors(built):
    """the codes of nmpc_create_opts for the configuration and the options, of nmpc_debug_variant for the call; no device is touched"""
    import ctypes as C
    import nmpc_amd
    L = nmpc_amd._lib.load()
    cc = KV.c_config(R.NLPConfig(**KV._cfg(2, 20, 0, 0, True)), 10)
    cc2 = KV.c_config(R.NLPConfig(**KV._cfg(2, 20, 0, 2, True)), 10)
    v = nmpc_amd._lib.CDebugVariant()
    assert KV.variant_of_config(cc, 0, CUS, -1, 0, 0)[0] == -1 and KV.variant_of_config(cc, 0, 0, 1, 0, 0)[0] == -1      # negative batch, no compute units
    assert KV.variant_of_config(cc, 6, CUS, 1, 0, 0)[0] == -1                                   # no such pin
    assert KV.variant_of_config(cc, 0, CUS, 4, 0, 1)[0] == -1                                   # a field call without obstacle rows
    assert KV.variant_of_config(cc2, 2, CUS, 4, 0, 1)[0] == -2                                  # a field call pinned off the column kernel
    assert KV.variant_of_config(cc2, 2, CUS, 4, 0, 0)[:2] == (0, (2, 2, 0, 0, 64))
    assert L.nmpc_debug_variant_of_config(None, None, CUS, 1, 0, 0, C.byref(v), None) == -1 and L.nmpc_debug_variant_of_config(C.byref(cc), None, CUS, 1, 0, 0, None, None) == -1
    assert L.nmpc_debug_variant_of_config(C.byref(cc), None, CUS, 1, 0, 0, C.byref(v), None) == 0 and v.kernel == 3      # options and kernel code are optional
    cc.m = 11
    assert KV.variant_of_config(cc, 0, CUS, 1, 0, 0)[0] == -2                                    # team size not instantiated
    cc.m, cc.N = 2, 1
    assert KV.variant_of_config(cc, 0, CUS, 1, 0, 0)[0] == -1


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
