"""CPU: the table of LIDAR solve-kernel instantiations (tests/lidar_variants.py) is exactly the set of lidar_solve_kernel symbols in the built
gfx950 code object, the launch descriptor nmpc_debug_lidar_variant is declared, exported and bound, the recipes cover the shape edges they
claim, and every recipe's inputs are ones on which the oracle converges and agrees with itself."""
import os
import re
import subprocess
from collections import Counter

import pytest

from tests import helpers as Hh
from tests import lidar_variants as LV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built_instantiations(tmp_path):
    """(rays, waves) of every lidar_solve_kernel symbol of lib/libnmpc_hip.so"""
    got = []
    for name in Hh.kernel_notes(tmp_path):
        if "lidar_solve_kernel" not in name:
            continue
        m = re.search(r"^_ZN10nmpc_lidar18lidar_solve_kernelILi(n?\d+)ELi(\d+)EEE", name)
        assert m, "LIDAR solve kernel with an unknown template signature: " + name
        got.append((-int(m.group(1)[1:]) if m.group(1).startswith("n") else int(m.group(1)), int(m.group(2))))
    return got


def test_table_equals_the_lidar_solve_kernels_of_the_code_object(built, tmp_path):
    """One instantiation per set of rows and rows for every instantiation: a new lidar_solve_kernel<R_, W_> without a row fails here, and so
    does a row whose instantiation is gone."""
    got = _built_instantiations(tmp_path)
    assert len(got) == len(set(got)), [v for v, n in Counter(got).items() if n > 1]
    rows = Counter(r.inst for r in LV.TABLE)
    print("LIDAR solve-kernel instantiations and their rows: %s" % sorted(rows.items()))
    assert not sorted(set(got) - set(rows)), "instantiations without a table row: %s" % sorted(set(got) - set(rows))
    assert not sorted(set(rows) - set(got)), "table rows without an instantiation: %s" % sorted(set(rows) - set(got))
    assert set(got) == {(-1, 1), (10, 1), (10, 2)}
    keys = [LV.row_key(r) for r in LV.TABLE]
    assert len(keys) == len(set(keys)), [k for k, n in Counter(keys).items() if n > 1]
    assert set(LV.SEEDS) <= set(keys), set(LV.SEEDS) - set(keys)      # no seed left behind by a row that is gone


def test_lidar_descriptor_declared_exported_and_bound(built):
    import ctypes as C
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc_debug.h")).read()
    assert re.search(r"\bnmpc_debug_lidar_variant\s*\(", hdr) and "nmpc_debug_lidar_variant_t" in hdr
    assert "nmpc_debug_lidar_variant" not in open(os.path.join(ROOT, "include", "nmpc_lidar.h")).read()      # a development aid, not product ABI
    assert "nmpc_debug_lidar_variant" in nmpc_amd._lib.DEBUG_EXPORTS and "nmpc_debug_lidar_variant" not in nmpc_amd._lib.LIDAR_EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert "nmpc_debug_lidar_variant" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    assert len(L.nmpc_debug_lidar_variant.argtypes) == 3
    # the struct of the header: four int32 then one int64
    V = nmpc_amd._lib.CDebugLidarVariant
    assert [f[0] for f in V._fields_] == ["rays", "waves", "two_wave_above", "threads", "lds_bytes"]
    assert C.sizeof(V) == 24 and V.lds_bytes.offset == 16 and V.two_wave_above.offset == 8
    fields = re.search(r"typedef struct nmpc_debug_lidar_variant \{(.*?)\} nmpc_debug_lidar_variant_t;", hdr, re.S).group(1)
    assert re.findall(r"\b(int32_t|int64_t)\s+(\w+);", fields) == [("int32_t", "rays"), ("int32_t", "waves"), ("int32_t", "two_wave_above"),
                                                                   ("int32_t", "threads"), ("int64_t", "lds_bytes")]
    # a null handle or a null result is an argument error without touching a device
    v = V()
    assert L.nmpc_debug_lidar_variant(None, 1, C.byref(v)) == -1
    assert L.nmpc_debug_lidar_variant(None, 1, None) == -1
    # the solve call and the descriptor choose through one function: both call it, and neither looks at the batch threshold itself
    src = open(os.path.join(os.path.dirname(nmpc_amd._lib.__file__), "csrc", "nmpc_lidar.hip")).read()
    for fn in ("nmpc_lidar_solve_batch", "nmpc_debug_lidar_variant"):
        body = re.search(r"\nint32_t %s\([^)]*\)\n\{\n(.*?)\n\}\n" % fn, src, re.S).group(1)
        assert "lidar_launch_choice(h, B, " in body and "n_cu" not in body and "cfg.R" not in body, fn


def test_recipes_cover_the_shape_edges():
    by = {inst: [r for r in LV.TABLE if r.inst == inst] for inst in ((-1, 1), (10, 1), (10, 2))}
    assert {r.R for r in by[(-1, 1)]} == {0, 1, 2, 5, 6, 9, 11, 15, 16}      # every ray count the table claims for the predicated kernel
    assert {r.R for r in by[(10, 1)]} == {10} and {r.R for r in by[(10, 2)]} == {10}
    assert {r.R for r in LV.TABLE} == set(range(0, 17)) - {3, 4, 7, 8, 12, 13, 14}      # 3 and 4: tests/test_gpu_lidar.py
    for inst in ((-1, 1), (10, 1)):
        rows = by[inst]
        assert {r.N % 4 for r in rows} == {0, 1, 2, 3}, inst
        assert any(r.N < 64 for r in rows) and any(r.N == 64 for r in rows) and any(r.N > 128 for r in rows), inst
        assert any(r.Nc == 1 and r.N > 1 for r in rows) and any(r.Nc == r.N and r.N > 1 for r in rows), inst
        assert all(r.B == 16 for r in rows)
    assert len(by[(10, 2)]) >= 1 and all(r.B is None for r in by[(10, 2)])
    assert all(r.max_iter == 600 for r in LV.TABLE)
    # the rows, stated a second time: dropping or adding one fails here

    def ncs(N):
        return {1, max(1, N // 2), N}
    short, lanes = (1, 2, 3, 4, 5, 9), (63, 64, 65, 127, 128, 129)
    want = {((-1, 1), N, Nc, R, "base") for R in (0, 1, 2, 5, 6, 9, 11, 15, 16) for N in short for Nc in ncs(N)}
    want |= {((-1, 1), N, Nc, R, "base") for R in (0, 5, 11, 16) for N in lanes for Nc in ncs(N)}
    want |= {((10, 1), N, Nc, 10, "base") for N in short + lanes for Nc in ncs(N)}
    want |= {((10, 2), N, Nc, 10, "base") for (N, Nc) in ((5, 2), (8, 4), (12, 6), (65, 1))}
    for v in ("lw0", "dmax_inf", "th2", "lw0_free"):
        want |= {((-1, 1), 3, 1, 16, v), ((-1, 1), 9, 4, 5, v), ((-1, 1), 65, 32, 11, v), ((10, 1), 64, 64, 10, v), ((10, 2), 8, 4, 10, v)}
    have = {LV.row_key(r) for r in LV.TABLE}
    assert have == want, (sorted(want - have), sorted(have - want))
    assert LV.VARIANTS == {"base": {}, "lw0": {"lw": 0.0}, "dmax_inf": {"d_max": LV.INF}, "th2": {"th_max": 2.0},
                           "lw0_free": {"lw": 0.0, "d_max": LV.INF, "xy_max": LV.INF}}
    # the infeasible instance is instance 1 of every recipe, by the scan where there are rays and by the pose where there are none
    for r in (by[(-1, 1)][0], by[(10, 1)][0]):
        cfg, P, W0 = LV.inputs(r)
        assert (P[1, 0] == cfg.xy_max + 1.0) if r.R == 0 else (P[1, 6] == 0.05 < cfg.d_min)
    # a shorter batch of the generator is a prefix of a longer one (the budget-independence test solves prefixes)
    cfg = LV.config(by[(10, 2)][0])
    P5, W5 = LV.batch(cfg, 5, 9)
    P3, W3 = LV.batch(cfg, 3, 9)
    assert (P5[:3] == P3).all() and (W5[:3] == W3).all()


@pytest.mark.parametrize("r", LV.TABLE, ids=[LV.row_id(r) for r in LV.TABLE])
def test_oracle_holds_its_point_on_the_lidar_recipe_inputs(built, r):
    """Every recipe is screened: the oracle, run twice more with w0 and the goal perturbed by a few ulp, returns equal status vectors,
    converges on every instance but the infeasible instance 1, and holds its point (1e-8) and its iteration counts.  So a GPU instance off
    the oracle's point, or a status that differs, is the GPU's doing, and the parity test needs no share."""
    s = LV.screen(r)
    assert s.status_equal and s.converged and s.held, (LV.row_id(r), r.seed, s)
    assert s.iters < r.max_iter
