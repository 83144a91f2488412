"""CPU: the tracking solve (nmpc_solve_batch_ref / nmpc_step_batch_ref) as far as it can be held without a device — the entry points are
declared, exported and bound; the table of tracking instantiations (tests/track_variants.py) is exactly the set of track_col_kernel symbols of
the built gfx950 code object and every recipe is named by the device-free descriptor; and the checker of the GPU tests
(tests/tracking_ipm.py) is the project's prototype on constant rows, meets the SLSQP fixtures, and converges on every recipe's inputs."""
import inspect
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

from oracle import ipm_proto as IP
from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import track_variants as TV
from tests import tracking_ipm as TI
from tests import tracking_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nmpc_solve_batch_ref", "nmpc_step_batch_ref")


def test_entry_points_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in nmpc_amd._lib.EXPORTS and n in exported, n
        assert len(getattr(L, n).argtypes) == 16, n
    assert "ref [B][S][n_x]" in hdr and "2 Q (X_k - xs_k)" in hdr and "take no per-stage reference" not in hdr
    dbg = open(os.path.join(ROOT, "include", "nmpc_debug.h")).read()
    assert re.search(r"\bnmpc_debug_track_variant_of_config\s*\(", dbg) and "nmpc_debug_track_variant_of_config" in nmpc_amd._lib.DEBUG_EXPORTS
    assert "nmpc_debug_track_variant_of_config" in exported and "nmpc_debug_track" not in hdr


def test_null_handle_is_an_argument_error(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert L.nmpc_solve_batch_ref(None, 1, None, None, 1, None, 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.nmpc_step_batch_ref(None, 1, None, None, None, None, 1, None, 0, None, None, None, None, None, None, None) == -1


def test_reference_in_both_signatures(built):
    import nmpc_amd
    for f in (nmpc_amd.NmpcSolver.solve_batch, nmpc_amd.NmpcSolver.step_batch):
        par = inspect.signature(f).parameters
        assert "reference" in par and par["reference"].default is None, f
    par = inspect.signature(nmpc_amd.simulate_tracking).parameters
    assert list(par)[:4] == ["solver", "x0", "reference_paths", "max_steps"] and "obstacle_paths" in par and "keep_states" in par


def _built_track_rows(tmp_path):
    got = []
    for name in Hh.kernel_notes(tmp_path):
        m = re.search(r"^_ZN4nmpc16track_col_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEE", name)
        if m:
            mm, thb, dl, tpb = (int(g) for g in m.groups())
            got.append((3, mm, thb, dl | TV.TRACK, tpb))
            continue
        assert not re.search(r"^_ZN4nmpc\d+track_\w*kernel", name), "tracking kernel with an unknown template signature: " + name
    return got


def test_table_equals_the_tracking_kernels_of_the_code_object(built, tmp_path):
    """one row per track_col_kernel symbol and one symbol per row; every row is a field row of the swarm table with 8 added, and every field
    row of the swarm table has its tracking row"""
    got = _built_track_rows(tmp_path)
    assert got and len(got) == len(set(got)), [v for v, n in Counter(got).items() if n > 1]
    rows = [r.row for r in TV.TRACK_TABLE]
    assert len(rows) == len(set(rows))
    assert not sorted(set(got) - set(rows)), "instantiations without a table row: %s" % sorted(set(got) - set(rows))
    assert not sorted(set(rows) - set(got)), "table rows without an instantiation: %s" % sorted(set(rows) - set(got))
    assert all(fl & 4 and fl & TV.TRACK for (_, _, _, fl, _) in got)
    field_rows = {r.row for r in KV.TABLE if r.row[0] == 3 and r.row[3] & 4}
    assert {(k, m, thb, fl ^ TV.TRACK, tpb) for (k, m, thb, fl, tpb) in got} == field_rows


def test_every_row_is_named_by_its_recipe(built):
    """the device-free descriptor answers each recipe (horizon by its rule, pin, B, ordered, field) with the recipe's row, in the LDS bytes of
    the sibling nmpc_solve_batch_obs launch (the reference's rows stay in device memory), with kernel code 3 or 4"""
    for r in TV.TRACK_TABLE:
        cc = KV.c_config(TV.recipe_cfg(r), r.max_iter)
        rc, got, lds, code = TV.track_variant_of_config(cc, r.pin, TV.CUS, r.B, r.ordered, r.field)
        assert rc == 0 and got == r.row and 0 < lds <= 160 * 1024, (r.row, rc, got, lds)
        assert code == (4 if got[4] > 64 else 3), (r.row, code)
        rc2, sib, lds2, _ = KV.variant_of_config(cc, r.pin, TV.CUS, r.B, r.ordered, 1)
        assert rc2 == 0 and sib == got[:3] + (got[3] ^ TV.TRACK,) + got[4:] and lds2 == lds, (r.row, sib, lds2, lds)
    # the flag flips where the rule says: one horizon below, the layout is still the richer one
    for r in TV.TRACK_TABLE:
        if r.horizon in ("factors_out", "duals_out", "waves4"):
            d = TV._cfg_dict(r, TV.horizon(r) - 1)
            _, below, _, _ = TV.track_variant_of_config(KV.c_config(R.NLPConfig(**d), 10), r.pin, TV.CUS, r.B, r.ordered, r.field)
            assert below != r.row, (r.row, below)


def test_descriptor_argument_errors(built):
    cc = KV.c_config(R.NLPConfig(**KV._cfg(2, 20, 0, 0, True)), 10)
    cc2 = KV.c_config(R.NLPConfig(**KV._cfg(2, 20, 0, 2, True)), 10)
    assert TV.track_variant_of_config(cc, 0, TV.CUS, 4, 0, 0)[:2] == (0, (3, 2, 0, 2 | 4 | TV.TRACK, 64))      # no obstacle rows: the field is never read
    assert TV.track_variant_of_config(cc, 0, TV.CUS, 4, 0, 1)[0] == -1           # a field without obstacle rows
    assert TV.track_variant_of_config(cc2, 2, TV.CUS, 4, 0, 0)[0] == -2          # pinned off the column kernel
    assert TV.track_variant_of_config(cc2, 1, TV.CUS, 4, 0, 1)[0] == -2
    assert TV.track_variant_of_config(cc2, 0, 0, 4, 0, 0)[0] == -1 and TV.track_variant_of_config(cc2, 0, TV.CUS, -1, 0, 0)[0] == -1
    c6 = KV.c_config(R.NLPConfig(**KV._cfg(6, KV.KERNEL1[6], 0, 0, True)), 10)                # beyond the column kernel's LDS
    assert TV.track_variant_of_config(c6, 0, TV.CUS, 4, 0, 0)[0] == -2


def test_checker_equals_the_prototype_on_constant_rows():
    """ref rows all equal to the goal, as one row and tiled: the iterate, the objective, the multipliers and the iteration count of
    oracle/ipm_proto.py bit for bit"""
    for cfg, seed in ((R.NLPConfig(m=2, N=8, T=0.3, dmin=0.4, v_max=0.15, w_max=1.5), 5), (Hh.cfg_mix3(6), 6),
                      (R.NLPConfig(m=1, N=8, T=0.2, dmin=0.0, v_max=0.2, w_max=1.0, pad_rows=False, th_max=3.5), 7)):
        P, W0 = Hh.batch(cfg, 2, seed)
        for p, w0 in zip(P, W0):
            a = IP.solve(cfg, p, w0)
            for ref in (p[cfg.nx:], np.tile(p[cfg.nx:], (cfg.N, 1))):
                b = TI.solve(cfg, np.concatenate([p[: cfg.nx], np.full(cfg.nx, np.nan)]), ref, w0)
                assert a["status"] == b["status"] == 0 and a["iters"] == b["iters"]
                assert np.array_equal(a["x"], b["x"]) and a["f"] == b["f"] and np.array_equal(a["lam"], b["lam"]) and a["kkt"] == b["kkt"]


def test_checker_meets_the_slsqp_fixtures():
    """the 15 fixtures of tests/golden/slsqp_track.npz: status 0, w within 1e-4 and f within 1e-6 relative of SLSQP's"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "slsqp_track.npz"))
    fam = TR.families()
    n = 0
    for name, cfg in fam.items():
        P, REF, W0 = TR.family_inputs(name, cfg)
        assert np.array_equal(REF, z[name + "_ref"]) and np.array_equal(P[:, : cfg.nx], z[name + "_p"][:, : cfg.nx])
        for b in range(P.shape[0]):
            r = TI.solve(cfg, P[b], REF[b], W0[b])
            dw, df = np.max(np.abs(r["x"] - z[name + "_w"][b])), abs(r["f"] - z[name + "_f"][b]) / max(1.0, abs(z[name + "_f"][b]))
            print("%s[%d]: status %d iters %d |dw| %.2e df %.2e" % (name, b, r["status"], r["iters"], dw, df))
            assert r["status"] == 0 and dw <= 1e-4 and df <= 1e-6, (name, b, r["status"], dw, df)
            n += 1
    assert n == 15


@pytest.mark.parametrize("r", TV.TRACK_TABLE, ids=[TV.row_id(r) for r in TV.TRACK_TABLE])
def test_checker_converges_on_the_recipe_inputs(built, r):
    """the screen: on every recipe's four instances the checker ends with status 0 (the allowance of one instance per row is not used)"""
    res = TV.checker(r)
    st = [o["status"] for o in res]
    print(TV.row_id(r), "N", TV.horizon(r), "status", st, "iters", [o["iters"] for o in res])
    assert st == [0] * TV.NB, (r.row, st)
