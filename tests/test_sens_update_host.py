"""CPU: the forward plan-update entry point (nmpc_sens_update_batch) is declared, exported and bound, its kernel has one instantiation per row of
tests/sens_points.SENS_TABLE, and the numpy reference the GPU tests hold it against (tests/sens_update_ref.py) is right on its own: the stage
recursion is the dense bordered solve, without dobs and rhs it is sens_ref.stage_recursion, with rhs = wbar alone it is the v of
sens_adjoint_ref.stage_adjoint, <obsbar, dobs> = <wbar, S_o dobs> and <pbar, dp> = <wbar, S_p dp> hold against the adjoint reference, every term
of M_o is visible in dw at 1000 x the parity bound, alpha keeps every linearised slack non-negative and is tight, and the fixtures
(tests/golden/sens_update_cases.npz) pass their own screen.

The parity bound is the project's: 100 x the spread of the recursion against itself under +-4 ulp moves of (w, lam_g, lam_x), + 1e-12, relative to
max|dw| (to alpha)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as Hh
from tests import sens_adjoint_ref as AR
from tests import sens_points as SP
from tests import sens_ref as S
from tests import sens_update_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
FIELD = [i for i, r in enumerate(ROWS) if r.kind in ("static", "moving")]
FIELD_IDS = [IDS[i] for i in FIELD]
VISIBLE = 1000.0
NAMES = list(AR.obs_case_configs())


def test_entry_point_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    m = re.search(r"int32_t\s+nmpc_sens_update_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m, "nmpc_sens_update_batch is not declared in include/nmpc.h"
    assert len(m.group(1).split(",")) == 15
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert "nmpc_sens_update_batch" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    assert "nmpc_sens_update_batch" in nmpc_amd._lib.EXPORTS
    assert len(L.nmpc_sens_update_batch.argtypes) == 15 and L.nmpc_sens_update_batch.restype is C.c_int32
    assert callable(nmpc_amd.NmpcSolver.sens_update_batch) and callable(nmpc_amd.AdvancedStepController)
    for word in ("M_o dobs", "alpha = min(1, min_i s_i / (-ds_i))", "goal, then rhs, then the obstacles in index order", "dobs [B][S][K][3]"):
        assert word in hdr, word


def test_null_handle_is_an_argument_error_without_a_device(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert L.nmpc_sens_update_batch(None, 1, None, None, 0, None, None, None, None, None, None, None, None, None, None) == -1


def test_table_equals_the_update_kernels_of_the_code_object(built, tmp_path):
    got = []
    for name in Hh.kernel_notes(tmp_path):
        m = re.search(r"^_ZN4nmpc11sens_kernelILi(\d+)ELi2EEE", name)
        if m:
            ms = int(m.group(1))
            got.append((ms % 16, ms // 16))
            continue
        assert not re.search(r"sens_(adjoint_|fwd_)?kernel(?!ILi\d+ELi[012]EEE)", name), "update kernel with an unknown template signature: " + name
    rows = [(r.m, r.field) for r in ROWS]
    assert len(got) == len(set(got)) == 20, sorted(got)
    assert set(got) == set(rows), (sorted(set(got) - set(rows)), sorted(set(rows) - set(got)))


@functools.lru_cache(maxsize=None)
def screened(i):
    """per point of row i: the inputs, the recursion, the dense solve, the spreads and the bounds"""
    r = ROWS[i]
    out = []
    for n, pt in enumerate(SP.points(r)):
        a = (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        dobs, rhs = UR.row_dobs(r, n), UR.row_rhs(r, n)
        ref = UR.stage_update(*a, dp=pt.dp, dobs=dobs, rhs=rhs)
        dense = UR.dense_update(*a, dp=pt.dp, dobs=dobs, rhs=rhs)
        sw, sa = UR.spread(*a, dp=pt.dp, dobs=dobs, rhs=rhs)
        out.append(dict(a=a, pt=pt, dobs=dobs, rhs=rhs, ref=ref, dense=dense, sw=sw, sa=sa, bw=100.0 * sw + 1e-12, ba=100.0 * sa + 1e-12))
    return out


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_recursion_is_the_dense_solve(i):
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        e = UR.rel(o["ref"]["dw"], o["dense"])
        print("%s %d: dw %.2e (spread %.2e), alpha %.6g (spread %.2e)" % (SP.row_id(r), n, e, o["sw"], o["ref"]["alpha"], o["sa"]))
        assert o["ref"]["info"] == 0
        assert e <= o["bw"], (n, e, o["sw"])
        assert (o["dobs"] is None) == (r.kind in ("own", None))
        assert np.abs(o["rhs"]).min() >= 0.5 and (o["dobs"] is None or np.abs(o["dobs"]).min() >= 0.01)      # weight on every entry
        assert o["dobs"] is None or o["dobs"].shape == np.shape(o["pt"].obs)


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_special_cases_are_the_two_existing_references(i):
    """dobs = rhs = 0: the dw of sens_ref.stage_recursion; rhs = wbar alone: the v of sens_adjoint_ref.stage_adjoint"""
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        fw = S.stage_recursion(*o["a"], dp=o["pt"].dp)["dw"]
        mine = UR.stage_update(*o["a"], dp=o["pt"].dp)
        assert mine["info"] == 0 and UR.rel(mine["dw"], fw) <= o["bw"], (n, UR.rel(mine["dw"], fw))
        wbar = AR.row_cotangent(r, n)
        v = AR.stage_adjoint(*o["a"], wbar)["v"]
        mine = UR.stage_update(*o["a"], rhs=wbar)
        assert mine["info"] == 0 and UR.rel(mine["dw"], v) <= o["bw"], (n, UR.rel(mine["dw"], v))
        assert not mine["dw"][: r.cfg.nx].any()      # v_X0 = 0


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_dot_product_identities_against_the_adjoint_reference(i):
    """<obsbar, dobs> = <wbar, S_o dobs> and <pbar, dp> = <wbar, S_p dp> with pbar, obsbar of sens_adjoint_ref.stage_adjoint: each side within its
    own parity bound"""
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        wbar = AR.row_cotangent(r, n)
        ad = AR.stage_adjoint(*o["a"], wbar)
        sp, so = AR.spread(*o["a"], wbar)
        dw = UR.stage_update(*o["a"], dp=o["pt"].dp)["dw"]
        lhs, rhs = ad["pbar"] @ o["pt"].dp, wbar @ dw
        tol = (100.0 * sp + 1e-12) * np.abs(ad["pbar"]).max() * np.abs(o["pt"].dp).sum() + o["bw"] * np.abs(dw).max() * np.abs(wbar).sum()
        assert abs(lhs - rhs) <= tol, (n, lhs, rhs, tol)
        eo = 0.0
        if o["dobs"] is not None:
            dw = UR.stage_update(*o["a"], dobs=o["dobs"])["dw"]
            lhs, rhs = np.sum(ad["obsbar"].reshape(o["dobs"].shape) * o["dobs"]), wbar @ dw
            tol = (100.0 * so + 1e-12) * np.abs(ad["obsbar"]).max() * np.abs(o["dobs"]).sum() + o["bw"] * np.abs(dw).max() * np.abs(wbar).sum()
            eo = abs(lhs - rhs)
            assert dw.any() and eo <= tol, (n, lhs, rhs, tol)
        print("%s %d: identities hold, obstacle side off by %.2e" % (SP.row_id(r), n, eo))


@pytest.mark.parametrize("i", FIELD, ids=FIELD_IDS)
def test_every_term_of_the_obstacle_blocks_is_visible_in_dw(i):
    """a kernel without the Sigma n n' term, without the radius column, or (per-stage fields) reading entry 0 at every stage: dw moves by 1000 x the
    point's parity bound or more on at least two points of the row"""
    r = ROWS[i]
    for drop in ("sigma_nn", "r_column") + (("first_entry",) if r.kind == "moving" else ()):
        f = []
        for o in screened(i):
            b = UR.stage_update(*o["a"], dp=o["pt"].dp, dobs=o["dobs"], rhs=o["rhs"], drop=drop)
            f.append(UR.rel(b["dw"], o["ref"]["dw"]) / o["bw"])
        f.sort()
        print("%s %-11s: factors %s" % (SP.row_id(r), drop, " ".join("%.1e" % v for v in f)))
        assert f[-2] >= VISIBLE, (drop, f)


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_alpha_keeps_every_slack_and_is_tight(i):
    """min_i (s_i + alpha ds_i) >= 0 within rounding; where alpha < 1 the limiting item's s + alpha ds is zero within the bound; halving the
    inputs doubles an alpha below 1/2"""
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        ref = o["ref"]; al = ref["alpha"]
        s, ds = UR.alpha_items(r.cfg, o["pt"].w, o["pt"].obs, ref["dw"], o["dobs"])
        m = (s > 0.0) & (ds < 0.0)
        assert 0.0 < al <= 1.0
        left = s[m] + al * ds[m]
        assert (left >= -4.0 * np.finfo(float).eps * s[m]).all(), (n, left.min())
        if al < 1.0:
            k = int(np.argmin(s[m] / -ds[m]))
            assert abs(left[k]) <= o["ba"] * s[m][k], (n, left[k], s[m][k])
        else:
            assert not m.any() or (s[m] / -ds[m]).min() >= 1.0
        if al < 0.5:
            half = UR.stage_update(*o["a"], dp=0.5 * o["pt"].dp, dobs=None if o["dobs"] is None else 0.5 * o["dobs"], rhs=0.5 * o["rhs"])
            assert abs(half["alpha"] - 2.0 * al) <= o["ba"] * 2.0 * al, (n, half["alpha"], al)
        print("%s %d: alpha %.6g over %d items, %d of them limiting" % (SP.row_id(r), n, al, s.size, int(m.sum())))


def test_nothing_to_do_is_alpha_one_and_no_change():
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3)
    pt = SP.points(r)[0]
    z = UR.stage_update(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=np.zeros(2 * r.cfg.nx), dobs=np.zeros_like(pt.obs), rhs=np.zeros(r.cfg.n_var))
    assert z["info"] == 0 and z["alpha"] == 1.0 and not z["dw"].any()
    n = UR.stage_update(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
    assert n["info"] == 0 and n["alpha"] == 1.0 and not n["dw"].any()


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_zero_dw_and_alpha(r):
    dobs, rhs = UR.row_dobs(r, 0), UR.row_rhs(r, 0)
    for name, pt, want in SP.verdict_cases(r, SP.points(r)[0]):
        a = UR.stage_update(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=pt.dp, dobs=dobs, rhs=rhs)
        assert a["info"] == want == SP.reference(r, pt)["info"], (name, a["info"], want)
        if want:
            assert not a["dw"].any() and a["alpha"] == 0.0, name
        else:
            assert a["dw"].any() and a["alpha"] > 0.0, name


# ---- the update is the NLP's derivative under a simultaneous move: tests/golden/sens_update_cases.npz
@pytest.fixture(scope="module")
def cases():
    return UR.load_cases()


def test_the_fixture_covers_its_configurations(cases):
    assert set(cases) == set(NAMES)
    for name, c in cases.items():
        cfg = c["cfg"]
        assert cfg.N <= 8 and c["h"] == UR.H_UPD == 2e-3
        assert c["p"].shape == (4, 2 * cfg.nx) and c["dx"].shape == (4, cfg.nx) and c["w"].shape == c["w_h"].shape == c["w_h2"].shape == (4, cfg.n_var), name
        assert c["obs"].shape == c["d"].shape == ((4, cfg.K, 3) if c["kind"] == "static" else (4, cfg.N, cfg.K, 3)), name
        assert np.allclose(np.linalg.norm(c["d"].reshape(4, -1), axis=1), 1.0, atol=1e-12) and np.allclose(np.linalg.norm(c["dx"], axis=1), 1.0, atol=1e-12), name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sens_update_cases.npz")) <= 200 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_the_fixtures_pass_their_own_screen(cases, name):
    c = cases[name]; cfg = c["cfg"]
    for b in range(4):
        s = UR.screen(cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], c["obs"][b], c["dx"][b], c["d"][b], c["w_h"][b], c["w_h2"][b], c["h"])
        print("%s %d: errors %.2e %.2e ratio %.3f, alpha(h) %.6f, |U_0| error %.2e against %.2e when the plan is left as it is" % (
            name, b, s["e1"], s["e2"], s["ratio"], s["alpha_h"], s["e_u"], s["e_u0"]))
        assert s["info"] == 0 and s["min_eig"] >= 1e-6, (name, b)
        assert 3.8 <= s["ratio"] <= 4.2, (name, b, s["ratio"])
        assert s["alpha_h"] == 1.0, (name, b, s["alpha_h"])
        assert s["e_u"] < s["e_u0"], (name, b)
        assert s["ok"]
