"""CPU: the adjoint plan-sensitivity entry point (nmpc_sens_adjoint_batch) is declared, exported and bound, its kernel has one instantiation per row of
tests/sens_points.SENS_TABLE, and the numpy reference the GPU tests hold it against (tests/sens_adjoint_ref.py) is right on its own: the stage
recursion is the dense adjoint solve, <pbar, dp> = <wbar, S_p dp> and <obsbar, dobs> = <wbar, S_o dobs> against the dense forward maps, a static
field given as [K, 3] is the stage sum of the same field given per stage, entry 0 of a per-stage field gets nothing, verdicts zero the outputs, every
term of M_o is visible at 1000 x the parity bound, and S_o predicts the oracle's re-solves under a moved field to first order
(tests/golden/sens_obs_cases.npz).

The parity bound is the project's: 100 x the spread of the recursion against itself under +-4 ulp moves of (w, lam_g, lam_x), + 1e-12, relative to
max|pbar| (max|obsbar|)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
FIELD = [i for i, r in enumerate(ROWS) if r.kind in ("static", "moving")]
FIELD_IDS = [IDS[i] for i in FIELD]
VISIBLE = 1000.0
OBS_NAMES = list(AR.obs_case_configs())


def test_entry_point_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    m = re.search(r"int32_t\s+nmpc_sens_adjoint_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m, "nmpc_sens_adjoint_batch is not declared in include/nmpc.h"
    assert len(m.group(1).split(",")) == 13
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert "nmpc_sens_adjoint_batch" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    assert "nmpc_sens_adjoint_batch" in nmpc_amd._lib.EXPORTS
    assert len(L.nmpc_sens_adjoint_batch.argtypes) == 13 and L.nmpc_sens_adjoint_batch.restype is C.c_int32
    assert callable(nmpc_amd.NmpcSolver.sens_adjoint_batch) and callable(nmpc_amd.NmpcLayer)
    for word in ("S_o : dobs -> dw", "-l (I - n n') / rr - Sigma n n'", "-Sigma n", "<pbar, dp> = <wbar, S_p dp>", "obsbar [B][S][K][3]"):
        assert word in hdr, word


def test_null_handle_is_an_argument_error_without_a_device(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert L.nmpc_sens_adjoint_batch(None, 1, None, None, 0, None, None, None, None, None, None, None, None) == -1


def test_table_equals_the_adjoint_kernels_of_the_code_object(built, tmp_path):
    got = []
    for name in Hh.kernel_notes(tmp_path):
        m = re.search(r"^_ZN4nmpc11sens_kernelILi(\d+)ELi1EEE", name)
        if m:
            ms = int(m.group(1))
            got.append((ms % 16, ms // 16))
            continue
        assert not re.search(r"sens_(adjoint_|fwd_)?kernel(?!ILi\d+ELi[012]EEE)", name), "adjoint kernel with an unknown template signature: " + name
    rows = [(r.m, r.field) for r in ROWS]
    assert len(got) == len(set(got)) == 20, sorted(got)
    assert set(got) == set(rows), (sorted(set(got) - set(rows)), sorted(set(rows) - set(got)))


@functools.lru_cache(maxsize=None)
def screened(i):
    """per point of row i: the recursion, the dense adjoint, the spread and the bounds"""
    r = ROWS[i]
    out = []
    for n, pt in enumerate(SP.points(r)):
        a = (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        wbar = AR.row_cotangent(r, n)
        ref = AR.stage_adjoint(*a, wbar)
        pb, ob = AR.dense_reference(*a, wbar)
        sp, so = AR.spread(*a, wbar)
        out.append(dict(wbar=wbar, ref=ref, pb=pb, ob=ob, sp=sp, so=so, bp=100.0 * sp + 1e-12, bo=100.0 * so + 1e-12))
    return out


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_recursion_is_the_dense_adjoint(i):
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        ep, eo = AR.rel(o["ref"]["pbar"], o["pb"]), AR.rel(o["ref"]["obsbar"], o["ob"])
        print("%s %d: pbar %.2e (spread %.2e), obsbar %.2e (spread %.2e)" % (SP.row_id(r), n, ep, o["sp"], eo, o["so"]))
        assert o["ref"]["info"] == 0
        assert ep <= o["bp"] and eo <= o["bo"], (n, ep, o["sp"], eo, o["so"])
        assert (o["ref"]["obsbar"] is None) == (r.kind in ("own", None))
        assert np.abs(o["wbar"]).min() >= 0.5      # weight on every entry, X_0 and X_N included


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_dot_product_identities_against_the_dense_forward_maps(i):
    """<pbar, dp> = <wbar, S_p dp> and <obsbar, dobs> = <wbar, S_o dobs> for random dp, dobs: to the parity bound, relative to |pbar| |dp|
    (|obsbar| |dobs|) — the two sides come from two solves with one matrix"""
    r = ROWS[i]; cfg = r.cfg
    rng = np.random.default_rng(r.seed)
    for n, (pt, o) in enumerate(zip(SP.points(r), screened(i))):
        W, A, _ = S.kkt_system(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        dP = rng.normal(size=(2 * cfg.nx, 3))
        lhs, rhs = o["ref"]["pbar"] @ dP, o["wbar"] @ AR.dense_s_p(cfg, W, A, dP)
        ep = np.abs(lhs - rhs).max() / (np.linalg.norm(o["ref"]["pbar"]) * np.linalg.norm(dP, axis=0).max())
        eo = 0.0
        if o["ref"]["obsbar"] is not None:
            Mo = AR.obstacle_matrix(cfg, pt.w, pt.lam_g, pt.obs)
            dO = rng.normal(size=(Mo.shape[1], 3))
            lhs, rhs = o["ref"]["obsbar"].reshape(-1) @ dO, o["wbar"] @ AR.dense_s_o(cfg, W, A, Mo, dO)
            eo = np.abs(lhs - rhs).max() / (np.linalg.norm(o["ref"]["obsbar"]) * np.linalg.norm(dO, axis=0).max())
        print("%s %d: identity of pbar %.2e, of obsbar %.2e" % (SP.row_id(r), n, ep, eo))
        assert ep <= o["bp"] and eo <= o["bo"], (n, ep, eo)


@pytest.mark.parametrize("i", [i for i in FIELD if ROWS[i].kind == "static"], ids=[IDS[i] for i in FIELD if ROWS[i].kind == "static"])
def test_static_field_is_the_stage_sum_of_the_same_field_per_stage(i):
    r = ROWS[i]; cfg = r.cfg
    for n, (pt, o) in enumerate(zip(SP.points(r), screened(i))):
        per_stage = np.broadcast_to(pt.obs, (cfg.N,) + pt.obs.shape).copy()
        b = AR.stage_adjoint(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, per_stage, o["wbar"])
        assert b["obsbar"].shape == (cfg.N, cfg.K, 3) and o["ref"]["obsbar"].shape == (1, cfg.K, 3)
        assert np.array_equal(b["pbar"].view(np.int64), o["ref"]["pbar"].view(np.int64))
        assert AR.rel(b["obsbar"].sum(axis=0), o["ref"]["obsbar"][0]) <= 1e-12, n      # the same terms in another order of summation


@pytest.mark.parametrize("i", [i for i in FIELD if ROWS[i].kind == "moving"], ids=[IDS[i] for i in FIELD if ROWS[i].kind == "moving"])
def test_entry_0_of_a_per_stage_field_gets_nothing(i):
    for o in screened(i):
        assert not o["ref"]["obsbar"][0].any() and o["ref"]["obsbar"][1:].any()
        assert not o["ob"][0].any()


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_zero_the_outputs(r):
    wbar = AR.row_cotangent(r, 0)
    for name, pt, want in SP.verdict_cases(r, SP.points(r)[0]):
        a = AR.stage_adjoint(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, wbar)
        assert a["info"] == want == SP.reference(r, pt)["info"], (name, a["info"], want)
        if want:
            assert not a["pbar"].any() and not a["obsbar"].any(), name
        else:
            assert a["pbar"].any() and a["obsbar"].any(), name


@pytest.mark.parametrize("i", FIELD, ids=FIELD_IDS)
def test_every_term_of_the_obstacle_blocks_is_visible(i):
    """a kernel without the Sigma n n' term, without the radius column, or (per-stage fields) reading entry 0 at every stage: the reference moves by
    1000 x the parity bound or more on at least two points of the row"""
    r = ROWS[i]
    for drop in ("sigma_nn", "r_column") + (("first_entry",) if r.kind == "moving" else ()):
        f = []
        for pt, o in zip(SP.points(r), screened(i)):
            b = AR.stage_adjoint(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, o["wbar"], drop=drop)
            assert np.array_equal(b["pbar"], o["ref"]["pbar"])      # M_o does not enter pbar
            f.append(AR.rel(b["obsbar"], o["ref"]["obsbar"]) / o["bo"])
        f.sort()
        print("%s %-11s: factors %s" % (SP.row_id(r), drop, " ".join("%.1e" % v for v in f)))
        assert f[-2] >= VISIBLE, (drop, f)


# ---- S_o is the NLP's obstacle derivative: tests/golden/sens_obs_cases.npz
@pytest.fixture(scope="module")
def obs_cases():
    return AR.load_obs_cases()


def test_the_obstacle_fixture_covers_its_configurations(obs_cases):
    assert set(obs_cases) == set(OBS_NAMES) and 3 <= len(OBS_NAMES) <= 4
    kinds = set()
    for name, c in obs_cases.items():
        cfg = c["cfg"]; kinds.add((cfg.m, c["kind"]))
        assert cfg.N <= 8 and c["h"] == AR.H_OBS
        assert c["p"].shape == (4, 2 * cfg.nx) and c["w"].shape == c["w_h"].shape == c["w_h2"].shape == (4, cfg.n_var), name
        assert c["obs"].shape == c["d"].shape == ((4, cfg.K, 3) if c["kind"] == "static" else (4, cfg.N, cfg.K, 3)), name
        assert np.allclose(np.linalg.norm(c["d"].reshape(4, -1), axis=1), 1.0, atol=1e-12), name
    assert kinds == {(1, "moving"), (2, "static"), (3, "moving")}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sens_obs_cases.npz")) <= 200 * 1024


@pytest.mark.parametrize("name", OBS_NAMES)
def test_obstacle_map_predicts_the_oracles_resolves(obs_cases, name):
    """the screen and the acceptance rule of tests/test_sens_host.py on sens_cases.npz: info 0, F_uu positive definite, the recursion is the dense
    solve, the prediction error of w + h S_o d falls by about 4 when h is halved and is below leaving the plan as it is"""
    c = obs_cases[name]; cfg = c["cfg"]
    for b in range(4):
        a = (cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], c["obs"][b])
        r = S.stage_recursion(*a)
        assert r["info"] == 0 and r["min_eig"] >= 1e-6 and not S.kkt_system(*a)[2], (name, b)
        wbar = AR.cotangent(cfg, b)
        ad = AR.stage_adjoint(*a, wbar)
        pb, ob = AR.dense_reference(*a, wbar)
        sp, so = AR.spread(*a, wbar)
        assert AR.rel(ad["pbar"], pb) <= 100.0 * sp + 1e-12 and AR.rel(ad["obsbar"], ob) <= 100.0 * so + 1e-12, (name, b)
        dw = AR.obs_prediction(*a, c["d"][b])
        e1, e2, ratio = S.prediction_errors(c["w"][b], dw, c["w_h"][b], c["w_h2"][b], c["h"])
        e0 = np.abs(c["w_h"][b] - c["w"][b]).max()
        mis = AR.obs_mismatch(c, b, ad["obsbar"].reshape(c["d"][b].shape), wbar)
        print("%s %d: errors %.2e %.2e ratio %.3f; leaving the plan as it is: %.2e; <obsbar, d> against <wbar, dq>: %.2e" % (name, b, e1, e2, ratio, e0, mis))
        assert 3.8 <= ratio <= 4.2, (name, b, ratio)
        assert e1 < e0, (name, b)
        assert np.count_nonzero(ad["obsbar"]) > 0
