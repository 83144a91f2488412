"""CPU: the plan-sensitivity entry point (nmpc_sens_batch) is declared, exported and bound, and the numpy reference the GPU tests hold it
against (tests/sens_ref.py) is right on the fixtures of tests/golden/sens_cases.npz: its stage recursion is its dense solve, it predicts the
oracle's re-solves to first order, saturated controls have no gain, and the two bad points get their verdicts.

Tolerance of recursion against dense solve: 100 x the spread of the recursion against itself under +-4 ulp moves of (w, lam_g, lam_x), + 1e-12,
relative to max|G| (max|dw|) — the project's pattern for two correct evaluations of one ill-conditioned definition (kernel_variants.path_spread)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import sens_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(S.case_configs())


@pytest.fixture(scope="module")
def cases():
    return S.load_cases()


def _field(c, b):
    return None if c["obs"] is None else c["obs"][b]


def test_entry_point_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    m = re.search(r"int32_t\s+nmpc_sens_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m, "nmpc_sens_batch is not declared in include/nmpc.h"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 14
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert "nmpc_sens_batch" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    assert "nmpc_sens_batch" in nmpc_amd._lib.EXPORTS
    assert len(L.nmpc_sens_batch.argtypes) == 14 and L.nmpc_sens_batch.restype is C.c_int32
    assert callable(nmpc_amd.NmpcSolver.sens_batch)
    for word in ("gain_stages", "Sigma_i = z_i / s_i", "G_k = -F_uu^-1 F_ux", "info  [B]"):      # the definition is written down where the ABI is
        assert word in hdr, word


def test_null_handle_is_an_argument_error_without_a_device(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert L.nmpc_sens_batch(None, 1, None, None, 0, None, None, None, None, None, None, 1, None, None) == -1


def test_the_fixture_covers_its_configurations(cases):
    assert set(cases) == set(NAMES)
    for name, c in cases.items():
        cfg = c["cfg"]
        assert c["p"].shape == (4, 2 * cfg.nx) and c["w"].shape == c["w_h"].shape == c["w_h2"].shape == (4, cfg.n_var), name
        assert c["lam_g"].shape == (4, cfg.n_g) and c["lam_x"].shape == (4, cfg.n_var) and c["h"] == 1e-2, name
        assert np.allclose(np.linalg.norm(c["d"], axis=1), 1.0, atol=1e-12), name
        assert (c["obs"] is None) == (c["kind"] is None), name
        if c["kind"]:
            assert c["obs"].shape == ((4, cfg.K, 3) if c["kind"] == "static" else (4, cfg.N, cfg.K, 3)), name
    active_pairs = sum(int((c["lam_g"][:, S.ineq_rows(c["cfg"])] < 0).sum()) for c in cases.values())
    assert active_pairs >= 20      # the barrier terms of the rows are exercised, not only the bounds


@pytest.mark.parametrize("name", NAMES)
def test_recursion_is_the_dense_solve(cases, name):
    c = cases[name]; cfg = c["cfg"]
    for b in range(4):
        a = (cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], _field(c, b))
        r = S.stage_recursion(*a, dp=c["d"][b])
        assert r["info"] == 0 and r["min_eig"] >= 1e-6, (name, b, r["info"], r["min_eig"])
        assert not S.kkt_system(*a)[2]
        eg, sg, ew, sw = S.recursion_against_dense(*a, dp=c["d"][b])
        print("%s %d: gains %.2e (spread %.2e), dw %.2e (spread %.2e), max|G| %.2e" % (name, b, eg, sg, ew, sw, np.abs(r["gains"]).max()))
        assert eg <= 100.0 * sg + 1e-12, (name, b, eg, sg)
        assert ew <= 100.0 * sw + 1e-12, (name, b, ew, sw)
        assert np.array_equal(r["dw"][: cfg.nx], c["d"][b][: cfg.nx])
        assert S.linearised_defect(cfg, c["w"][b], r["dw"]) <= 1e-12 * max(1.0, np.abs(r["dw"]).max())


@pytest.mark.parametrize("name", NAMES)
def test_first_order_prediction_of_the_oracles_resolves(cases, name):
    c = cases[name]; cfg = c["cfg"]
    for b in range(4):
        r = S.stage_recursion(cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], _field(c, b), dp=c["d"][b])
        e1, e2, ratio = S.prediction_errors(c["w"][b], r["dw"], c["w_h"][b], c["w_h2"][b], c["h"])
        e0 = np.abs(c["w_h"][b] - c["w"][b]).max()
        print("%s %d: errors %.2e %.2e ratio %.3f; leaving the plan as it is: %.2e" % (name, b, e1, e2, ratio, e0))
        assert 3.8 <= ratio <= 4.2, (name, b, ratio)
        assert e1 < e0, (name, b)


def test_saturated_stage0_controls_have_no_gain(cases):
    """saturated: the control's bound term |lam_x| / s is at least 1e7.  Its row of G_0 is then -F_ux / (that term) to first order, and the
    entries of F_ux are below 100 on these fixtures (max|G| <= 82 with F_uu of order 1): <= 1e-5."""
    seen = 0
    for name, c in cases.items():
        cfg = c["cfg"]
        for b in range(4):
            u0 = slice(cfg.nx * (cfg.N + 1), cfg.nx * (cfg.N + 1) + cfg.nu)
            lu0, ub = c["lam_x"][b][u0], R.bounds(cfg)[1][u0]
            sat = np.flatnonzero(np.abs(lu0) / (ub - np.abs(c["w"][b][u0])) >= 1e7)
            if sat.size == 0:
                continue
            G0 = S.stage_recursion(cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], _field(c, b))["gains"][0]
            print("%s %d: saturated controls %s, largest gain of their rows %.2e, of the others %.2e" % (
                name, b, sat.tolist(), np.abs(G0[sat]).max(), np.abs(np.delete(G0, sat, axis=0)).max()))
            assert np.abs(G0[sat]).max() <= 1e-5, (name, b)
            seen += sat.size
    assert seen >= 4, seen


def test_indefinite_point_gets_info_1(cases):
    c = cases["three3"]; cfg = c["cfg"]
    lam_g, k = S.indefinite_point(cfg, c["w"][0], c["lam_g"][0])
    r = S.stage_recursion(cfg, c["p"][0], c["w"][0], lam_g, c["lam_x"][0], dp=c["d"][0])
    print("stage %d, smallest eigenvalue of an F_uu %.3f" % (k, r["min_eig"]))
    assert k >= 1 and r["info"] == 1 and r["min_eig"] <= -1.0
    assert not r["gains"].any() and not r["dw"].any()


def test_positive_multiplier_without_slack_gets_info_2(cases):
    c = cases["three3"]; cfg = c["cfg"]
    w, lam_x = S.infeasible_point(cfg, c["w"][0], c["lam_x"][0])
    r = S.stage_recursion(cfg, c["p"][0], w, c["lam_g"][0], lam_x, dp=c["d"][0])
    assert r["info"] == 2 and not r["gains"].any() and not r["dw"].any()
    # the verdict goes before the indefinite one
    lam_g, _ = S.indefinite_point(cfg, w, c["lam_g"][0])
    assert S.stage_recursion(cfg, c["p"][0], w, lam_g, lam_x)["info"] == 2
