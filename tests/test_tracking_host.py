"""CPU: the pose-reference entry points (nmpc_eval_batch_ref, nmpc_kkt_batch_ref) are declared,
exported and bound, and the numpy restatement the GPU tests hold them against (tests/tracking_ref.py) is oracle.nlp_ref's cost for a
constant path, differentiates correctly for a moving one, and agrees with its own SLSQP fixtures (tests/golden/slsqp_track.npz)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import tracking_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nmpc_eval_batch_ref": 11, "nmpc_kkt_batch_ref": 13}      # name -> arguments in include/nmpc.h
GOLDEN = os.path.join(ROOT, "tests", "golden", "slsqp_track.npz")


def test_entry_points_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name + " is not declared in include/nmpc.h"
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs, name
        assert name in exported and name in nmpc_amd._lib.EXPORTS, name
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int32, name
    # every exported nmpc_* symbol that is not a debug or LIDAR one is declared in the header, and the other way round
    declared = set(re.findall(r"\b(nmpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    public = {s for s in exported if s.startswith("nmpc_") and not s.startswith(("nmpc_debug_", "nmpc_lidar_"))}
    assert public == declared, public ^ declared
    # the layout and the gradient of a stage are written down where the ABI is
    for word in ("ref [B][S][n_x]", "2 Q (X_k - xs_k)"):
        assert word in hdr, word


def test_python_surface_takes_a_reference():
    import inspect
    import nmpc_amd
    for f in ("eval_batch", "kkt_batch"):
        assert "reference" in inspect.signature(getattr(nmpc_amd.NmpcSolver, f)).parameters, f


def test_null_handle_is_an_argument_error_without_a_device(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert L.nmpc_eval_batch_ref(None, 1, None, None, None, 1, None, 0, None, None, None) == -1
    assert L.nmpc_kkt_batch_ref(None, 1, None, None, 1, None, 0, None, None, None, None, None, None) == -1


def _random_w(cfg, rng):
    lbx, ubx, _, _ = R.bounds(cfg)
    return rng.uniform(np.maximum(lbx, -2.0), np.minimum(ubx, 2.0))


@pytest.mark.parametrize("cfg", [R.cfg_one(5), R.cfg_six(4), R.cfg_obs3(7)], ids=["one", "six", "obs3"])
def test_constant_path_is_the_goal_cost_exactly(cfg):
    rng = np.random.default_rng(11)
    for _ in range(3):
        w = _random_w(cfg, rng)
        p = rng.uniform(-2.0, 2.0, 2 * cfg.nx)
        xs = p[cfg.nx:]
        for ref in (xs, np.tile(xs, (cfg.N, 1))):
            assert TR.objective(cfg, w, ref) == R.objective(cfg, w, p)
            assert np.array_equal(TR.grad_objective(cfg, w, ref), R.grad_objective(cfg, w, p))


@pytest.mark.parametrize("cfg", [R.cfg_one(5), R.cfg_six(4)], ids=["one", "six"])
def test_gradient_matches_central_differences_for_a_moving_path(cfg):
    rng = np.random.default_rng(12)
    w = _random_w(cfg, rng)
    ref = TR.line_path(cfg, rng.uniform(-1.0, 1.0, cfg.nx), rng.uniform(-0.2, 0.2, cfg.nx), cfg.N)
    assert np.ptp(ref, axis=0).min() > 0.0      # every component moves
    g = TR.grad_objective(cfg, w, ref)
    h = 1e-5      # the cost is quadratic: central differences are exact up to rounding, ~1e-16 |f| / h
    fd = np.empty_like(g)
    for j in range(w.size):
        e = np.zeros_like(w); e[j] = h
        fd[j] = (TR.objective(cfg, w + e, ref) - TR.objective(cfg, w - e, ref)) / (2 * h)
    assert np.max(np.abs(fd - g)) <= 1e-7, np.max(np.abs(fd - g))
    # and the path matters: the gradient of the path frozen at its row 0 is another one
    assert np.max(np.abs(g - TR.grad_objective(cfg, w, ref[0]))) > 1e-3


def test_fixtures_load_and_pass_their_own_kkt_screen():
    from tests.golden import gen_tracking_cases as G
    z = np.load(GOLDEN)
    fams = TR.families()
    assert set(z.files) == {n + s for n in fams for s in ("_p", "_ref", "_w0", "_w", "_f", "_w_pol", "_f_pol")}
    moved = 0.0
    for name, cfg in fams.items():
        P, REF, W0 = TR.family_inputs(name, cfg)      # the stored inputs are the generator's
        assert np.array_equal(z[name + "_p"], P, equal_nan=True) and np.array_equal(z[name + "_ref"], REF) and np.array_equal(z[name + "_w0"], W0)
        assert np.isnan(P[:, cfg.nx:]).all() and REF.shape == (3, cfg.N, cfg.nx)
        for p, ref, w, f in zip(P, REF, z[name + "_w_pol"], z[name + "_f_pol"]):
            assert abs(TR.objective(cfg, w, ref) - f) <= 1e-12 * max(1.0, abs(f))
            k = TR.kkt_report(cfg, w, p, ref)
            assert G.passes(k), (name, k)
            # a tracking problem: the frozen path has another cost at the stored point
            assert abs(TR.objective(cfg, w, ref[0]) - f) > 1e-6
        moved = max(moved, float(np.max(np.abs(z[name + "_w"] - z[name + "_w_pol"]))))
    assert moved <= 1e-6, moved      # the polish is a convergence witness
