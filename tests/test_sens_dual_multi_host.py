"""CPU: nmpc_sens_update_batch_multi_duals (csrc/nmpc_sens_dual_multi.hip) as far as it can be held without a GPU.

  - the entry point is declared with its twenty arguments, exported, in nmpc_amd._lib.EXPORTS and bound; a NULL handle is an argument error
    without a device; the Python names exist;
  - the built gfx950 code object has the twenty instantiations of dual_dirs_kernel<MS>, team sizes 1 .. 10 with and without the per-instance
    field, none with scratch, none with more than 64 KB of LDS; their registers and LDS are printed (DESIGN.md section 5 quotes them);
  - the inputs of tests/test_gpu_sens_dual_multi.py hold on the numpy reference alone: every (row, point, direction) of
    tests/sens_dual_multi_ref.py has info 0, 0 < alpha_dual <= 1, max|dlam_g| > 0 and max|dlam_x| > 0 (all 600; none replaced), and two
    exchanged directions of a point are at least 1000 parity bounds apart in the measure of tests/sens_dual_ref.parity — so a kernel that returns
    direction a in a slot of direction b misses the parity check by that factor;
  - AdvancedStepController.correct_scenarios(update_duals=True) and commit_scenario on a stub solver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sens_dual_multi_ref as DM
from tests import sens_dual_ref as DR
from tests import sens_points as SP
from tests.test_sens_multi_host import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
NAME = "nmpc_sens_update_batch_multi_duals"
ARGS = ["h", "B", "D", "p", "obs", "obs_stages", "w", "lam_g", "lam_x", "dp", "dobs", "rhs", "dw", "alpha", "dlam_g", "dlam_x", "dlam_p", "alpha_dual",
        "info", "stream"]


def test_entry_point_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m, NAME + " is not declared in include/nmpc.h"
    args = [a.strip().split("*")[-1].split()[-1] for a in m.group(1).split(",")]
    assert args == ARGS, args
    multi = re.search(r"int32_t\s+nmpc_sens_update_batch_multi\s*\(([^;]*)\)\s*;", hdr)
    assert [a.split()[-1] for a in m.group(1).split(",")[:14]] == [a.split()[-1] for a in multi.group(1).split(",")[:14]]      # the multi call's, then four more
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert NAME in nmpc_amd._lib.EXPORTS
    L = nmpc_amd._lib.load()
    f = getattr(L, NAME)
    assert len(f.argtypes) == 20 and f.restype is C.c_int32
    assert [t is C.c_int32 for t in f.argtypes] == [n in ("B", "D", "obs_stages") for n in ARGS]
    assert not re.search(r"#define NMPC_QUERY_[A-Z_]+ ([7-9]|\d\d)", hdr)      # no new query
    for gone in ("Multiplier updates for many directions are not provided", "The multiplier of p is not\n * updated here"):
        assert gone not in hdr


def test_null_handle_is_an_argument_error_without_a_device(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert getattr(L, NAME)(*([None, 1, 1] + [None] * 2 + [0] + [None] * 14)) == -1


def test_python_names_exist(built):
    import inspect
    import nmpc_amd
    assert "want_duals" in inspect.signature(nmpc_amd.NmpcSolver.sens_update_multi).parameters
    assert "want_duals" in inspect.signature(nmpc_amd.NmpcSolver.plan_jacobian).parameters
    assert "update_duals" in inspect.signature(nmpc_amd.AdvancedStepController.correct_scenarios).parameters
    assert hasattr(nmpc_amd.AdvancedStepController, "commit_scenario")


def test_code_object_has_the_twenty_instantiations_without_scratch_within_64_kb_of_lds(built, tmp_path):
    got = {}
    for name, note in _kernel_notes(tmp_path, "dual_dirs_kernel").items():
        m = re.search(r"^_ZN4nmpc16dual_dirs_kernelILi(\d+)EEE", name)
        assert m, "a kernel of that name with an unknown template signature: " + name
        assert "sens_dual" not in name and "plan_dirs_kernel" not in name
        ms = int(m.group(1))
        got[(ms // 16, ms % 16)] = note
    for (f, m), note in sorted(got.items()):
        print("dual_dirs_kernel m = %2d field %d: %3d registers, %5d bytes of LDS" % (m, f, note["vgpr_count"], note["group_segment_fixed_size"]))
    assert set(got) == {(f, m) for f in (0, 1) for m in range(1, 11)}, sorted(got)
    for key, note in got.items():
        assert note["private_segment_fixed_size"] == 0, (key, note)
        assert note["group_segment_fixed_size"] <= 65536, (key, note)


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_inputs_hold_on_the_reference_alone(i):
    r = ROWS[i]
    assert not DM.RESEED
    least, below_one = np.inf, 0
    for n in range(SP.NPOINTS):
        ref = DM.reference(r, n)
        assert len(ref) == DM.NDIRS
        for d, a in enumerate(ref):
            assert a["info"] == 0 and 0.0 < a["alpha_dual"] <= 1.0, (n, d, a["info"], a["alpha_dual"])
            assert np.abs(a["dlam_g"]).max() > 0.0 and np.abs(a["dlam_x"]).max() > 0.0, (n, d)
            below_one += a["alpha_dual"] < 1.0
        for a in range(DM.NDIRS):
            for b in range(a + 1, DM.NDIRS):
                # the reference's directions a and b exchanged: what the parity check of either slot would see, in units of its bound
                gap = min(DR.parity(r.cfg, ref[b]["dlam_g"], ref[b]["dlam_x"], ref[a], ref[a]["bd"])["worst"],
                          DR.parity(r.cfg, ref[a]["dlam_g"], ref[a]["dlam_x"], ref[b], ref[b]["bd"])["worst"])
                least = min(least, gap)
                assert gap >= 1000.0, (n, a, b, gap)
    print("%s: an exchanged pair of directions is at least %.1e bounds away; alpha_dual < 1 on %d of %d directions" % (
        SP.row_id(r), least, below_one, SP.NPOINTS * DM.NDIRS))


def test_dlam_p_of_the_reference_is_the_formula():
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); cfg = r.cfg
    ref = DM.reference(r, 1)[2]
    dp = DM.MR.directions(r, 1)[2][0]
    dX = ref["dw"][: (cfg.N + 1) * cfg.nx].reshape(cfg.N + 1, cfg.nx)
    want = np.array([2.0 * cfg.q[e % 3] * (sum(dX[k, e] for k in range(cfg.N)) - cfg.N * dp[cfg.nx + e]) for e in range(cfg.nx)])
    assert np.array_equal(ref["dlam_p"][: cfg.nx], ref["dlam_g"][: cfg.nx])
    assert (np.abs(ref["dlam_p"][cfg.nx:] - want) <= DM.dlam_p_tol(cfg, ref["dw"], dp)).all() and np.abs(want).max() > 0.0


# ---- the controller on a stub solver
class _Cfg:
    nx, nu, N = 3, 2, 2


class _Stub:
    """what AdvancedStepController uses of NmpcSolver, on CPU tensors: solve_batch returns a canned point, sens_update_multi canned steps for
    D = 3 scenarios (sens_update_batch the steps of one scenario, chosen by .scenario) and both record their arguments"""

    def __init__(self, B=4, D=3):
        import torch
        self.torch, self.device, self.cfg, self.B, self.D = torch, torch.device("cpu"), _Cfg, B, D
        self.n_p, self.n_var, self.n_g = 6, 13, 9
        g = torch.Generator().manual_seed(5)
        rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) - 0.5
        self.point = dict(x=rnd(B, 13), lam_g=rnd(B, 9), lam_x=rnd(B, 13), status=torch.tensor([0, 0, 2, 0], dtype=torch.int32),
                          iters=torch.zeros(B, dtype=torch.int32), kkt=torch.zeros(B, dtype=torch.float64), f=torch.zeros(B, dtype=torch.float64))
        self.step = dict(dw=rnd(B, D, 13), dlam_g=rnd(B, D, 9), dlam_x=rnd(B, D, 13),
                         alpha=torch.tensor([[1.0, 0.5, 1.0], [1.0, 1.0, 0.5], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], dtype=torch.float64),
                         alpha_dual=torch.tensor([[1.0, 1.0, 0.25], [0.25, 1.0, 0.75], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], dtype=torch.float64),
                         info=torch.tensor([0, 0, 0, 1], dtype=torch.int32))
        self.calls = []
        self.scenario = 0

    def duals_supported(self):
        return True

    def _dev(self, a, shape):
        return self.torch.as_tensor(a, dtype=self.torch.float64).reshape(shape)

    def solve_batch(self, p, w0, obstacles=None, want_duals=False, **kw):
        assert want_duals
        return dict(self.point)

    def _record(self, name, p, w, lam_g, lam_x, dp, dobs, obstacles, want_duals):
        self.calls.append(dict(name=name, p=p.clone(), w=w.clone(), lam_g=lam_g.clone(), lam_x=lam_x.clone(), dp=dp.clone(),
                               dobs=None if dobs is None else dobs.clone(), obstacles=None if obstacles is None else obstacles.clone(), want_duals=want_duals))

    def sens_update_multi(self, p, w, lam_g, lam_x, dp=None, dobs=None, rhs=None, obstacles=None, want_alpha=True, want_duals=False):
        self._record("multi", p, w, lam_g, lam_x, dp, dobs, obstacles, want_duals)
        keys = ("dw", "alpha", "info") + (("dlam_g", "dlam_x", "alpha_dual") if want_duals else ())
        return {k: self.step[k] for k in keys}

    def sens_update_batch(self, p, w, lam_g, lam_x, dp=None, dobs=None, rhs=None, obstacles=None, want_alpha=True, want_duals=False):
        self._record("single", p, w, lam_g, lam_x, dp, dobs, obstacles, want_duals)
        keys = ("dw", "alpha", "dlam_g", "dlam_x", "alpha_dual") if want_duals else ("dw", "alpha")
        out = {k: self.step[k][:, self.scenario] for k in keys}
        out["info"] = self.step["info"]
        return out


def _prepared(tau=0.9):
    import torch
    import nmpc_amd
    s = _Stub()
    ctl = nmpc_amd.AdvancedStepController(s, tau=tau)
    g = torch.Generator().manual_seed(7)
    p = torch.rand(4, 6, generator=g, dtype=torch.float64); obs = torch.rand(4, 2, 1, 3, generator=g, dtype=torch.float64)
    ctl.prepare(p, torch.zeros(4, 13, dtype=torch.float64), obstacles=obs)
    x0c = p[:, None, :3] + 0.01 * torch.arange(1, 4, dtype=torch.float64)[None, :, None]
    obc = obs[:, None] + 0.02 * torch.arange(1, 4, dtype=torch.float64)[None, :, None, None, None]
    return s, ctl, p, obs, x0c, obc


def test_scenarios_flag_off_is_todays_dict(built):
    import torch
    s, ctl, p, obs, x0c, obc = _prepared()
    out = ctl.correct_scenarios(x0c, obstacles=obc)
    assert set(out) == {"w", "u0", "step", "alpha", "info", "corrected"} and s.calls[-1]["want_duals"] is False
    step = torch.where(s.step["alpha"] == 1.0, s.step["alpha"], 0.9 * s.step["alpha"])
    ok = (s.step["info"] == 0) & (s.point["status"] == 0)
    w = torch.where(ok[:, None, None], s.point["x"][:, None] + step[:, :, None] * s.step["dw"], s.point["x"][:, None].expand(4, 3, 13))
    assert torch.equal(out["w"].view(torch.int64), w.contiguous().view(torch.int64)) and torch.equal(out["step"], step) and torch.equal(out["corrected"], ok)
    with pytest.raises(RuntimeError):
        ctl.commit_scenario(0)      # no dual-updating correct_scenarios before it


def test_scenarios_step_rule_and_multipliers(built):
    import torch
    s, ctl, p, obs, x0c, obc = _prepared()
    plan = ctl._plan
    out = ctl.correct_scenarios(x0c, obstacles=obc, update_duals=True)
    assert s.calls[-1]["want_duals"] is True and s.calls[-1]["name"] == "multi"
    assert set(out) == {"w", "u0", "step", "alpha", "info", "corrected", "lam_g", "lam_x", "alpha_dual"}
    want = torch.tensor([[1.0, 0.45, 0.9 * 0.25], [0.9 * 0.25, 1.0, 0.45], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    assert torch.equal(out["step"], want)      # min(primal, 1 if alpha_dual == 1 else tau alpha_dual)
    ok = out["corrected"]
    assert ok.tolist() == [True, True, False, False] and ctl.last["uncorrected"] == 2
    for key, base, d in (("w", "x", "dw"), ("lam_g", "lam_g", "dlam_g"), ("lam_x", "lam_x", "dlam_x")):
        for b in range(4):
            for k in range(3):
                w = s.point[base][b] + want[b, k] * s.step[d][b, k] if ok[b] else s.point[base][b]
                assert torch.equal(out[key][b, k].view(torch.int64), w.view(torch.int64)), (key, b, k)
    assert torch.equal(out["alpha_dual"], s.step["alpha_dual"]) and ctl._plan is plan
    # the same scenario through correct(update_duals=True) gives the same step and the same bits
    for k in range(3):
        s.scenario = k
        one = ctl.correct(x0c[:, k], obstacles=obc[:, k], update_duals=True)
        assert torch.equal(one["step"], out["step"][:, k])
        for key in ("w", "lam_g", "lam_x"):
            assert torch.equal(one[key].view(torch.int64), out[key][:, k].contiguous().view(torch.int64)), (key, k)


@pytest.mark.parametrize("pick", ["int", "indices"])
def test_commit_scenario_leaves_what_correct_with_commit_leaves(built, pick):
    import torch
    s, ctl, p, obs, x0c, obc = _prepared()
    ctl.correct_scenarios(x0c, obstacles=obc, update_duals=True)
    idx = torch.tensor([1, 1, 1, 1]) if pick == "int" else torch.tensor([2, 0, 1, 2])
    ctl.commit_scenario(1 if pick == "int" else idx)
    got = ctl._plan
    # the same with correct(commit=True), instance by instance on a second controller
    s2, ctl2, p2, obs2, _, _ = _prepared()
    want = {k: (None if v is None else v.clone()) for k, v in ctl2._plan.items()}
    for k in sorted(set(idx.tolist())):
        s3, ctl3, _, _, _, _ = _prepared()
        s3.scenario = k
        ctl3.correct(x0c[:, k], obstacles=obc[:, k], commit=True)
        rows = idx == k
        for key in ("p", "w", "lam_g", "lam_x", "obstacles"):
            want[key][rows] = ctl3._plan[key][rows]
    for key in ("p", "w", "lam_g", "lam_x", "obstacles", "status"):
        assert torch.equal(got[key].contiguous().view(torch.int64) if got[key].dtype == torch.float64 else got[key], want[key].view(torch.int64) if want[key].dtype == torch.float64 else want[key]), key
    # the uncorrected instances keep the prepared base
    for b in (2, 3):
        assert torch.equal(got["p"][b], p[b]) and torch.equal(got["w"][b], s.point["x"][b]) and torch.equal(got["obstacles"][b], obs[b])
    with pytest.raises(RuntimeError):
        ctl.commit_scenario(0)      # one commit per correct_scenarios: the scenarios were taken relative to the old base
    ctl2.correct_scenarios(x0c, obstacles=obc, update_duals=True)
    with pytest.raises(ValueError):
        ctl2.commit_scenario(3)      # D = 3 scenarios
