"""CPU: the multiplier updates of the forward plan update (nmpc_sens_update_batch_duals) are declared, exported and bound, their kernel has one
instantiation per row of tests/sens_points.SENS_TABLE, and the numpy reference the GPU tests hold it against (tests/sens_dual_ref.py) is right on
its own: the stage walk is the lower block of one bordered dense solve, stationarity (a) of include/nmpc.h holds with oracle.nlp_ref's exact
Hessian and Jacobian and central differences of grad_lag — nothing of the W restatement in it —, every term class is visible in dlam at 1000 x the
parity bound, and the structural zeros are exact.  Then AdvancedStepController's update_duals / commit on a stub solver.

The parity bound is the project's: 100 x the spread of the reference against itself under +-4 ulp moves of (w, lam_g, lam_x), + 1e-12, relative to
max|dlam_g|, max|dlam_x| (to alpha_dual) — and, with the spread taken the same way, per stage block of dlam_g and dlam_x relative to the block's
own maximum (tests/sens_dual_ref.stage_blocks), which the dense solve and the kernel are held to as well.  The identity's bound is measured the same way — the residual of (a) at the unmoved point with the moved
point's (dw, dlam), x 100, + 1e-12 — plus 1e-10 for the rounding of the central differences (tests/sens_dual_ref.FD_TOL), relative to the largest
term of (a).  Recorded over the table (stage walk and dense solve): the identity's residual is at most 1.9e-12 of its largest term, the bound 1.0e-10 or more."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as Hh
from tests import sens_dual_ref as DR
from tests import sens_points as SP
from tests import sens_update_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
VISIBLE = 1000.0
NARGS = 18


# ---- H1: the symbols
def test_entry_point_declared_exported_and_bound(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    m = re.search(r"int32_t\s+nmpc_sens_update_batch_duals\s*\(([^;]*)\)\s*;", hdr)
    assert m, "nmpc_sens_update_batch_duals is not declared in include/nmpc.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == NARGS and [a.split("*")[-1].strip() for a in args[13:16]] == ["dlam_g", "dlam_x", "alpha_dual"] and args[16].endswith("info")
    plain = re.search(r"int32_t\s+nmpc_sens_update_batch\s*\(([^;]*)\)\s*;", hdr)
    assert [a.split()[-1] for a in args[:13]] == [a.split()[-1] for a in plain.group(1).split(",")[:13]]      # the arguments of the plain call, then three more
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    assert "nmpc_sens_update_batch_duals" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = nmpc_amd._lib.load()
    assert "nmpc_sens_update_batch_duals" in nmpc_amd._lib.EXPORTS
    assert len(L.nmpc_sens_update_batch_duals.argtypes) == NARGS and L.nmpc_sens_update_batch_duals.restype is C.c_int32
    for word in ("dlam_g,i = Sigma_i ds_i", "dlam_x,j = beta_j dw_j", "dnu_{k-1} = A_k' dnu_k - r_Xk", "min(1, min_i z_i / (-dz_i))"):
        assert word in hdr, word


def test_null_handle_is_an_argument_error_without_a_device(built):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    assert L.nmpc_sens_update_batch_duals(*([None, 1] + [None] * 2 + [0] + [None] * 13)) == -1


def test_table_equals_the_dual_kernels_of_the_code_object(built, tmp_path):
    got = []
    for name in Hh.kernel_notes(tmp_path):
        m = re.search(r"^_ZN4nmpc16sens_dual_kernelILi(\d+)EEE", name)
        if m:
            ms = int(m.group(1))
            got.append((ms % 16, ms // 16))
            continue
        assert "sens_dual" not in name, "multiplier-update kernel with an unknown template signature: " + name
    rows = [(r.m, r.field) for r in ROWS]
    assert len(got) == len(set(got)) == 20, sorted(got)
    assert set(got) == set(rows), (sorted(set(got) - set(rows)), sorted(set(rows) - set(got)))


# ---- H2: the reference
def _args(r, pt):
    return (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)


@functools.lru_cache(maxsize=None)
def screened(i):
    """per point of row i: the inputs, the stage walk, the dense solve, the spreads and the bounds"""
    r = ROWS[i]
    out = []
    for n, pt in enumerate(SP.points(r)):
        kw = dict(dp=pt.dp, dobs=UR.row_dobs(r, n), rhs=UR.row_rhs(r, n))
        sp = DR.spread(*_args(r, pt), **kw)
        out.append(dict(pt=pt, kw=kw, ref=DR.stage_duals(*_args(r, pt), **kw), dense=DR.dense_duals(*_args(r, pt), **kw), sp=sp, bd=DR.bounds(sp)))
    return out


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_stage_walk_is_the_dense_solve(i):
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        ref, de, bd = o["ref"], o["dense"], o["bd"]
        e = DR.parity(r.cfg, ref["dlam_g"], ref["dlam_x"], de, bd)
        eg, ex = e["g"], e["x"]
        ea = abs(ref["alpha_dual"] - de["alpha_dual"]) / de["alpha_dual"]
        print("%s %d: dlam_g %.2e (bound %.2e), dlam_x %.2e (%.2e), alpha_dual %.6g: %.2e (%.2e); max|dlam_g| %.2e, max|dlam_x| %.2e; worst measure, stage blocks included, %.3f of its bound" % (
            SP.row_id(r), n, eg, bd["g"], ex, bd["x"], ref["alpha_dual"], ea, bd["a"], np.abs(ref["dlam_g"]).max(), np.abs(ref["dlam_x"]).max(), e["worst"]))
        assert ref["info"] == 0 and 0.0 < ref["alpha_dual"] <= 1.0
        assert eg <= bd["g"] and ex <= bd["x"] and ea <= bd["a"], (n, eg, ex, ea, bd)
        assert e["worst"] <= 1.0, (n, e, bd)
        assert UR.rel(ref["dw"], de["dw"]) <= 100.0 * UR.spread(*_args(r, o["pt"]), **o["kw"])[0] + 1e-12


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_stationarity_holds_with_the_exact_hessian_and_jacobian(i):
    """identity (a), for the stage walk and for the dense solve"""
    r = ROWS[i]
    for n, o in enumerate(screened(i)):
        for name in ("ref", "dense"):
            d = o[name]
            res, scale = DR.identity(*_args(r, o["pt"]), d["dw"], d["dlam_g"], d["dlam_x"], **o["kw"])
            print("%s %d %-5s: residual of (a) %.2e of its largest term %.2e (bound %.2e)" % (SP.row_id(r), n, name, res / scale, scale, o["bd"]["ident"]))
            assert res <= o["bd"]["ident"] * scale, (n, name, res / scale, o["bd"]["ident"])


def test_nothing_to_do_is_alpha_dual_one_and_no_change():
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3)
    pt = SP.points(r)[0]
    z = DR.stage_duals(*_args(r, pt), dp=np.zeros(2 * r.cfg.nx), dobs=np.zeros_like(pt.obs), rhs=np.zeros(r.cfg.n_var))
    assert z["info"] == 0 and z["alpha_dual"] == 1.0 and not z["dlam_g"].any() and not z["dlam_x"].any()


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_zero_everything(r):
    kw = dict(dobs=UR.row_dobs(r, 0), rhs=UR.row_rhs(r, 0))
    for name, pt, want in SP.verdict_cases(r, SP.points(r)[0]):
        a = DR.stage_duals(*_args(r, pt), dp=pt.dp, **kw)
        assert a["info"] == want, (name, a["info"], want)
        if want:
            assert not a["dlam_g"].any() and not a["dlam_x"].any() and a["alpha_dual"] == 0.0, name
        else:
            assert a["dlam_g"].any() and a["dlam_x"].any() and a["alpha_dual"] > 0.0, name


# ---- H3: every term is visible, the structural zeros are exact
def _moved(i, change):
    """per point of row i: how far dlam of the changed point lies from the point's own, in units of the point's parity bound (the larger of the
    two outputs)"""
    r = ROWS[i]
    f = []
    for o in screened(i):
        b = DR.stage_duals(*_args(r, change(o["pt"])), **o["kw"])
        assert b["info"] == 0
        f.append(DR.parity(r.cfg, b["dlam_g"], b["dlam_x"], o["ref"], o["bd"])["worst"])
    return sorted(f)


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_every_term_class_is_visible_in_dlam(i):
    """a reference without the multipliers of one term class is 1000 x the point's parity bound or more away in dlam on at least two points of
    the row, in the measure the parity tests hold the kernel to (tests/sens_dual_ref.parity): dlam_g or dlam_x relative to its maximum, or one
    stage block of either relative to the block's own.  The stage blocks matter: the walk runs backward and adds up, so max|dlam| sits in the
    first stages, and against it alone the defects' curvature on m3_moving_field shows at 27, 64, 135, 278 and 7415 x the bound on the row's five
    points; against the stages' own maxima at 1.9e3 .. 1.2e8 x.  Smallest second-best factor of the table: 2.9e5 (m1_moving_field, defect)."""
    r = ROWS[i]
    low = []
    for cls in SP.classes_of(r.cfg):
        f = _moved(i, lambda pt: SP.zero_class(r.cfg, pt, cls))
        print("%s %-8s: factors %s" % (SP.row_id(r), cls, " ".join("%.1e" % v for v in f)))
        if f[-2] < VISIBLE:
            low.append((cls, f))
    assert not low, low


@pytest.mark.parametrize("i", [i for i, r in enumerate(ROWS) if r.cfg.M > 1], ids=[IDS[i] for i, r in enumerate(ROWS) if r.cfg.M > 1])
def test_a_wrong_pair_index_is_visible_in_dlam(i):
    r = ROWS[i]
    f = _moved(i, lambda pt: SP.reverse_pairs(r.cfg, pt))
    print("%s: factors %s" % (SP.row_id(r), " ".join("%.1e" % v for v in f)))
    assert f[-2] >= VISIBLE, f


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_structural_zeros_are_exact_and_carry_nothing(i):
    """dlam is exactly 0.0 on the entries of SP.null_masks — but for the initial block, whose dlam_g is dnu_init of (e) — and on the rows and
    bounds without a multiplier; what the inputs hold on the masked entries changes no bit of the outputs"""
    r = ROWS[i]; cfg = r.cfg
    mg, mx = SP.null_masks(cfg)
    mg = mg.copy(); mg[: cfg.nx] = False
    for o in screened(i):
        ref, pt = o["ref"], o["pt"]
        assert not ref["dlam_g"][mg].any() and not ref["dlam_x"][mx].any()
        assert ref["dlam_g"][: cfg.nx].any()
        rows = DR.S.ineq_rows(cfg)
        assert not ref["dlam_g"][rows][pt.lam_g[rows] >= 0.0].any() and not ref["dlam_x"][pt.lam_x == 0.0].any()
        assert not np.signbit(ref["dlam_g"][ref["dlam_g"] == 0.0]).any() and not np.signbit(ref["dlam_x"][ref["dlam_x"] == 0.0]).any()
        z = DR.stage_duals(*_args(r, SP.zero_nulls(cfg, pt)), **o["kw"])
        for key in ("dw", "dlam_g", "dlam_x"):
            assert np.array_equal(z[key].view(np.int64), ref[key].view(np.int64)), key
        assert z["alpha_dual"] == ref["alpha_dual"]


def test_alpha_dual_keeps_every_sign_and_is_tight():
    for i in (2, 12, 19):
        r = ROWS[i]
        for o in screened(i):
            ref, pt = o["ref"], o["pt"]
            z, dz = DR.dual_items(r.cfg, pt.lam_g, pt.lam_x, ref["dlam_g"], ref["dlam_x"])
            m = (z > 0.0) & (dz < 0.0)
            al = ref["alpha_dual"]
            left = z[m] + al * dz[m]
            assert (left >= -4.0 * np.finfo(float).eps * z[m]).all()
            if al < 1.0:
                assert abs(left[int(np.argmin(z[m] / -dz[m]))]) <= o["bd"]["a"] * z[m][int(np.argmin(z[m] / -dz[m]))]


# ---- H4: the controller's flags on a stub solver
class _Cfg:
    nx, nu, N = 3, 2, 2


class _Stub:
    """what AdvancedStepController uses of NmpcSolver, on CPU tensors: solve_batch returns a canned point, sens_update_batch canned steps and
    records its arguments"""

    def __init__(self, B=4):
        import torch
        self.torch, self.device, self.cfg, self.B = torch, torch.device("cpu"), _Cfg, B
        self.n_p, self.n_var, self.n_g = 6, 13, 9
        g = torch.Generator().manual_seed(5)
        rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) - 0.5
        self.point = dict(x=rnd(B, 13), lam_g=rnd(B, 9), lam_x=rnd(B, 13), status=torch.tensor([0, 0, 0, 0][:B], dtype=torch.int32),
                          iters=torch.zeros(B, dtype=torch.int32), kkt=torch.zeros(B, dtype=torch.float64), f=torch.zeros(B, dtype=torch.float64))
        self.step = dict(dw=rnd(B, 13), dlam_g=rnd(B, 9), dlam_x=rnd(B, 13), alpha=torch.tensor([1.0, 0.5, 1.0, 1.0], dtype=torch.float64),
                         alpha_dual=torch.tensor([1.0, 1.0, 0.25, 1.0], dtype=torch.float64), info=torch.tensor([0, 0, 0, 1], dtype=torch.int32))
        self.calls = []

    def duals_supported(self):
        return True

    def _dev(self, a, shape):
        return self.torch.as_tensor(a, dtype=self.torch.float64).reshape(shape)

    def solve_batch(self, p, w0, obstacles=None, want_duals=False, **kw):
        assert want_duals
        return dict(self.point)

    def sens_update_batch(self, p, w, lam_g, lam_x, dp=None, dobs=None, rhs=None, obstacles=None, want_alpha=True, want_duals=False):
        self.calls.append(dict(p=p.clone(), w=w.clone(), lam_g=lam_g.clone(), lam_x=lam_x.clone(), dp=dp.clone(), dobs=None if dobs is None else dobs.clone(),
                               obstacles=None if obstacles is None else obstacles.clone(), want_duals=want_duals))
        keys = ("dw", "alpha", "info") + (("dlam_g", "dlam_x", "alpha_dual") if want_duals else ())
        return {k: self.step[k] for k in keys}


def _prepared(tau=0.9):
    import torch
    import nmpc_amd
    s = _Stub()
    ctl = nmpc_amd.AdvancedStepController(s, tau=tau)
    g = torch.Generator().manual_seed(7)
    p = torch.rand(4, 6, generator=g, dtype=torch.float64); obs = torch.rand(4, 2, 1, 3, generator=g, dtype=torch.float64)
    ctl.prepare(p, torch.zeros(4, 13, dtype=torch.float64), obstacles=obs)
    x0 = p[:, :3] + 0.01; ob2 = obs + 0.02
    return s, ctl, p, obs, x0, ob2


def test_controller_flags_off_is_todays_dict(built):
    import torch
    s, ctl, p, obs, x0, ob2 = _prepared()
    out = ctl.correct(x0, obstacles=ob2)
    assert set(out) == {"w", "u0", "step", "alpha", "info", "corrected"} and s.calls[-1]["want_duals"] is False
    step = torch.where(s.step["alpha"] == 1.0, s.step["alpha"], 0.9 * s.step["alpha"])
    ok = s.step["info"] == 0
    w = torch.where(ok[:, None], s.point["x"] + step[:, None] * s.step["dw"], s.point["x"])
    assert torch.equal(out["w"].view(torch.int64), w.view(torch.int64)) and torch.equal(out["step"], step) and torch.equal(out["corrected"], ok)
    assert torch.equal(out["u0"], w[:, 9:11]) and ctl.last["uncorrected"] == 1


def test_controller_step_rule_with_duals(built):
    import torch
    s, ctl, p, obs, x0, ob2 = _prepared()
    plan = ctl._plan
    out = ctl.correct(x0, obstacles=ob2, update_duals=True)
    assert s.calls[-1]["want_duals"] is True
    assert torch.equal(out["step"], torch.tensor([1.0, 0.9 * 0.5, 0.9 * 0.25, 1.0], dtype=torch.float64))      # min(primal, 1 if alpha_dual == 1 else tau alpha_dual)
    st, ok = out["step"][:, None], (s.step["info"] == 0)[:, None]
    for key, base, d in (("w", "x", "dw"), ("lam_g", "lam_g", "dlam_g"), ("lam_x", "lam_x", "dlam_x")):
        want = torch.where(ok, s.point[base] + st * s.step[d], s.point[base])
        assert torch.equal(out[key].view(torch.int64), want.view(torch.int64)), key
    assert torch.equal(out["lam_g"][3], s.point["lam_g"][3]) and torch.equal(out["lam_x"][3], s.point["lam_x"][3])      # not corrected: the prepared multipliers
    assert torch.equal(out["alpha_dual"], s.step["alpha_dual"])
    assert ctl._plan is plan      # commit=False leaves the base as it is


def test_controller_commit_moves_the_base_of_the_corrected_instances(built):
    import torch
    s, ctl, p, obs, x0, ob2 = _prepared()
    out = ctl.correct(x0, obstacles=ob2, commit=True)
    assert s.calls[-1]["want_duals"] is True and "lam_g" in out      # commit implies update_duals
    st, ok = out["step"], out["corrected"]
    first = s.calls[-1]
    x1 = p[:, :3] + 0.03; ob3 = obs + 0.05
    ctl.correct(x1, obstacles=ob3)
    second = s.calls[-1]
    p_base = torch.where(ok[:, None], p + st[:, None] * first["dp"], p)
    o_base = torch.where(ok[:, None, None, None], obs + st[:, None, None, None] * first["dobs"], obs)
    assert torch.equal(second["p"], p_base) and torch.equal(second["obstacles"], o_base)
    assert torch.equal(second["w"], out["w"]) and torch.equal(second["lam_g"], out["lam_g"]) and torch.equal(second["lam_x"], out["lam_x"])
    assert torch.equal(second["dp"][:, :3], x1 - p_base[:, :3]) and not second["dp"][:, 3:].any()
    assert torch.equal(second["dobs"], ob3 - o_base)
    # the uncorrected instance keeps the prepared base
    assert torch.equal(second["p"][3], p[3]) and torch.equal(second["w"][3], s.point["x"][3]) and torch.equal(second["obstacles"][3], obs[3])
    # a full step lands on the measured parameters within rounding, a limited one part of the way
    assert torch.allclose(second["p"][0, :3], x0[0], rtol=0, atol=1e-15) and torch.allclose(second["p"][1, :3], p[1, :3] + 0.45 * 0.01, rtol=0, atol=1e-15)


# ---- the screens of the end-to-end GPU checks (tests/golden/sens_update_cases.npz), on the reference alone
@pytest.mark.parametrize("name", list(UR.load_cases()))
def test_the_fixtures_pass_the_certificate_and_chain_screens(name):
    """at least 3 of 4 instances per configuration have a certificate ratio r(h) / r(h/2) in [3.5, 4.5] with the updated multipliers — second
    order, where the old multipliers leave a first-order residual — and a chained correction (h / 2, commit, h) that is closer to the oracle's
    re-solve than the single one.  Recorded: ratios 4.000 .. 4.145 on the kept ones (two_static 0: 4.704, dropped), r(h) 23 .. 919 times
    smaller than with the old multipliers; chained |w - w(h)| 0.49 .. 0.52 of the single correction's on all twelve."""
    c = UR.load_cases()[name]
    cert = [DR.screen_certificate(c, b) for b in range(4)]
    chain = [DR.screen_chain(c, b) for b in range(4)]
    for b in range(4):
        print("%s %d: r(h) %.2e r(h/2) %.2e ratio %.3f, old multipliers %.2e (x %.1f)%s; single %.2e chained %.2e%s" % (
            name, b, cert[b]["r_h"], cert[b]["r_h2"], cert[b]["ratio"], cert[b]["r_old"], cert[b]["r_old"] / cert[b]["r_h"], "" if cert[b]["keep"] else " dropped",
            chain[b]["single"], chain[b]["chained"], "" if chain[b]["keep"] else " dropped"))
    assert sum(x["keep"] for x in cert) >= 3 and sum(x["keep"] for x in chain) >= 3
    for x in cert:
        if x["keep"]:
            assert x["r_h"] < x["r_old"]
