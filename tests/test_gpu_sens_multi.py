"""-m gpu: nmpc_sens_update_batch_multi (csrc/nmpc_sens_multi.hip), NmpcSolver.sens_update_multi / plan_jacobian and
AdvancedStepController.correct_scenarios.

Every instantiation of plan_dirs_kernel<MS> against tests/sens_update_ref.stage_update per direction (tests/sens_multi_ref.py) on the constructed
points of tests/sens_points.py.  With c = nmpc_query(NMPC_QUERY_SENS_DIRS_PER_PASS) the calls run at every distinct D of
{1, 2, c - 1, c, c + 1, min(2 c + 1, 64), 64}: the six distinct directions of a point stand round-robin in the D slots under a seeded permutation,
and every slot is held to the reference of its direction by the project's bound, 100 x that direction's spread + 1e-12 relative to max|dw| and
to alpha; two directions exchanged are at least 1000 bounds apart (tests/test_sens_multi_host.py).  Then the bit-level properties inside the
kernel, the agreement with nmpc_sens_update_batch, the verdict batches, the argument errors, the workspace, the Jacobian and its duality with
nmpc_sens_adjoint_batch, and the controller."""
import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import sens_adjoint_ref as AR
from tests import sens_multi_ref as MR
from tests import sens_points as SP
from tests import sens_update_ref as UR

pytestmark = pytest.mark.gpu

ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
_CACHE = {}
BIT_EQUAL = {}      # row id -> (dw entries bit-equal to nmpc_sens_update_batch, dw entries, alpha values bit-equal, alpha values)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _solver(cfg, max_batch, **kw):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=10, pair_rows=cfg.pair_rows), max_batch=max_batch, **kw)


def _product_solver(cfg, max_batch, **kw):
    import nmpc_amd
    solver_kw = {k: kw.pop(k) for k in ("kernel",) if k in kw}
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, pair_rows=cfg.pair_rows, **kw), max_batch=max_batch, **solver_kw)


def _point_arrays(r, pts):
    obs = np.stack([pt.obs for pt in pts]) if r.field else None      # an "own" row calls with (NULL, 0): the handle's field, no dobs
    return [np.stack([getattr(pt, k) for pt in pts]) for k in ("p", "w", "lam_g", "lam_x")], obs


def _call(s, r, pts, stacks, **kw):
    """stacks: per point (dp [D, n_p], dobs [D, ...] or None, rhs [D, n_var])"""
    a, obs = _point_arrays(r, pts)
    dobs = None if stacks[0][1] is None else np.stack([x[1] for x in stacks])
    out = s.sens_update_multi(*a, dp=np.stack([x[0] for x in stacks]), dobs=dobs, rhs=np.stack([x[2] for x in stacks]), obstacles=obs, **kw)
    return {k: _np(v) for k, v in out.items()}


def _slot_seed(r, D):
    return 100 * r.seed + D


def ran(i):
    """row i: its handle, the call at every D of the row's list on the row's points, and the stacked reference — once per session"""
    if i in _CACHE:
        return _CACHE[i]
    r = ROWS[i]
    pts = SP.points(r); n = len(pts)
    s = _solver(r.cfg, 2 * n + 20)
    c = s.sens_dirs_per_pass
    assert c == 64 - 5 * r.m
    calls = {}
    for D in MR.d_values(c):
        sl = MR.slots(D, _slot_seed(r, D))
        stacks = [MR.stack(r, k, sl) for k in range(n)]
        calls[D] = dict(slots=sl, stacks=stacks, out=_call(s, r, pts, stacks))
    ref = [MR.reference(r, k) for k in range(n)]
    _CACHE[i] = dict(row=r, pts=pts, n=n, solver=s, c=c, calls=calls, ref=ref)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_parity_of_every_slot_against_numpy(i):
    o = ran(i); r = o["row"]; cfg = r.cfg
    worst = (0.0, 0.0, 0.0, 0)
    for D, call in o["calls"].items():
        dw, alpha, info = call["out"]["dw"], call["out"]["alpha"], call["out"]["info"]
        assert dw.shape == (o["n"], D, cfg.n_var) and alpha.shape == (o["n"], D) and info.shape == (o["n"],)
        for b in range(o["n"]):
            assert info[b] == 0
            for slot, d in enumerate(call["slots"]):
                ref = o["ref"][b][d]
                bw, ba = MR.bound(ref)
                ew = UR.rel(dw[b, slot], ref["dw"]); ea = abs(alpha[b, slot] - ref["alpha"]) / ref["alpha"]
                worst = max(worst, (max(ew / bw, ea / ba), ew, ea, D))
                assert ref["info"] == 0 and ew <= bw and ea <= ba, (D, b, slot, d, ew, bw, ea, ba)
                assert 0.0 < alpha[b, slot] <= 1.0
    print("%s (c = %d, D in %s): largest error %.2e of its bound (dw %.2e, alpha %.2e, at D = %d)" % (
        SP.row_id(r), o["c"], sorted(o["calls"]), worst[0], worst[1], worst[2], worst[3]))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_same_bits_in_every_slot_and_d_reversed_repeated_and_without_alpha(i):
    o = ran(i); r = o["row"]
    first = {}      # (point, direction) -> bits of (dw, alpha) where the direction was first seen
    for D, call in o["calls"].items():
        out = call["out"]
        for b in range(o["n"]):
            for slot, d in enumerate(call["slots"]):
                got = (_bits(out["dw"][b, slot]), _bits(out["alpha"][b, slot: slot + 1]))
                want = first.setdefault((b, d), got)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (D, b, slot, d)
    call = o["calls"][64]; f = call["out"]
    back = _call(o["solver"], r, o["pts"][::-1], call["stacks"][::-1])
    again = _call(o["solver"], r, o["pts"], call["stacks"])
    assert np.array_equal(back["info"][::-1], f["info"]) and np.array_equal(again["info"], f["info"])
    for key in ("dw", "alpha"):
        assert np.array_equal(_bits(back[key][::-1]), _bits(f[key])), key
        assert np.array_equal(_bits(again[key]), _bits(f[key])), key
    only = _call(o["solver"], r, o["pts"], call["stacks"], want_alpha=False)
    assert only["alpha"] is None and np.array_equal(_bits(only["dw"]), _bits(f["dw"])) and np.array_equal(only["info"], f["info"])


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_agrees_with_the_single_direction_call(i):
    """direction 0 is the input of tests/test_gpu_sens_update.py: nmpc_sens_update_batch on it and the slot that holds it agree to the sum of the
    two bounds (both are held to the same reference); how many entries are bit-equal is printed, a record"""
    o = ran(i); r = o["row"]; s = o["solver"]; pts = o["pts"]
    a, obs = _point_arrays(r, pts)
    d0 = [MR.directions(r, k)[0] for k in range(o["n"])]
    single = s.sens_update_batch(*a, dp=np.stack([x[0] for x in d0]), dobs=None if d0[0][1] is None else np.stack([x[1] for x in d0]),
                                 rhs=np.stack([x[2] for x in d0]), obstacles=obs)
    sdw, sal = _np(single["dw"]), _np(single["alpha"])
    call = o["calls"][64]; slot = call["slots"].index(0)
    mdw, mal = call["out"]["dw"][:, slot], call["out"]["alpha"][:, slot]
    for b in range(o["n"]):
        bw, ba = MR.bound(o["ref"][b][0])
        ew = np.abs(mdw[b] - sdw[b]).max() / np.abs(o["ref"][b][0]["dw"]).max(); ea = abs(mal[b] - sal[b]) / o["ref"][b][0]["alpha"]
        assert ew <= 2.0 * bw and ea <= 2.0 * ba, (b, ew, bw, ea, ba)
    BIT_EQUAL[SP.row_id(r)] = (int((_bits(mdw) == _bits(sdw)).sum()), mdw.size, int((_bits(mal) == _bits(sal)).sum()), mal.size)
    print("%s: bit-equal to nmpc_sens_update_batch: %d of %d dw entries, %d of %d alpha values" % ((SP.row_id(r),) + BIT_EQUAL[SP.row_id(r)]))
    if len(BIT_EQUAL) == 20:
        t = np.array(list(BIT_EQUAL.values())).sum(axis=0)
        print("all rows: bit-equal to nmpc_sens_update_batch: %d of %d dw entries, %d of %d alpha values" % tuple(t))


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_in_a_mixed_batch(r):
    """each verdict case is one instance between clean points: all D slots of it are zeros, and its neighbours keep the bits of the parity call"""
    i = ROWS.index(r)
    o = ran(i); cfg = r.cfg
    D = o["c"] + 1      # two groups
    par = o["calls"][D]; sl = par["slots"]
    cases = SP.verdict_cases(r, o["pts"][0])[1:]
    batch, stacks, clean = [], [], []
    for c, (name, pt, want) in enumerate(cases):
        a = c % o["n"]; clean.append(a)
        batch += [o["pts"][a], pt]
        stacks += [par["stacks"][a], par["stacks"][0]]      # the case is point 0 moved: it takes point 0's directions
    s = _solver(cfg, len(batch))
    got = _call(s, r, batch, stacks)
    info = got["info"]
    dirs0 = MR.directions(r, 0)
    for c, (name, pt, want) in enumerate(cases):
        b = 2 * c + 1
        a = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        ref0 = UR.stage_update(*a, dp=dirs0[0][0], dobs=dirs0[0][1], rhs=dirs0[0][2])
        assert info[b] == ref0["info"] == want, (name, info[b], ref0["info"], want)
        if want:
            assert not got["dw"][b].any() and (got["alpha"][b] == 0.0).all() and got["alpha"][b].shape == (D,), name
        else:      # the pair row of the wrong sign: no Sigma, its Hessian term stays in
            for d in range(MR.NDIRS):
                ref = UR.stage_update(*a, dp=dirs0[d][0], dobs=dirs0[d][1], rhs=dirs0[d][2])
                sw, sa = UR.spread(*a, dp=dirs0[d][0], dobs=dirs0[d][1], rhs=dirs0[d][2])
                for slot in [k for k, x in enumerate(sl) if x == d]:
                    ew, ea = UR.rel(got["dw"][b, slot], ref["dw"]), abs(got["alpha"][b, slot] - ref["alpha"]) / ref["alpha"]
                    assert ew <= 100.0 * sw + 1e-12 and ea <= 100.0 * sa + 1e-12, (name, d, slot, ew, sw, ea, sa)
        a = clean[c]
        assert info[2 * c] == 0
        assert np.array_equal(_bits(got["dw"][2 * c]), _bits(par["out"]["dw"][a])) and np.array_equal(_bits(got["alpha"][2 * c]), _bits(par["out"]["alpha"][a])), name


def test_argument_errors_leave_the_outputs_as_they_were():
    import torch
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); o = ran(ROWS.index(r)); cfg = r.cfg; s = o["solver"]
    B, D = 2, 3
    d = s.device
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=d)
    p, w, lg, lx, dp, rh = t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_g), t(B, cfg.n_var), t(B, 65, 2 * cfg.nx), t(B, 65, cfg.n_var)
    ob, dob = t(B, cfg.N, cfg.K, 3), t(B, 65, cfg.N, cfg.K, 3)
    MARK, IMARK = 0x7FF4DEADBEEF0123, 0x5A5A5A5A
    dw = torch.full((B, 65, cfg.n_var), MARK, dtype=torch.int64, device=d)
    al = torch.full((B, 65), MARK, dtype=torch.int64, device=d)
    info = torch.full((B,), IMARK, dtype=torch.int32, device=d)
    ptr = lambda x: None if x is None else x.data_ptr()

    def raw(lib_s, B_, D_, p_, obs_, S_, w_, lg_, lx_, dp_, dob_, rh_, dw_, al_, info_):
        rc = lib_s.lib.nmpc_sens_update_batch_multi(lib_s._h, B_, D_, ptr(p_), ptr(obs_), S_, ptr(w_), ptr(lg_), ptr(lx_), ptr(dp_), ptr(dob_), ptr(rh_),
                                                    ptr(dw_), ptr(al_), ptr(info_), lib_s._stream())
        torch.cuda.synchronize()
        assert (dw == MARK).all() and (al == MARK).all() and (info == IMARK).all(), "an argument error wrote to an output"
        return rc
    ok = (p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, info)
    assert raw(s, B, 0, *ok) == -1                                                     # D = 0
    assert raw(s, B, 65, *ok) == -1                                                    # D beyond NMPC_SENS_MAX_DIRS
    assert raw(s, B, -1, *ok) == -1
    assert raw(s, B, D, p, ob, cfg.N, w, lg, lx, dp, dob, rh, None, al, info) == -1    # dw is required
    assert raw(s, B, D, p, None, 0, w, lg, lx, dp, dob, rh, dw, al, info) == -1        # dobs without obs
    assert raw(s, s.max_batch + 1, D, *ok) == -1
    for k in range(4):      # null p, w, lam_g, lam_x
        a = [p, w, lg, lx]; a[k] = None
        assert raw(s, B, D, a[0], ob, cfg.N, a[1], a[2], a[3], dp, dob, rh, dw, al, info) == -1, k
    assert raw(s, B, D, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, None) == -1
    assert raw(s, B, D, p, ob, 2, w, lg, lx, dp, dob, rh, dw, al, info) == -1          # obs_stages neither 1 nor N
    assert raw(s, 0, D, None, None, 0, None, None, None, None, None, None, dw, None, None) == 0
    k1 = _product_solver(R.cfg_two(8), 4, kernel=1)
    c2 = R.cfg_two(8)
    assert raw(k1, 0, D, None, None, 0, None, None, None, None, None, None, dw, None, None) == -2
    assert raw(k1, B, D, t(B, 2 * c2.nx), None, 0, t(B, c2.n_var), t(B, c2.n_g), t(B, c2.n_var), t(B, D, 2 * c2.nx), None, None, dw, al, info) == -2
    with pytest.raises(ValueError):
        s.sens_update_multi(_np(p), _np(w), _np(lg), _np(lx), dobs=_np(dob[:, :D]))      # dobs without obstacles=
    with pytest.raises(ValueError):
        s.sens_update_multi(_np(p), _np(w), _np(lg), _np(lx), obstacles=_np(ob))         # no direction given
    with pytest.raises(ValueError):
        s.sens_update_multi(_np(p), _np(w), _np(lg), _np(lx), dp=_np(dp))                # D = 65


@pytest.mark.parametrize("cfg", [R.cfg_two(8), R.cfg_six(6), R.cfg_ten(5)], ids=["m2", "m6", "m10"])
def test_solve_multi_solve_returns_the_first_solves_bits(cfg):
    B, D = 4, 64
    P, W0 = Hh.batch(cfg, B, 11)
    s = _product_solver(cfg, B)
    before = s.workspace_bytes
    a = s.solve_batch(P, W0, want_duals=True)
    rng = np.random.default_rng(5)
    up = s.sens_update_multi(P, a["x"], a["lam_g"], a["lam_x"], dp=0.02 * UR._weights(rng, (B, D, 2 * cfg.nx)), rhs=UR._weights(rng, (B, D, cfg.n_var)))
    b = s.solve_batch(P, W0, want_duals=True)
    assert up["dw"].shape == (B, D, cfg.n_var) and s.workspace_bytes == before
    for key in ("x", "f", "kkt", "lam_g", "lam_x", "lam_p"):
        assert np.array_equal(_bits(_np(a[key])), _bits(_np(b[key]))), key
    assert np.array_equal(_np(a["iters"]), _np(b["iters"])) and np.array_equal(_np(a["status"]), _np(b["status"]))


# ---- the Jacobian
def _column_refs(r, pt, dps=None, dobs=None):
    """[(dw, bound relative to max|dw|)] of the unit directions by the reference"""
    a = (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
    out = []
    for c in range(len(dps if dps is not None else dobs)):
        kw = dict(dp=dps[c]) if dps is not None else dict(dobs=dobs[c])
        ref = UR.stage_update(*a, **kw)
        assert ref["info"] == 0
        out.append((ref["dw"], 100.0 * UR.spread(*a, **kw)[0] + 1e-12))
    return out


JAC_ROWS = [i for i, r in enumerate(ROWS) if r.field and r.m in (1, 3, 6, 10)]


@pytest.mark.parametrize("i", JAC_ROWS, ids=[IDS[i] for i in JAC_ROWS])
def test_plan_jacobian_wrt_p_and_its_duality_with_the_adjoint_call(i):
    o = ran(i); r = o["row"]; cfg = r.cfg; s = o["solver"]
    pt = o["pts"][1]
    a, obs = _point_arrays(r, [pt])
    out = s.plan_jacobian(*a, obstacles=obs)
    J, info = _np(out["J"])[0], _np(out["info"])
    n_p = 2 * cfg.nx
    assert J.shape == (cfg.n_var, n_p) and info[0] == 0
    refs = _column_refs(r, pt, dps=np.eye(n_p))
    worst = 0.0
    for c, (dw, bw) in enumerate(refs):
        e = UR.rel(J[:, c], dw)
        worst = max(worst, e / bw)
        assert e <= bw, (c, e, bw)
    # <wbar, J dp> = <pbar, dp>: against nmpc_sens_adjoint_batch on the same point, the two calls' bounds added
    wbar = AR.row_cotangent(r, 1)
    pbar = _np(s.sens_adjoint_batch(*a, wbar[None], obstacles=obs)["pbar"])[0]
    sp, _ = AR.spread(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, wbar)
    tol = np.array([bw * np.abs(dw).max() for dw, bw in refs]) * np.abs(wbar).sum() + (100.0 * sp + 1e-12) * np.abs(pbar).max()
    err = np.abs(wbar @ J - pbar)
    print("%s: Jacobian columns within %.2e of their bounds; |wbar' J - pbar| at most %.2e, tolerance at least %.2e" % (SP.row_id(r), worst, err.max(), tol.min()))
    assert (err <= tol).all(), (err.max(), tol.min())


OBS_ROWS = [ROWS.index(next(r for r in ROWS if r.kind == "static" and r.m == 2)), ROWS.index(next(r for r in ROWS if r.kind == "moving" and r.m == 4))]


@pytest.mark.parametrize("i", OBS_ROWS, ids=[IDS[i] for i in OBS_ROWS])
def test_plan_jacobian_wrt_obstacles(i):
    """a static field (6 columns) and a per-stage field of eight obstacles (N = 3: 72 columns, two launches)"""
    o = ran(i); r = o["row"]; cfg = r.cfg; s = o["solver"]
    pt = o["pts"][2]
    a, obs = _point_arrays(r, [pt])
    out = s.plan_jacobian(*a, obstacles=obs, wrt="obstacles")
    J = _np(out["J"])[0]
    n = pt.obs.size
    assert J.shape == (cfg.n_var, n) and _np(out["info"])[0] == 0
    refs = _column_refs(r, pt, dobs=np.eye(n).reshape((n,) + pt.obs.shape))
    for c, (dw, bw) in enumerate(refs):
        assert np.abs(J[:, c] - dw).max() <= bw * np.abs(dw).max(), (c, np.abs(J[:, c] - dw).max(), bw, np.abs(dw).max())
    if r.kind == "moving":
        assert not J[:, : cfg.K * 3].any()      # entry 0 of a per-stage field carries nothing


# ---- the controller
def _six_with_a_field():
    cfg = R.cfg_six(8)
    cfg.obstacles = [(0.1, -0.2, 0.15)]
    return cfg


def test_correct_scenarios_is_correct_per_scenario():
    import nmpc_amd
    cfg = _six_with_a_field()
    B, D = 3, 3
    P, W0 = Hh.batch(cfg, B, 23)
    obs = np.tile(np.asarray(cfg.obstacles, float)[None], (B, 1, 1))
    rng = np.random.default_rng(9)
    amp = np.array([2e-3, 2e-3, 0.3])      # the last scenario is far enough for a step limit
    x0c = P[:, None, : cfg.nx] + amp[None, :, None] * rng.standard_normal((B, D, cfg.nx))
    obc = obs[:, None] + 2e-3 * rng.standard_normal((B, D) + obs.shape[1:])
    s = _product_solver(cfg, B)
    ctl = nmpc_amd.AdvancedStepController(s)
    pre = ctl.prepare(P, W0, obstacles=obs)
    multi = ctl.correct_scenarios(x0c, obstacles=obc)
    unc = ctl.last["uncorrected"]
    w, lam_g, lam_x, status = (_np(pre[k]) for k in ("x", "lam_g", "lam_x", "status"))
    assert multi["w"].shape == (B, D, cfg.n_var) and multi["u0"].shape == (B, D, cfg.nu) and multi["step"].shape == (B, D) and multi["corrected"].shape == (B,)
    uo = cfg.nx * (cfg.N + 1)
    for d in range(D):
        one = ctl.correct(x0c[:, d], obstacles=obc[:, d])
        assert ctl.last["uncorrected"] == unc
        assert np.array_equal(_np(one["corrected"]), _np(multi["corrected"])) and np.array_equal(_np(one["info"]), _np(multi["info"]))
        for b in range(B):
            mw, ow, step = _np(multi["w"])[b, d], _np(one["w"])[b], float(_np(multi["step"])[b, d])
            if not _np(multi["corrected"])[b]:
                assert np.array_equal(_bits(mw), _bits(w[b])) and np.array_equal(_bits(ow), _bits(w[b]))
                continue
            dp = np.concatenate([x0c[b, d] - P[b, : cfg.nx], np.zeros(cfg.nx)])
            a = (cfg, P[b], w[b], lam_g[b], lam_x[b], obs[b])
            ref = UR.stage_update(*a, dp=dp, dobs=obc[b, d] - obs[b])
            sw, sa = UR.spread(*a, dp=dp, dobs=obc[b, d] - obs[b])
            tol = (100.0 * sw + 1e-12) * np.abs(ref["dw"]).max() * step
            al_m, al_o = float(_np(multi["alpha"])[b, d]), float(_np(one["alpha"])[b])
            print("instance %d scenario %d: |w_multi - w_correct| %.2e, tolerance %.2e, step %.6f / %.6f" % (b, d, np.abs(mw - ow).max(), tol, step, float(_np(one["step"])[b])))
            assert np.abs(mw - ow).max() <= tol, (b, d, np.abs(mw - ow).max(), tol)
            assert abs(al_m - al_o) <= (100.0 * sa + 1e-12) * ref["alpha"] and (al_m == 1.0) == (al_o == 1.0)
            assert step == (1.0 if al_m == 1.0 else ctl.tau * al_m)
            assert np.array_equal(_bits(_np(multi["u0"])[b, d]), _bits(mw[uo: uo + cfg.nu]))
    print("correct_scenarios: %d of %d instances corrected (status %s)" % (int(_np(multi["corrected"]).sum()), B, status.tolist()))
    assert _np(multi["corrected"]).any()
    assert (_np(multi["alpha"])[_np(multi["corrected"])] < 1.0).any(), "no scenario met a step limit: the tau * alpha branch was not run"


def test_correct_scenarios_leaves_an_unconverged_plan_as_it_is():
    import nmpc_amd
    cfg = _six_with_a_field()
    B, D = 2, 3
    P, W0 = Hh.batch(cfg, B, 23)
    obs = np.tile(np.asarray(cfg.obstacles, float)[None], (B, 1, 1))
    ctl = nmpc_amd.AdvancedStepController(_product_solver(cfg, B, max_iter=1))
    pre = ctl.prepare(P, W0, obstacles=obs)
    out = ctl.correct_scenarios(P[:, None, : cfg.nx] + 1e-3 * np.ones((B, D, cfg.nx)), obstacles=np.tile(obs[:, None], (1, D, 1, 1)))
    assert (_np(pre["status"]) != 0).all() and not _np(out["corrected"]).any() and ctl.last["uncorrected"] == B
    for d in range(D):
        assert np.array_equal(_bits(_np(out["w"])[:, d]), _bits(_np(pre["x"])))
