"""-m gpu: nmpc_sens_update_batch (csrc/nmpc_sens.hip) and nmpc_amd.AdvancedStepController.

Every instantiation of sens_kernel<MS, SENS_UPDATE> against tests/sens_update_ref.py on the constructed points of tests/sens_points.py, with the point's dp
and a seeded dobs and rhs that have weight on every entry: dw and alpha on every row.  The bound is the project's: 100 x that point's spread
+ 1e-12, relative to max|dw| and to alpha; a kernel without the Sigma n n' term or the radius column of M_o, or one that reads the wrong entry
of the field, is 1000 x that bound away (tests/test_sens_update_host.py).  Then the bit-level properties, the agreement with nmpc_sens_batch and
nmpc_sens_adjoint_batch, the verdict batches, the argument errors, the oracle's re-solves under a moved state and field
(tests/golden/sens_update_cases.npz, tests/golden/sens_obs_cases.npz), and the controller."""
import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import sens_adjoint_ref as AR
from tests import sens_points as SP
from tests import sens_ref as S
from tests import sens_update_ref as UR

pytestmark = pytest.mark.gpu

ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
_CACHE = {}


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


def _stack(xs):
    return None if xs is None or xs[0] is None else np.stack(xs)


def _call(s, r, pts, dps=None, dobs=None, rhs=None, **kw):
    obs = np.stack([pt.obs for pt in pts]) if r.field else None      # an "own" row calls with (NULL, 0): the handle's field, no dobs
    out = s.sens_update_batch(np.stack([pt.p for pt in pts]), np.stack([pt.w for pt in pts]), np.stack([pt.lam_g for pt in pts]),
                              np.stack([pt.lam_x for pt in pts]), dp=_stack(dps), dobs=_stack(dobs), rhs=_stack(rhs), obstacles=obs, **kw)
    return {k: _np(v) for k, v in out.items()}


def _raw(s, r, pts, dps, dobs, rhs, want_dw, want_alpha):
    """the C call itself, for the output combinations the method does not offer: (dw or None, alpha or None, info)"""
    import torch
    B = len(pts)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=s.device)
    ptr = lambda x: None if x is None else x.data_ptr()
    cfg = r.cfg
    obs = t(np.stack([pt.obs for pt in pts])) if r.field else None
    S_ = 0 if obs is None else (1 if obs.dim() == 3 else cfg.N)
    a = [t(np.stack([getattr(pt, k) for pt in pts])) for k in ("p", "w", "lam_g", "lam_x")]
    dp_, do_, rh_ = t(_stack(dps)), t(_stack(dobs)), t(_stack(rhs))
    dw = torch.empty((B, cfg.n_var), dtype=torch.float64, device=s.device) if want_dw else None
    al = torch.empty(B, dtype=torch.float64, device=s.device) if want_alpha else None
    info = torch.full((B,), -7, dtype=torch.int32, device=s.device)
    rc = s.lib.nmpc_sens_update_batch(s._h, B, ptr(a[0]), ptr(obs), S_, ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(dp_), ptr(do_), ptr(rh_), ptr(dw), ptr(al), ptr(info),
                                      s._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _np(dw), _np(al), _np(info)


def ran(i):
    """row i: its handle, the call on its points, the same batch reversed, and the reference with its spread per point — once per session"""
    if i in _CACHE:
        return _CACHE[i]
    r = ROWS[i]
    pts = SP.points(r); n = len(pts)
    dps = [pt.dp for pt in pts]
    dobs = [UR.row_dobs(r, k) for k in range(n)]
    rhs = [UR.row_rhs(r, k) for k in range(n)]
    s = _solver(r.cfg, 2 * n + 2)
    full = _call(s, r, pts, dps, dobs, rhs)
    back = _call(s, r, pts[::-1], dps[::-1], dobs[::-1], rhs[::-1])
    ref = [UR.stage_update(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=a, dobs=b, rhs=c) for pt, a, b, c in zip(pts, dps, dobs, rhs)]
    spread = [UR.spread(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=a, dobs=b, rhs=c) for pt, a, b, c in zip(pts, dps, dobs, rhs)]
    _CACHE[i] = dict(row=r, pts=pts, dps=dps, dobs=dobs, rhs=rhs, n=n, solver=s, full=full, back=back, ref=ref, spread=spread)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_parity_against_numpy(i):
    o = ran(i); r = o["row"]; cfg = r.cfg
    dw, alpha, info = o["full"]["dw"], o["full"]["alpha"], o["full"]["info"]
    assert dw.shape == (o["n"], cfg.n_var) and alpha.shape == (o["n"],)
    worst = (0.0, 0.0, 0.0, 0.0)
    for b in range(o["n"]):
        ref, (sw, sa) = o["ref"][b], o["spread"][b]
        assert info[b] == ref["info"] == 0, (b, info[b], ref["info"])
        ew = UR.rel(dw[b], ref["dw"]); ea = abs(alpha[b] - ref["alpha"]) / ref["alpha"]
        print("%s %d: dw %.2e (spread %.2e), alpha %.6g against %.6g: %.2e (spread %.2e), max|dw| %.2e" % (
            SP.row_id(r), b, ew, sw, alpha[b], ref["alpha"], ea, sa, np.abs(ref["dw"]).max()))
        worst = max(worst, (max(ew, ea), ew, max(sw, sa), ea))
        assert ew <= 100.0 * sw + 1e-12, (b, ew, sw)
        assert ea <= 100.0 * sa + 1e-12, (b, ea, sa)
        assert 0.0 < alpha[b] <= 1.0
    print("%s: largest parity error %.2e (dw %.2e, alpha %.2e) at spread %.2e" % (SP.row_id(r), worst[0], worst[1], worst[3], worst[2]))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_same_bits_reversed_repeated_and_per_output(i):
    """the reversed batch, a second call, and the dw-only / alpha-only calls return the bits of the first call; with both outputs NULL the same info"""
    o = ran(i); r = o["row"]; f, k = o["full"], o["back"]
    again = _call(o["solver"], r, o["pts"], o["dps"], o["dobs"], o["rhs"])
    assert np.array_equal(k["info"][::-1], f["info"]) and np.array_equal(again["info"], f["info"])
    for key in ("dw", "alpha"):
        assert np.array_equal(_bits(k[key][::-1]), _bits(f[key])), key
        assert np.array_equal(_bits(again[key]), _bits(f[key])), key
    only = _call(o["solver"], r, o["pts"], o["dps"], o["dobs"], o["rhs"], want_alpha=False)
    assert only["alpha"] is None and np.array_equal(_bits(only["dw"]), _bits(f["dw"])) and np.array_equal(only["info"], f["info"])
    dw, al, info = _raw(o["solver"], r, o["pts"], o["dps"], o["dobs"], o["rhs"], False, True)
    assert dw is None and np.array_equal(_bits(al), _bits(f["alpha"])) and np.array_equal(info, f["info"])
    dw, al, info = _raw(o["solver"], r, o["pts"], o["dps"], o["dobs"], o["rhs"], False, False)
    assert dw is None and al is None and np.array_equal(info, f["info"])


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_agrees_with_the_two_existing_calls(i):
    """dp alone: the dw of nmpc_sens_batch, within the two calls' bounds.  rhs = wbar alone: dw is the v of the adjoint call's text, so
    sum_k 2 Q v_Xk and -M_o' v, formed in numpy from the device's dw, reproduce pbar_xs and obsbar of nmpc_sens_adjoint_batch, each side within
    its own bound (an extra check, not the parity measure)"""
    o = ran(i); r = o["row"]; cfg = r.cfg; pts = o["pts"]; s = o["solver"]
    obs = np.stack([pt.obs for pt in pts]) if r.field else None
    P, Wp, LG, LX = (np.stack([getattr(pt, k) for pt in pts]) for k in ("p", "w", "lam_g", "lam_x"))
    fw = _np(s.sens_batch(P, Wp, LG, LX, dp=np.stack(o["dps"]), obstacles=obs)["dw"])
    up = _call(s, r, pts, o["dps"])
    wbars = [AR.row_cotangent(r, k) for k in range(o["n"])]
    ad = s.sens_adjoint_batch(P, Wp, LG, LX, np.stack(wbars), obstacles=obs)
    pbar, obsbar = _np(ad["pbar"]), _np(ad["obsbar"])
    v = _call(s, r, pts, rhs=wbars, want_alpha=False)["dw"]
    qd = np.tile(np.asarray(cfg.q, float), cfg.m)
    for b, pt in enumerate(pts):
        a = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        _, s1 = S.spread(*a, dp=pt.dp)
        s2, _ = UR.spread(*a, dp=pt.dp)
        e = UR.rel(up["dw"][b], fw[b])
        print("%s %d: dp alone against nmpc_sens_batch %.2e (spreads %.2e, %.2e)" % (SP.row_id(r), b, e, s1, s2))
        assert e <= (100.0 * s1 + 1e-12) + (100.0 * s2 + 1e-12), (b, e, s1, s2)
        sp, so = AR.spread(*a, wbars[b])
        sv, _ = UR.spread(*a, rhs=wbars[b])
        bv = (100.0 * sv + 1e-12) * np.abs(v[b]).max()
        assert not v[b][: cfg.nx].any()
        xs = AR._pbar_xs(cfg, v[b])
        tol = (100.0 * sp + 1e-12) * np.abs(pbar[b]).max() + bv * 2.0 * qd * cfg.N
        assert (np.abs(xs - pbar[b][cfg.nx:]) <= tol).all(), (b, np.abs(xs - pbar[b][cfg.nx:]).max(), tol.min())
        eo = 0.0
        if obsbar is not None:
            Mo = AR.obstacle_matrix(cfg, pt.w, pt.lam_g, pt.obs)
            ob = -(Mo.T @ v[b])
            tol = (100.0 * so + 1e-12) * np.abs(obsbar[b]).max() + bv * np.abs(Mo).sum(axis=0)
            eo = np.abs(ob - obsbar[b].reshape(-1)).max()
            assert (np.abs(ob - obsbar[b].reshape(-1)) <= tol).all(), (b, eo, tol.min())
        print("%s %d: rhs = wbar alone: pbar_xs off by %.2e, obsbar by %.2e" % (SP.row_id(r), b, np.abs(xs - pbar[b][cfg.nx:]).max(), eo))


@pytest.mark.parametrize("i", [i for i, r in enumerate(ROWS) if r.kind == "moving"], ids=[IDS[i] for i, r in enumerate(ROWS) if r.kind == "moving"])
def test_entry_0_of_a_per_stage_dobs_is_not_read(i):
    o = ran(i); r = o["row"]
    other = [d.copy() for d in o["dobs"]]
    for n, d in enumerate(other):
        d[0] = 7.0 + n
    got = _call(o["solver"], r, o["pts"], o["dps"], other, o["rhs"])
    for key in ("dw", "alpha"):
        assert np.array_equal(_bits(got[key]), _bits(o["full"][key])), key


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_in_a_mixed_batch(r):
    """each verdict case is one instance between clean points: dw and alpha are zeros and its neighbours keep the bits of the parity call"""
    i = ROWS.index(r)
    o = ran(i); cfg = r.cfg
    cases = SP.verdict_cases(r, o["pts"][0])[1:]
    batch, dps, dobs, rhs, clean = [], [], [], [], []
    for c, (name, pt, want) in enumerate(cases):
        a = c % o["n"]; clean.append(a)
        batch += [o["pts"][a], pt]
        dps += [o["dps"][a], pt.dp]; dobs += [o["dobs"][a], o["dobs"][0]]; rhs += [o["rhs"][a], o["rhs"][0]]
    s = _solver(cfg, len(batch))
    got = _call(s, r, batch, dps, dobs, rhs)
    info = got["info"]
    for c, (name, pt, want) in enumerate(cases):
        b = 2 * c + 1
        a = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        ref = UR.stage_update(*a, dp=pt.dp, dobs=o["dobs"][0], rhs=o["rhs"][0])
        assert info[b] == ref["info"] == want, (name, info[b], ref["info"], want)
        if want:
            assert not got["dw"][b].any() and got["alpha"][b] == 0.0, name
        else:      # the pair row of the wrong sign: no Sigma, its Hessian term stays in
            sw, sa = UR.spread(*a, dp=pt.dp, dobs=o["dobs"][0], rhs=o["rhs"][0])
            ew, ea = UR.rel(got["dw"][b], ref["dw"]), abs(got["alpha"][b] - ref["alpha"]) / ref["alpha"]
            print("%s: dw %.2e (spread %.2e), alpha %.2e (spread %.2e)" % (name, ew, sw, ea, sa))
            assert ew <= 100.0 * sw + 1e-12 and ea <= 100.0 * sa + 1e-12, (name, ew, sw, ea, sa)
        a = clean[c]
        assert info[2 * c] == 0
        assert np.array_equal(_bits(got["dw"][2 * c]), _bits(o["full"]["dw"][a])) and np.array_equal(_bits(got["alpha"][2 * c]), _bits(o["full"]["alpha"][a])), name


def test_argument_errors():
    import torch
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); o = ran(ROWS.index(r)); cfg = r.cfg; s = o["solver"]
    B = 2
    d = s.device
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=d)
    p, w, lg, lx, dp, rh, dw, al = t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_g), t(B, cfg.n_var), t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_var), t(B)
    ob, dob = t(B, cfg.N, cfg.K, 3), t(B, cfg.N, cfg.K, 3)
    info = torch.zeros(B, dtype=torch.int32, device=d)
    ptr = lambda x: None if x is None else x.data_ptr()

    def raw(B_, p_, obs_, S_, w_, lg_, lx_, dp_, dob_, rh_, dw_, al_, info_):
        return s.lib.nmpc_sens_update_batch(s._h, B_, ptr(p_), ptr(obs_), S_, ptr(w_), ptr(lg_), ptr(lx_), ptr(dp_), ptr(dob_), ptr(rh_), ptr(dw_), ptr(al_),
                                            ptr(info_), s._stream())
    assert raw(B, p, None, 0, w, lg, lx, dp, dob, rh, dw, al, info) == -1      # dobs without obs: the handle's own field has no change to give
    for k in range(4):      # null p, w, lam_g, lam_x
        a = [p, w, lg, lx]; a[k] = None
        assert raw(B, a[0], ob, cfg.N, a[1], a[2], a[3], dp, dob, rh, dw, al, info) == -1, k
    assert raw(B, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, None) == -1
    assert raw(B, p, ob, 2, w, lg, lx, dp, dob, rh, dw, al, info) == -1              # obs_stages neither 1 nor N
    assert raw(B, p, None, cfg.N, w, lg, lx, dp, None, rh, dw, al, info) == -1       # obs_stages without a field
    assert raw(s.max_batch + 1, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, info) == -1
    assert raw(-1, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, info) == -1
    assert raw(0, None, None, 0, None, None, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    for pin in (1, 2):
        k = _product_solver(R.cfg_two(8), 4, kernel=pin)
        assert k.lib.nmpc_sens_update_batch(k._h, 0, None, None, 0, None, None, None, None, None, None, None, None, None, None) == -2
    with pytest.raises(ValueError):
        s.sens_update_batch(_np(p), _np(w), _np(lg), _np(lx), dobs=_np(dob))


# ---- on a solve's own output
def _fixture_batch(c):
    cfg = c["cfg"]
    return c["p"], np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in c["p"]]), c["obs"]


def test_solve_update_solve_returns_the_first_solves_bits():
    c = UR.load_cases()["three_moving"]; cfg = c["cfg"]
    P, W0, obs = _fixture_batch(c)
    s = _product_solver(cfg, 4)
    a = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    dp = np.stack([UR.case_dp(cfg, dx) for dx in c["dx"]])
    up = s.sens_update_batch(P, a["x"], a["lam_g"], a["lam_x"], dp=dp, dobs=c["d"], rhs=np.stack([AR.cotangent(cfg, b) for b in range(4)]), obstacles=obs)
    b = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    assert (_np(a["status"]) == 0).all() and (_np(up["info"]) == 0).all()
    for key in ("x", "f", "kkt", "lam_g", "lam_x", "lam_p"):
        assert np.array_equal(_bits(_np(a[key])), _bits(_np(b[key]))), key
    assert np.array_equal(_np(a["iters"]), _np(b["iters"]))


def _end_to_end(cases, with_state):
    """(largest |w_dev + dw_dev - w(h)| over the instances, the same for the numpy reference at the oracle's own point and multipliers), dw for the
    step h (dx, d) itself, so that the call's alpha is the alpha of that step; alpha == 1 is asserted on every instance"""
    worst = worst_ref = 0.0
    for name, c in cases.items():
        cfg = c["cfg"]; h = c["h"]
        P, W0, obs = _fixture_batch(c)
        s = _product_solver(cfg, 4)
        a = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
        dp = h * np.stack([UR.case_dp(cfg, dx) for dx in c["dx"]]) if with_state else None
        up = s.sens_update_batch(P, a["x"], a["lam_g"], a["lam_x"], dp=dp, dobs=h * c["d"], obstacles=obs)
        assert (_np(a["status"]) == 0).all() and (_np(up["info"]) == 0).all(), name
        w, dw, alpha = _np(a["x"]), _np(up["dw"]), _np(up["alpha"])
        for b in range(4):
            ref = UR.stage_update(cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], c["obs"][b], dp=None if dp is None else dp[b], dobs=h * c["d"][b])
            eg, er = np.abs(w[b] + dw[b] - c["w_h"][b]).max(), np.abs(c["w"][b] + ref["dw"] - c["w_h"][b]).max()
            print("%s %d: |w + h dw - w(h)| of the device %.2e, of the reference %.2e, alpha %.6f (reference %.6f), |w - w_oracle| %.1e" % (
                name, b, eg, er, alpha[b], ref["alpha"], np.abs(w[b] - c["w"][b]).max()))
            worst, worst_ref = max(worst, eg), max(worst_ref, er)
            assert alpha[b] == 1.0, (name, b, alpha[b])
    return worst, worst_ref


def test_update_against_the_oracles_resolves_under_a_moved_state_and_field():
    """tests/golden/sens_update_cases.npz end to end: solve on the device with duals, one update launch for the simultaneous move h (dx, d), the
    prediction against the oracle's re-solve.  Tolerance: 10 x the same figure for the numpy reference at the oracle's own point and least-squares
    multipliers (the step's O(h^2) and the barrier's O(mu) are in both, the solve's 1e-6 point parity only in the device's — the margin of
    tests/test_gpu_sens_adjoint.py::test_obstacle_gradient_against_the_oracles_resolves).  Measured on MI355X: 5.02e-4 for both, on the same
    instance."""
    worst, worst_ref = _end_to_end(UR.load_cases(), True)
    print("largest prediction error: device %.3e, reference %.3e, tolerance %.3e" % (worst, worst_ref, 10.0 * worst_ref))
    assert worst <= 10.0 * worst_ref, (worst, worst_ref)


def test_update_against_the_oracles_resolves_under_a_moved_field():
    """the same on tests/golden/sens_obs_cases.npz, where only the field moves (dp == NULL).  Measured on MI355X: 1.57e-4 for both."""
    cases = AR.load_obs_cases()
    for c in cases.values():
        c["dx"] = np.zeros((4, c["cfg"].nx))
    worst, worst_ref = _end_to_end(cases, False)
    print("largest prediction error: device %.3e, reference %.3e, tolerance %.3e" % (worst, worst_ref, 10.0 * worst_ref))
    assert worst <= 10.0 * worst_ref, (worst, worst_ref)


# ---- the controller
@pytest.mark.parametrize("name", list(AR.obs_case_configs()))
def test_controller_is_the_direct_call_and_improves_the_first_control(name):
    import nmpc_amd
    c = UR.load_cases()[name]; cfg = c["cfg"]; h = c["h"]
    P, W0, obs = _fixture_batch(c)
    s = _product_solver(cfg, 4)
    ctl = nmpc_amd.AdvancedStepController(s)
    pre = ctl.prepare(P, W0, obstacles=obs)
    x0m = P[:, : cfg.nx] + h * c["dx"]
    out = ctl.correct(x0m, obstacles=obs + h * c["d"])
    assert (_np(pre["status"]) == 0).all()
    # the direct call with the controller's own differences
    import torch
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=s.device)
    dp = torch.zeros((4, 2 * cfg.nx), dtype=torch.float64, device=s.device)
    dp[:, : cfg.nx] = t(x0m) - t(P)[:, : cfg.nx]
    direct = s.sens_update_batch(P, pre["x"], pre["lam_g"], pre["lam_x"], dp=dp, dobs=t(obs + h * c["d"]) - t(obs), obstacles=obs)
    assert (_np(direct["info"]) == 0).all() and (_np(direct["alpha"]) == 1.0).all()
    assert np.array_equal(_bits(_np(out["w"])), _bits(_np(pre["x"] + direct["dw"])))
    assert _np(out["corrected"]).all() and ctl.last["uncorrected"] == 0 and (_np(out["step"]) == 1.0).all() and (_np(out["alpha"]) == 1.0).all()
    uo = cfg.nx * (cfg.N + 1); sl = slice(uo, uo + cfg.nu)
    u0, u_pre = _np(out["u0"]), _np(pre["x"])[:, sl]
    assert np.array_equal(_bits(u0), _bits(_np(out["w"])[:, sl]))
    for b in range(4):
        e1, e0 = np.abs(u0[b] - c["w_h"][b][sl]).max(), np.abs(u_pre[b] - c["w_h"][b][sl]).max()
        print("%s %d: |U_0 - U_0(h)| corrected %.2e, prepared %.2e" % (name, b, e1, e0))
        assert e1 < e0, (name, b, e1, e0)
    # a correction with nothing to correct returns the prepared plan, and the solver's state is untouched: the same solve again, the same bits
    same = ctl.correct(P[:, : cfg.nx])
    assert np.array_equal(_np(same["w"]), _np(pre["x"])) and (_np(same["alpha"]) == 1.0).all()
    again = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    assert np.array_equal(_bits(_np(again["x"])), _bits(_np(pre["x"])))


def test_controller_leaves_an_unconverged_plan_as_it_is():
    import nmpc_amd
    c = UR.load_cases()["two_static"]; cfg = c["cfg"]; h = c["h"]
    P, W0, obs = _fixture_batch(c)
    ctl = nmpc_amd.AdvancedStepController(_product_solver(cfg, 4, max_iter=1))
    pre = ctl.prepare(P, W0, obstacles=obs)
    out = ctl.correct(P[:, : cfg.nx] + h * c["dx"], obstacles=obs + h * c["d"])
    assert (_np(pre["status"]) != 0).all()
    assert np.array_equal(_bits(_np(out["w"])), _bits(_np(pre["x"])))
    assert not _np(out["corrected"]).any() and ctl.last["uncorrected"] == 4


def test_controller_needs_a_handle_with_multipliers():
    import nmpc_amd
    with pytest.raises(RuntimeError, match="multipliers"):
        nmpc_amd.AdvancedStepController(_product_solver(R.cfg_two(8), 4, kernel=1))
