"""-m gpu: nmpc_sens_adjoint_batch (csrc/nmpc_sens.hip) and nmpc_amd.NmpcLayer.

Every instantiation of sens_kernel<MS, SENS_ADJOINT> against tests/sens_adjoint_ref.py on the constructed points of tests/sens_points.py, with a seeded
cotangent that has weight on every entry: pbar on every row, obsbar on the rows with a per-instance field.  The bound is the project's:
100 x that point's spread + 1e-12 relative to max|pbar| / max|obsbar|; a kernel without the Sigma n n' term or the radius column, or one that reads
the wrong entry of the field, is 1000 x that bound away (tests/test_sens_adjoint_host.py).  Then the verdict batches, the bit-level properties,
<wbar, dw> of nmpc_sens_batch against <pbar, dp>, the oracle's re-solves under a moved obstacle field (tests/golden/sens_obs_cases.npz), and the
autograd layer."""
import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import sens_adjoint_ref as AR
from tests import sens_points as SP
from tests import sens_ref as S

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


def _has_obsbar(r):
    return r.kind in ("static", "moving")


def _call(s, r, pts, wbars, **kw):
    obs = np.stack([pt.obs for pt in pts]) if r.field else None      # an "own" row calls with (NULL, 0): the handle's field, no obsbar
    out = s.sens_adjoint_batch(np.stack([pt.p for pt in pts]), np.stack([pt.w for pt in pts]), np.stack([pt.lam_g for pt in pts]),
                               np.stack([pt.lam_x for pt in pts]), np.stack(wbars), obstacles=obs, **kw)
    return {k: _np(v) for k, v in out.items()}


def ran(i):
    """row i: its handle, the call on its points, the same batch reversed, and the reference with its spread per point — once per session"""
    if i in _CACHE:
        return _CACHE[i]
    r = ROWS[i]
    pts = SP.points(r); n = len(pts)
    wbars = [AR.row_cotangent(r, k) for k in range(n)]
    s = _solver(r.cfg, 2 * n + 2)
    full = _call(s, r, pts, wbars)
    back = _call(s, r, pts[::-1], wbars[::-1])
    ref = [AR.stage_adjoint(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, wb, want_obsbar=_has_obsbar(r)) for pt, wb in zip(pts, wbars)]
    spread = [AR.spread(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, wb) for pt, wb in zip(pts, wbars)]
    _CACHE[i] = dict(row=r, pts=pts, wbars=wbars, n=n, solver=s, full=full, back=back, ref=ref, spread=spread)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_parity_against_numpy(i):
    o = ran(i); r = o["row"]; cfg = r.cfg
    pbar, obsbar, info = o["full"]["pbar"], o["full"]["obsbar"], o["full"]["info"]
    assert pbar.shape == (o["n"], 2 * cfg.nx) and (obsbar is None) == (not _has_obsbar(r))
    if obsbar is not None:
        assert obsbar.shape == ((o["n"], cfg.K, 3) if r.kind == "static" else (o["n"], cfg.N, cfg.K, 3))
    worst = (0.0, 0.0)
    for b in range(o["n"]):
        ref, (sp, so) = o["ref"][b], o["spread"][b]
        assert info[b] == ref["info"] == 0, (b, info[b], ref["info"])
        ep = AR.rel(pbar[b], ref["pbar"])
        eo = AR.rel(obsbar[b].reshape(ref["obsbar"].shape), ref["obsbar"]) if obsbar is not None else 0.0
        print("%s %d: pbar %.2e (spread %.2e), obsbar %.2e (spread %.2e), max|pbar| %.2e" % (SP.row_id(r), b, ep, sp, eo, so, np.abs(ref["pbar"]).max()))
        worst = max(worst, (max(ep, eo), max(sp, so)))
        assert ep <= 100.0 * sp + 1e-12, (b, ep, sp)
        assert eo <= 100.0 * so + 1e-12, (b, eo, so)
        if r.kind == "moving":
            assert not obsbar[b, 0].any(), b      # entry 0 of a per-stage field: exactly zero
    print("%s: largest parity error %.2e at spread %.2e" % (SP.row_id(r), worst[0], worst[1]))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_same_bits_reversed_repeated_and_per_output(i):
    """the reversed batch, a second call, and pbar-only / obsbar-only calls all return the bits of the first call"""
    o = ran(i); r = o["row"]; f, k = o["full"], o["back"]
    again = _call(o["solver"], r, o["pts"], o["wbars"])
    outs = ["pbar"] + (["obsbar"] if _has_obsbar(r) else [])
    assert np.array_equal(k["info"][::-1], f["info"]) and np.array_equal(again["info"], f["info"])
    for key in outs:
        assert np.array_equal(_bits(k[key][::-1]), _bits(f[key])), key
        assert np.array_equal(_bits(again[key]), _bits(f[key])), key
    if _has_obsbar(r):
        po = _call(o["solver"], r, o["pts"], o["wbars"], want_obsbar=False)
        oo = _call(o["solver"], r, o["pts"], o["wbars"], want_pbar=False)
        assert po["obsbar"] is None and oo["pbar"] is None
        assert np.array_equal(_bits(po["pbar"]), _bits(f["pbar"])) and np.array_equal(_bits(oo["obsbar"]), _bits(f["obsbar"]))
    none = _call(o["solver"], r, o["pts"], o["wbars"], want_pbar=False, want_obsbar=False)      # both NULL still computes info
    assert none["pbar"] is None and none["obsbar"] is None and np.array_equal(none["info"], f["info"])


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_consistent_with_the_forward_call(i):
    """<wbar, dw> of nmpc_sens_batch(dp) against <pbar, dp>, each side within its own parity bound (an extra check, not the parity measure)"""
    o = ran(i); r = o["row"]; pts = o["pts"]
    obs = np.stack([pt.obs for pt in pts]) if r.field else None
    fw = o["solver"].sens_batch(np.stack([pt.p for pt in pts]), np.stack([pt.w for pt in pts]), np.stack([pt.lam_g for pt in pts]),
                                np.stack([pt.lam_x for pt in pts]), dp=np.stack([pt.dp for pt in pts]), obstacles=obs)
    dw = _np(fw["dw"])
    for b, pt in enumerate(pts):
        sp, _ = o["spread"][b]
        _, sw = S.spread(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=pt.dp)
        pbar, wbar = o["full"]["pbar"][b], o["wbars"][b]
        lhs, rhs = pbar @ pt.dp, wbar @ dw[b]
        tol = (100.0 * sp + 1e-12) * np.abs(pbar).max() * np.abs(pt.dp).sum() + (100.0 * sw + 1e-12) * np.abs(dw[b]).max() * np.abs(wbar).sum()
        print("%s %d: <pbar, dp> %.6e, <wbar, dw> %.6e, difference %.2e (allowed %.2e)" % (SP.row_id(r), b, lhs, rhs, abs(lhs - rhs), tol))
        assert abs(lhs - rhs) <= tol, (b, lhs, rhs, tol)


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_in_a_mixed_batch(r):
    """each verdict case is one instance between clean points: its outputs are zeros and its neighbours keep the bits of the parity call"""
    i = ROWS.index(r)
    o = ran(i); cfg = r.cfg
    cases = SP.verdict_cases(r, o["pts"][0])[1:]
    batch, wbars, clean = [], [], []
    for c, (name, pt, want) in enumerate(cases):
        clean.append(c % o["n"])
        batch += [o["pts"][clean[-1]], pt]
        wbars += [o["wbars"][clean[-1]], o["wbars"][0]]
    s = _solver(cfg, len(batch))
    got = _call(s, r, batch, wbars)
    info = got["info"]
    for c, (name, pt, want) in enumerate(cases):
        b = 2 * c + 1
        ref = AR.stage_adjoint(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, o["wbars"][0])
        assert info[b] == ref["info"] == want, (name, info[b], ref["info"], want)
        if want:
            assert not got["pbar"][b].any() and not got["obsbar"][b].any(), name
        else:      # the pair row of the wrong sign: no Sigma, its Hessian term stays in
            sp, so = AR.spread(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, o["wbars"][0])
            ep, eo = AR.rel(got["pbar"][b], ref["pbar"]), AR.rel(got["obsbar"][b], ref["obsbar"])
            print("%s: pbar %.2e (spread %.2e), obsbar %.2e (spread %.2e)" % (name, ep, sp, eo, so))
            assert ep <= 100.0 * sp + 1e-12 and eo <= 100.0 * so + 1e-12, (name, ep, sp, eo, so)
        a = clean[c]
        assert info[2 * c] == 0
        assert np.array_equal(_bits(got["pbar"][2 * c]), _bits(o["full"]["pbar"][a])) and np.array_equal(_bits(got["obsbar"][2 * c]), _bits(o["full"]["obsbar"][a])), name


# ---- on a solve's own output
def _fixture_batch(c):
    cfg = c["cfg"]
    return c["p"], np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in c["p"]]), c["obs"]


def _product_solver(cfg, max_batch, **kw):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, pair_rows=cfg.pair_rows), max_batch=max_batch, **kw)


def test_solve_adjoint_solve_returns_the_first_solves_bits():
    c = AR.load_obs_cases()["three_moving"]; cfg = c["cfg"]
    P, W0, obs = _fixture_batch(c)
    s = _product_solver(cfg, 4)
    a = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    wbar = np.stack([AR.cotangent(cfg, b) for b in range(4)])
    ad = s.sens_adjoint_batch(P, a["x"], a["lam_g"], a["lam_x"], wbar, obstacles=obs)
    b = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    assert (_np(a["status"]) == 0).all() and (_np(ad["info"]) == 0).all()
    for key in ("x", "f", "kkt", "lam_g", "lam_x", "lam_p"):
        assert np.array_equal(_bits(_np(a[key])), _bits(_np(b[key]))), key
    assert np.array_equal(_np(a["iters"]), _np(b["iters"]))


def test_argument_errors():
    import torch
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); o = ran(ROWS.index(r)); cfg = r.cfg; s = o["solver"]
    B = 2
    d = s.device
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=d)
    p, w, lg, lx, wb, pb = t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_g), t(B, cfg.n_var), t(B, cfg.n_var), t(B, 2 * cfg.nx)
    ob, obb = t(B, cfg.N, cfg.K, 3), t(B, cfg.N, cfg.K, 3)
    info = torch.zeros(B, dtype=torch.int32, device=d)
    ptr = lambda x: None if x is None else x.data_ptr()

    def raw(B_, p_, obs_, S_, w_, lg_, lx_, wb_, pb_, obb_, info_):
        return s.lib.nmpc_sens_adjoint_batch(s._h, B_, ptr(p_), ptr(obs_), S_, ptr(w_), ptr(lg_), ptr(lx_), ptr(wb_), ptr(pb_), ptr(obb_), ptr(info_), s._stream())
    assert raw(B, p, None, 0, w, lg, lx, wb, pb, obb, info) == -1      # obsbar without obs: the handle's own field has no cotangent
    for k in range(5):      # null p, w, lam_g, lam_x, wbar
        a = [p, w, lg, lx, wb]; a[k] = None
        assert raw(B, a[0], ob, cfg.N, a[1], a[2], a[3], a[4], pb, obb, info) == -1, k
    assert raw(B, p, ob, cfg.N, w, lg, lx, wb, pb, obb, None) == -1
    assert raw(B, p, ob, 2, w, lg, lx, wb, pb, obb, info) == -1              # obs_stages neither 1 nor N
    assert raw(B, p, None, cfg.N, w, lg, lx, wb, pb, None, info) == -1       # obs_stages without a field
    assert raw(s.max_batch + 1, p, ob, cfg.N, w, lg, lx, wb, pb, obb, info) == -1
    assert raw(-1, p, ob, cfg.N, w, lg, lx, wb, pb, obb, info) == -1
    assert raw(0, None, None, 0, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    for pin in (1, 2):
        k = _product_solver(R.cfg_two(8), 4, kernel=pin)
        assert k.lib.nmpc_sens_adjoint_batch(k._h, 0, None, None, 0, None, None, None, None, None, None, None, None) == -2
    with pytest.raises(ValueError):
        s.sens_adjoint_batch(_np(p), _np(w), _np(lg), _np(lx), _np(wb), want_obsbar=True)


def test_obstacle_gradient_against_the_oracles_resolves():
    """the fixtures end to end: solve on the device with duals, one adjoint call, <obsbar, d> against <wbar, dq> with dq the extrapolated difference
    quotient of the fixture's oracle re-solves, relative to |wbar| |dq|.  Tolerance: 10 x the largest value of the same mismatch for the numpy
    reference at the oracle's own point and least-squares multipliers (1.58e-4 on the committed fixtures, so 1.6e-3: the extrapolation's O(h^2) and
    the barrier's O(mu) are in both, the solve's 1e-6 point parity only in the device's).  Measured on MI355X: 1.50e-4, on the instance that also
    leads the reference's."""
    worst_ref = worst = 0.0
    for name, c in AR.load_obs_cases().items():
        cfg = c["cfg"]
        P, W0, obs = _fixture_batch(c)
        s = _product_solver(cfg, 4)
        a = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
        wbar = np.stack([AR.cotangent(cfg, b) for b in range(4)])
        ad = s.sens_adjoint_batch(P, a["x"], a["lam_g"], a["lam_x"], wbar, obstacles=obs)
        assert (_np(a["status"]) == 0).all() and (_np(ad["info"]) == 0).all(), name
        ob = _np(ad["obsbar"])
        for b in range(4):
            ref = AR.stage_adjoint(cfg, c["p"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b], c["obs"][b], wbar[b])
            mr, mg = AR.obs_mismatch(c, b, ref["obsbar"].reshape(c["d"][b].shape), wbar[b]), AR.obs_mismatch(c, b, ob[b], wbar[b])
            print("%s %d: mismatch of the device %.2e, of the reference %.2e, |w - w_oracle| %.1e" % (name, b, mg, mr, np.abs(_np(a["x"])[b] - c["w"][b]).max()))
            worst_ref, worst = max(worst_ref, mr), max(worst, mg)
    print("largest mismatch: device %.3e, reference %.3e, tolerance %.3e" % (worst, worst_ref, 10.0 * worst_ref))
    assert worst <= 10.0 * worst_ref, (worst, worst_ref)


# ---- the autograd layer
def _layer_instances(cfg, B, seed=7):
    """two robots far apart with goals a third of the horizon's reach ahead: no bound and no row is active at the solution"""
    rng = np.random.default_rng(seed)
    reach = cfg.v_max * cfg.T * cfg.N
    P = []
    for _ in range(B):
        s = Hh.sample_points(rng, cfg.m, cfg.dmin + 0.3, lim=0.5)
        th = rng.uniform(-np.pi, np.pi, cfg.m); ang = th + rng.uniform(-0.3, 0.3, cfg.m)
        g = s + (rng.uniform(0.2, 0.4, cfg.m) * reach)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        gth = th + rng.uniform(-0.05, 0.05, cfg.m)
        P.append(np.concatenate([np.concatenate([s, th[:, None]], 1).reshape(-1), np.concatenate([g, gth[:, None]], 1).reshape(-1)]))
    P = np.stack(P)
    return P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P])


def test_layer_gradients_are_the_direct_call_bit_for_bit():
    import nmpc_amd
    import torch
    c = AR.load_obs_cases()["two_static"]; cfg = c["cfg"]
    P, W0, obs = _fixture_batch(c)
    P = P.copy(); P[1, :2] = obs[1, 0, :2]      # instance 1: robot 0 starts on the obstacle, infeasible at stage 0 (status 3)
    W0 = np.stack([R.cold_start(cfg, q[: cfg.nx]) for q in P])
    s = _product_solver(cfg, 4)
    layer = nmpc_amd.NmpcLayer(s)
    d = s.device
    p = torch.tensor(P, dtype=torch.float64, device=d, requires_grad=True)
    ob = torch.tensor(obs, dtype=torch.float64, device=d, requires_grad=True)
    w0 = torch.tensor(W0, dtype=torch.float64, device=d, requires_grad=True)
    cvec = torch.tensor(np.stack([AR.cotangent(cfg, b) for b in range(4)]), dtype=torch.float64, device=d)
    w = layer(p, w0, obstacles=ob)
    (cvec * w).sum().backward()
    status = _np(layer.last["status"])
    assert status[1] == 3 and (np.delete(status, 1) == 0).all(), status
    assert set(layer.last) >= {"status", "iters", "kkt", "f", "info", "grad_dropped"}
    assert int(layer.last["grad_dropped"]) == 1
    assert w0.grad is None
    r = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    assert np.array_equal(_bits(_np(r["x"])), _bits(_np(w.detach())))
    ad = s.sens_adjoint_batch(P, r["x"], r["lam_g"], r["lam_x"], cvec, obstacles=obs)
    gp, go = _np(p.grad), _np(ob.grad)
    assert gp.shape == P.shape and go.shape == obs.shape
    for b in (0, 2, 3):
        assert np.array_equal(_bits(gp[b]), _bits(_np(ad["pbar"])[b])) and np.array_equal(_bits(go[b]), _bits(_np(ad["obsbar"])[b])), b
        assert gp[b].any() and go[b].any()
    assert not gp[1].any() and not go[1].any()
    # p alone: no obstacle gradient is asked for, the same bits
    p2 = torch.tensor(P, dtype=torch.float64, device=d, requires_grad=True)
    (cvec * layer(p2, w0.detach(), obstacles=torch.tensor(obs, dtype=torch.float64, device=d))).sum().backward()
    assert np.array_equal(_bits(_np(p2.grad)), _bits(gp))


def test_layer_needs_a_handle_with_multipliers():
    import nmpc_amd
    with pytest.raises(RuntimeError, match="multipliers"):
        nmpc_amd.NmpcLayer(_product_solver(R.cfg_two(8), 4, kernel=2))


def test_layer_gradient_against_central_differences():
    """d <c, w*> / d p_j for a few j by central differences of device re-solves at p +- h e_j, h = 5e-3, against the layer's gradient, relative to
    the largest difference quotient.  Tolerance: 10 x the disagreement of the CPU oracle's own central differences at h and h / 2 on the same
    instances and components — the truncation error of the quotient the gradient is held against (1.56e-6 on these instances, so 1.6e-5).
    Measured on MI355X: 2.1e-6."""
    import nmpc_amd
    import torch
    from oracle import oracle_lib as O
    cfg = R.cfg_two(8); h = 5e-3
    P, W0 = _layer_instances(cfg, 4)
    comps = [0, 2, cfg.nx + 1, cfg.nx + 3]
    cvec = np.random.default_rng(3).normal(size=cfg.n_var)
    O.build()
    oc = O.make_config(cfg, max_iter=2000)
    Wo = O.solve_batch(oc, P, W0)

    def oracle_cd(hh):
        out = np.zeros((len(P), len(comps)))
        for a, j in enumerate(comps):
            e = np.zeros(2 * cfg.nx); e[j] = hh
            out[:, a] = ((O.solve_batch(oc, P + e, Wo["x"])["x"] - O.solve_batch(oc, P - e, Wo["x"])["x"]) @ cvec) / (2 * hh)
        return out
    assert (Wo["status"] == 0).all()
    a, b = oracle_cd(h), oracle_cd(0.5 * h)
    tol = 10.0 * np.abs(a - b).max() / np.abs(b).max()
    s = _product_solver(cfg, 4)
    layer = nmpc_amd.NmpcLayer(s)
    p = torch.tensor(P, dtype=torch.float64, device=s.device, requires_grad=True)
    w = layer(p, torch.tensor(W0, dtype=torch.float64, device=s.device))
    (torch.tensor(cvec, device=s.device) * w).sum().backward()
    assert (_np(layer.last["status"]) == 0).all() and int(layer.last["grad_dropped"]) == 0
    lam = s.solve_batch(P, W0, want_duals=True)
    assert np.abs(_np(lam["lam_x"])).max() <= 1e-6 and np.abs(_np(lam["lam_g"])[:, S.ineq_rows(cfg)]).max() <= 1e-6      # unconstrained at the solution
    g = _np(p.grad)[:, comps]
    cd = np.zeros_like(g)
    for k, j in enumerate(comps):
        e = np.zeros(2 * cfg.nx); e[j] = h
        wp, wm = s.solve_batch(P + e, _np(w.detach())), s.solve_batch(P - e, _np(w.detach()))
        assert (_np(wp["status"]) == 0).all() and (_np(wm["status"]) == 0).all()
        cd[:, k] = ((_np(wp["x"]) - _np(wm["x"])) @ cvec) / (2 * h)
    err = np.abs(g - cd).max() / np.abs(cd).max()
    print("layer gradient against central differences: %.3e (tolerance %.3e; the oracle's quotients against the same gradient: %.3e)" % (
        err, tol, np.abs(g - b).max() / np.abs(b).max()))
    assert err <= tol, (err, tol)
