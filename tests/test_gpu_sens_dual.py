"""-m gpu: nmpc_sens_update_batch_duals (csrc/nmpc_sens_dual.hip) and AdvancedStepController's update_duals / commit.

Every instantiation of sens_dual_kernel<MS> against tests/sens_dual_ref.py on the constructed points of tests/sens_points.py, with the point's dp
and the seeded dobs and rhs of tests/sens_update_ref.py: dlam_g, dlam_x and alpha_dual on every row, and stationarity (a) of include/nmpc.h
evaluated in numpy on the device's outputs.  The bounds are those of tests/test_sens_dual_host.py: 100 x that point's spread + 1e-12, relative to
max|dlam_g|, max|dlam_x| and to alpha_dual, and the same per stage block relative to the block's own maximum (tests/sens_dual_ref.stage_blocks:
the entries of the last stages are small beside max|dlam|); the identity's carries 1e-10 for its central differences.  Then the bit-level properties (dw, alpha and
info are those of nmpc_sens_update_batch; every output alone), the verdict batches, the argument errors, and on the instances of
tests/golden/sens_update_cases.npz the certificate, the chained correction and the sensitivity calls at the corrected point."""
import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import sens_dual_ref as DR
from tests import sens_points as SP
from tests import sens_update_ref as UR

pytestmark = pytest.mark.gpu

ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
OUT = ("dw", "alpha", "dlam_g", "dlam_x", "alpha_dual")
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


def _raw(s, r, pts, dps, dobs, rhs, want):
    """the C call itself with the outputs named in `want` and NULL for the others, every output between guard bands (tests/helpers.guarded_call:
    nothing written outside, every element written, a second call the same bits): {name: array}, info included"""
    import torch
    B = len(pts); cfg = r.cfg
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=s.device)
    ptr = lambda x: None if x is None else x.data_ptr()
    obs = t(np.stack([pt.obs for pt in pts])) if r.field else None
    S_ = 0 if obs is None else (1 if obs.dim() == 3 else cfg.N)
    a = [t(np.stack([getattr(pt, k) for pt in pts])) for k in ("p", "w", "lam_g", "lam_x")]
    dp_, do_, rh_ = t(_stack(dps)), t(_stack(dobs)), t(_stack(rhs))
    size = dict(dw=B * cfg.n_var, alpha=B, dlam_g=B * cfg.n_g, dlam_x=B * cfg.n_var, alpha_dual=B)
    outs = {k: (size[k], "f8") for k in want}
    outs["info"] = (B, "i4")

    def call(p):
        return s.lib.nmpc_sens_update_batch_duals(s._h, B, ptr(a[0]), ptr(obs), S_, ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(dp_), ptr(do_), ptr(rh_), p.get("dw"),
                                                  p.get("alpha"), p.get("dlam_g"), p.get("dlam_x"), p.get("alpha_dual"), p["info"], s._stream())
    got = Hh.guarded_call(outs, a + [x for x in (obs, dp_, do_, rh_) if x is not None], call)
    return {k: (v.reshape(B, -1) if v.size > B else v) for k, v in got.items()}


def ran(i):
    """row i: its handle, the call on its points, the same batch reversed, the plain call, and the reference with its bounds per point — once per
    session"""
    if i in _CACHE:
        return _CACHE[i]
    r = ROWS[i]
    pts = SP.points(r); n = len(pts)
    dps = [pt.dp for pt in pts]
    dobs = [UR.row_dobs(r, k) for k in range(n)]
    rhs = [UR.row_rhs(r, k) for k in range(n)]
    s = _solver(r.cfg, 2 * n + 2)
    full = _call(s, r, pts, dps, dobs, rhs, want_duals=True)
    back = _call(s, r, pts[::-1], dps[::-1], dobs[::-1], rhs[::-1], want_duals=True)
    plain = _call(s, r, pts, dps, dobs, rhs)
    kw = [dict(dp=a, dobs=b, rhs=c) for a, b, c in zip(dps, dobs, rhs)]
    ref = [DR.stage_duals(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, **k) for pt, k in zip(pts, kw)]
    bd = [DR.bounds(DR.spread(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, **k)) for pt, k in zip(pts, kw)]
    _CACHE[i] = dict(row=r, pts=pts, dps=dps, dobs=dobs, rhs=rhs, kw=kw, n=n, solver=s, full=full, back=back, plain=plain, ref=ref, bd=bd)
    return _CACHE[i]


# ---- G1
@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_parity_against_numpy(i):
    o = ran(i); r = o["row"]; cfg = r.cfg; f = o["full"]
    assert f["dlam_g"].shape == (o["n"], cfg.n_g) and f["dlam_x"].shape == (o["n"], cfg.n_var) and f["alpha_dual"].shape == (o["n"],)
    worst = 0.0
    for b, pt in enumerate(o["pts"]):
        ref, bd = o["ref"][b], o["bd"][b]
        assert f["info"][b] == ref["info"] == 0, (b, f["info"][b], ref["info"])
        e = DR.parity(cfg, f["dlam_g"][b], f["dlam_x"][b], ref, bd)
        eg, ex = e["g"], e["x"]
        ea = abs(f["alpha_dual"][b] - ref["alpha_dual"]) / ref["alpha_dual"]
        res, scale = DR.identity(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, f["dw"][b], f["dlam_g"][b], f["dlam_x"][b], **o["kw"][b])
        print("%s %d: dlam_g %.2e (bound %.2e), dlam_x %.2e (%.2e), alpha_dual %.6g against %.6g: %.2e (%.2e), identity (a) %.2e of %.2e (%.2e)" % (
            SP.row_id(r), b, eg, bd["g"], ex, bd["x"], f["alpha_dual"][b], ref["alpha_dual"], ea, bd["a"], res / scale, scale, bd["ident"]))
        print("%s %d: per stage block, in units of the block's bound: dlam_g %s, dlam_x %s" % (
            SP.row_id(r), b, " ".join("%.3f" % v for v in e["gk"] / bd["gk"]), " ".join("%.3f" % v for v in e["xk"] / bd["xk"])))
        worst = max(worst, e["worst"], ea / bd["a"], res / scale / bd["ident"])
        assert eg <= bd["g"], (b, eg, bd["g"])
        assert e["worst"] <= 1.0, (b, e, bd)      # the whole outputs, and every stage block against its own maximum
        assert ex <= bd["x"], (b, ex, bd["x"])
        assert ea <= bd["a"], (b, ea, bd["a"])
        assert res <= bd["ident"] * scale, (b, res / scale, bd["ident"])
        assert 0.0 < f["alpha_dual"][b] <= 1.0
    print("%s: largest error %.3f of its bound" % (SP.row_id(r), worst))


# ---- G2
@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_same_bits_as_the_plain_call_reversed_repeated_and_per_output(i):
    """dw, alpha and info are those of nmpc_sens_update_batch; the reversed batch and a second call return the bits of the first; every output
    alone (the four others NULL, dw among them), and the call with all three multiplier outputs NULL, return the bits of the full call; the
    structural zeros are exact"""
    o = ran(i); r = o["row"]; cfg = r.cfg; f, k, pl = o["full"], o["back"], o["plain"]
    assert np.array_equal(pl["info"], f["info"]) and np.array_equal(k["info"][::-1], f["info"])
    for key in ("dw", "alpha"):
        assert np.array_equal(_bits(pl[key]), _bits(f[key])), key
    again = _call(o["solver"], r, o["pts"], o["dps"], o["dobs"], o["rhs"], want_duals=True)
    for key in OUT:
        assert np.array_equal(_bits(k[key][::-1]), _bits(f[key])), key
        assert np.array_equal(_bits(again[key]), _bits(f[key])), key
    for want in [(key,) for key in OUT] + [("dw", "alpha"), ()]:
        got = _raw(o["solver"], r, o["pts"], o["dps"], o["dobs"], o["rhs"], want)
        assert np.array_equal(got["info"], f["info"]), want
        for key in want:
            assert np.array_equal(_bits(got[key]), _bits(f[key])), (want, key)
    mg, mx = SP.null_masks(cfg)
    mg = mg.copy(); mg[: cfg.nx] = False      # the initial block carries dnu_init
    rows = DR.S.ineq_rows(cfg)
    for b, pt in enumerate(o["pts"]):
        g, x = f["dlam_g"][b], f["dlam_x"][b]
        assert not g[mg].any() and not x[mx].any() and g[: cfg.nx].any(), b
        assert not g[rows][pt.lam_g[rows] >= 0.0].any() and not x[pt.lam_x == 0.0].any(), b
        assert not np.signbit(g[g == 0.0]).any() and not np.signbit(x[x == 0.0]).any(), b


# ---- G3
@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_in_a_mixed_batch(r):
    """each verdict case is one instance between clean points: its dlam are zeros and alpha_dual = 0, and its neighbours keep the bits of the parity
    call"""
    i = ROWS.index(r)
    o = ran(i); cfg = r.cfg
    cases = SP.verdict_cases(r, o["pts"][0])[1:]
    batch, dps, dobs, rhs, clean = [], [], [], [], []
    for c, (name, pt, want) in enumerate(cases):
        a = c % o["n"]; clean.append(a)
        batch += [o["pts"][a], pt]
        dps += [o["dps"][a], pt.dp]; dobs += [o["dobs"][a], o["dobs"][0]]; rhs += [o["rhs"][a], o["rhs"][0]]
    s = _solver(cfg, len(batch))
    got = _call(s, r, batch, dps, dobs, rhs, want_duals=True)
    for c, (name, pt, want) in enumerate(cases):
        b = 2 * c + 1
        kw = dict(dp=pt.dp, dobs=o["dobs"][0], rhs=o["rhs"][0])
        ref = DR.stage_duals(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, **kw)
        assert got["info"][b] == ref["info"] == want, (name, got["info"][b], ref["info"], want)
        if want:
            assert not got["dlam_g"][b].any() and not got["dlam_x"][b].any() and got["alpha_dual"][b] == 0.0, name
            assert not got["dw"][b].any() and got["alpha"][b] == 0.0, name
        else:      # the pair row of the wrong sign: no Sigma and no multiplier step on it, its Hessian term stays in
            bd = DR.bounds(DR.spread(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, **kw))
            e = DR.parity(cfg, got["dlam_g"][b], got["dlam_x"][b], ref, bd)
            ea = abs(got["alpha_dual"][b] - ref["alpha_dual"]) / ref["alpha_dual"]
            print("%s: dlam_g %.2e (%.2e), dlam_x %.2e (%.2e), alpha_dual %.2e (%.2e), worst measure %.3f of its bound" % (
                name, e["g"], bd["g"], e["x"], bd["x"], ea, bd["a"], e["worst"]))
            assert e["g"] <= bd["g"] and e["x"] <= bd["x"] and ea <= bd["a"] and e["worst"] <= 1.0, name
        a = clean[c]
        assert got["info"][2 * c] == 0
        for key in OUT:
            assert np.array_equal(_bits(got[key][2 * c]), _bits(o["full"][key][a])), (name, key)


# ---- G4
def test_argument_errors_and_unsupported_kernels():
    import torch
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); o = ran(ROWS.index(r)); cfg = r.cfg; s = o["solver"]
    B = 2
    d = s.device
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=d)
    p, w, lg, lx, dp, rh, dw, al = t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_g), t(B, cfg.n_var), t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_var), t(B)
    dg, dx, ad = t(B, cfg.n_g), t(B, cfg.n_var), t(B)
    ob, dob = t(B, cfg.N, cfg.K, 3), t(B, cfg.N, cfg.K, 3)
    info = torch.zeros(B, dtype=torch.int32, device=d)
    ptr = lambda x: None if x is None else x.data_ptr()

    def raw(B_, p_, obs_, S_, w_, lg_, lx_, dp_, dob_, rh_, dw_, al_, info_):
        return s.lib.nmpc_sens_update_batch_duals(s._h, B_, ptr(p_), ptr(obs_), S_, ptr(w_), ptr(lg_), ptr(lx_), ptr(dp_), ptr(dob_), ptr(rh_), ptr(dw_),
                                                  ptr(al_), ptr(dg), ptr(dx), ptr(ad), ptr(info_), s._stream())
    assert raw(B, p, None, 0, w, lg, lx, dp, dob, rh, dw, al, info) == -1      # dobs without obs
    for k in range(4):      # null p, w, lam_g, lam_x: the multiplier outputs need them as every output does
        a = [p, w, lg, lx]; a[k] = None
        assert raw(B, a[0], ob, cfg.N, a[1], a[2], a[3], dp, dob, rh, dw, al, info) == -1, k
        assert raw(B, a[0], ob, cfg.N, a[1], a[2], a[3], dp, dob, rh, None, None, info) == -1, k
    assert raw(B, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, None) == -1
    assert raw(B, p, ob, 2, w, lg, lx, dp, dob, rh, dw, al, info) == -1              # obs_stages neither 1 nor N
    assert raw(B, p, None, cfg.N, w, lg, lx, dp, None, rh, dw, al, info) == -1       # obs_stages without a field
    assert raw(s.max_batch + 1, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, info) == -1
    assert raw(-1, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, info) == -1
    assert raw(0, None, None, 0, None, None, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    for pin in (1, 2):
        k = _product_solver(R.cfg_two(8), 4, kernel=pin)
        assert k.lib.nmpc_sens_update_batch_duals(k._h, 0, None, None, 0, *([None] * 13)) == -2
    with pytest.raises(ValueError):
        s.sens_update_batch(_np(p), _np(w), _np(lg), _np(lx), dobs=_np(dob), want_duals=True)


# ---- on a solve's own output: tests/golden/sens_update_cases.npz (4 instances per configuration, their dx, d and h = H_UPD)
NAMES = list(UR.load_cases())
MARGIN = 10.0      # the device against the reference at the oracle's own point: the margin of the sibling end-to-end tests (tests/test_gpu_sens_update.py)
_E2E = {}


def _fixture_batch(c):
    cfg = c["cfg"]
    return c["p"], np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in c["p"]]), c["obs"]


def _e2e(name):
    """one configuration, once per session: the device's solve with multipliers, the update with multipliers along the unit direction (dx, d),
    max(stat, eq) of kkt_batch along it, and the reference's screens"""
    if name in _E2E:
        return _E2E[name]
    import torch
    c = UR.load_cases()[name]; cfg = c["cfg"]; h = c["h"]
    P, W0, obs = _fixture_batch(c)
    s = _product_solver(cfg, 4)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=s.device)
    a = s.solve_batch(P, W0, obstacles=obs, want_duals=True)
    dp = np.stack([UR.case_dp(cfg, dx) for dx in c["dx"]])
    up = s.sens_update_batch(P, a["x"], a["lam_g"], a["lam_x"], dp=dp, dobs=c["d"], obstacles=obs, want_duals=True)
    assert (_np(a["status"]) == 0).all() and (_np(up["info"]) == 0).all(), name

    def kkt(step, duals):
        """max(stat, eq) [4] at (p + step dp, obs + step d) with (w + step dw, lam + step dlam or lam)"""
        sd = step if duals else 0.0
        res = s.kkt_batch(t(P) + step * t(dp), a["x"] + step * up["dw"], a["lam_g"] + sd * up["dlam_g"], a["lam_x"] + sd * up["dlam_x"], obstacles=t(obs) + step * t(c["d"]))
        return _np(res)[:, :2].max(axis=1)
    base = kkt(0.0, True)
    out = dict(c=c, cfg=cfg, h=h, solver=s, P=P, W0=W0, obs=obs, dp=dp, sol=a, up=up, base=base, r_h=kkt(h, True) - base, r_h2=kkt(0.5 * h, True) - base,
               r_old=kkt(h, False) - base, cert=[DR.screen_certificate(c, b) for b in range(4)], chain=[DR.screen_chain(c, b) for b in range(4)])
    _E2E[name] = out
    return out


# ---- G5
def test_certificate_is_second_order_with_the_updated_multipliers():
    """r(h): the increase of max(stat, eq) of nmpc_kkt_batch at (p + h dp, obs + h d) with (w + h dw, lam + h dlam) over its value at h = 0.  On the
    instances whose reference ratio r(h) / r(h/2) lies in [3.5, 4.5] (tests/sens_dual_ref.screen_certificate; at least 3 of 4 per configuration)
    the device's ratio lies within 10 x the reference's largest deviation from 4, and r(h) is smaller than the same quantity with the old
    multipliers — a first-order residual — by at least a tenth of the reference's smallest factor.
    Measured: see DESIGN.md section 5."""
    dev_ref, dev_gpu, fac_ref, fac_gpu = 0.0, 0.0, np.inf, np.inf
    for name in NAMES:
        o = _e2e(name)
        assert sum(x["keep"] for x in o["cert"]) >= 3, name
        for b, x in enumerate(o["cert"]):
            ratio = o["r_h"][b] / o["r_h2"][b]
            print("%s %d: device r(h) %.2e r(h/2) %.2e ratio %.3f, old multipliers %.2e (x %.1f), at h = 0 %.1e | reference ratio %.3f, x %.1f%s" % (
                name, b, o["r_h"][b], o["r_h2"][b], ratio, o["r_old"][b], o["r_old"][b] / o["r_h"][b], o["base"][b], x["ratio"], x["r_old"] / x["r_h"],
                "" if x["keep"] else " (dropped)"))
            if not x["keep"]:
                continue
            dev_ref, dev_gpu = max(dev_ref, abs(x["ratio"] - 4.0)), max(dev_gpu, abs(ratio - 4.0))
            fac_ref, fac_gpu = min(fac_ref, x["r_old"] / x["r_h"]), min(fac_gpu, o["r_old"][b] / o["r_h"][b])
            assert 0.0 < o["r_h"][b] < o["r_old"][b], (name, b)
    print("largest |ratio - 4|: device %.3f, reference %.3f; smallest factor over the old multipliers: device %.1f, reference %.1f" % (dev_gpu, dev_ref, fac_gpu, fac_ref))
    assert dev_gpu <= MARGIN * dev_ref, (dev_gpu, dev_ref)
    assert fac_gpu >= fac_ref / MARGIN, (fac_gpu, fac_ref)


# ---- G6
def test_chained_correction_relinearises_midway():
    """correct to h / 2 with commit=True, then correct to h, against one correct to h, both against the oracle's re-solve w(h).  On the instances
    where the chained plan is closer on the reference (tests/sens_dual_ref.screen_chain; at least 3 of 4 per configuration) the device's largest
    error is within 10 x the reference's, for either plan, and its chained plan is the closer one there too.  commit=False leaves the base
    untouched, and with both flags off the dict is today's, bit for bit.  Measured: see DESIGN.md section 5."""
    import nmpc_amd
    import torch
    worst = dict(single=0.0, chained=0.0, single_ref=0.0, chained_ref=0.0)
    for name in NAMES:
        o = _e2e(name); c, cfg, h, s = o["c"], o["cfg"], o["h"], o["solver"]
        assert sum(x["keep"] for x in o["chain"]) >= 3, name
        P, obs = o["P"], o["obs"]
        at = lambda f: (P[:, : cfg.nx] + f * h * c["dx"], obs + f * h * c["d"])
        ctl = nmpc_amd.AdvancedStepController(s)
        pre = ctl.prepare(P, o["W0"], obstacles=obs)
        x1, o1 = at(1.0)
        one = ctl.correct(x1, obstacles=o1)
        # flags off: today's dict — the direct call with the controller's own differences
        t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=s.device)
        dp = torch.zeros((4, 2 * cfg.nx), dtype=torch.float64, device=s.device)
        dp[:, : cfg.nx] = t(x1) - t(P)[:, : cfg.nx]
        direct = s.sens_update_batch(P, pre["x"], pre["lam_g"], pre["lam_x"], dp=dp, dobs=t(o1) - t(obs), obstacles=obs)
        step = torch.where(direct["alpha"] == 1.0, direct["alpha"], 0.99 * direct["alpha"])
        assert set(one) == {"w", "u0", "step", "alpha", "info", "corrected"}
        assert np.array_equal(_bits(_np(one["w"])), _bits(_np(pre["x"] + step[:, None] * direct["dw"]))) and np.array_equal(_np(one["step"]), _np(step))
        # commit=False leaves the base untouched: the same object, the same bits, the same correction afterwards
        plan = ctl._plan
        saved = {k: (None if v is None else v.clone()) for k, v in plan.items()}
        dual = ctl.correct(x1, obstacles=o1, update_duals=True)
        assert ctl._plan is plan and all(torch.equal(plan[k], saved[k]) for k in saved)
        again = ctl.correct(x1, obstacles=o1)
        for key in one:
            assert torch.equal(again[key], one[key]), key
        assert {"lam_g", "lam_x", "alpha_dual"} <= set(dual) and _np(dual["corrected"]).all()
        # the chain
        xh, oh = at(0.5)
        half = ctl.correct(xh, obstacles=oh, commit=True)
        assert ctl._plan is not plan and np.array_equal(_bits(_np(ctl._plan["w"])), _bits(_np(half["w"])))
        two = ctl.correct(x1, obstacles=o1, update_duals=True)
        assert _np(half["corrected"]).all() and _np(two["corrected"]).all(), (name, _np(half["info"]), _np(two["info"]))
        w1, w2 = _np(one["w"]), _np(two["w"])
        for b, x in enumerate(o["chain"]):
            e1, e2 = np.abs(w1[b] - c["w_h"][b]).max(), np.abs(w2[b] - c["w_h"][b]).max()
            print("%s %d: |w - w(h)| single %.2e chained %.2e (steps %.3f then %.3f) | reference single %.2e chained %.2e%s" % (
                name, b, e1, e2, _np(half["step"])[b], _np(two["step"])[b], x["single"], x["chained"], "" if x["keep"] else " (dropped)"))
            if x["keep"]:
                worst = dict(single=max(worst["single"], e1), chained=max(worst["chained"], e2), single_ref=max(worst["single_ref"], x["single"]),
                             chained_ref=max(worst["chained_ref"], x["chained"]))
    print("largest |w - w(h)|: device single %.3e chained %.3e, reference single %.3e chained %.3e" % (worst["single"], worst["chained"], worst["single_ref"], worst["chained_ref"]))
    assert worst["single"] <= MARGIN * worst["single_ref"] and worst["chained"] <= MARGIN * worst["chained_ref"], worst
    assert worst["chained"] < worst["single"], worst


# ---- G7
def test_sensitivity_calls_run_at_the_corrected_primal_dual_point():
    """nmpc_sens_batch at (p + h dp, obs + h d) with the corrected (w, lam_g, lam_x) of one correct(update_duals=True): info == 0 on the instances
    of the certificate, without a re-solve"""
    import nmpc_amd
    for name in NAMES:
        o = _e2e(name); c, cfg, h, s = o["c"], o["cfg"], o["h"], o["solver"]
        P, obs = o["P"], o["obs"]
        ctl = nmpc_amd.AdvancedStepController(s)
        ctl.prepare(P, o["W0"], obstacles=obs)
        x1, o1 = P[:, : cfg.nx] + h * c["dx"], obs + h * c["d"]
        out = ctl.correct(x1, obstacles=o1, update_duals=True)
        Pm = P.copy(); Pm[:, : cfg.nx] = x1
        step = _np(out["step"])
        sens = s.sens_batch(Pm, out["w"], out["lam_g"], out["lam_x"], dp=o["dp"], gains=1, obstacles=o1)
        info = _np(sens["info"])
        print("%s: steps %s, info at the corrected point %s" % (name, step, info))
        for b, x in enumerate(o["cert"]):
            if x["keep"]:
                assert step[b] == 1.0 and info[b] == 0 and _np(sens["dw"])[b].any(), (name, b, step[b], info[b])
