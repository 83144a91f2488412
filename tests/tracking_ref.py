"""Independent restatement of the NLP with a pose reference per stage (the *_ref entry points): oracle.nlp_ref computes everything, and only
the cost is replaced — stage k (k = 0..N-1) measures X_k against row k of `ref`, sum_k (X_k - ref_k)' Q (X_k - ref_k) + U_k' R U_k.  `ref` is
[n_x] (one row for the horizon: oracle.nlp_ref's cost with xs = ref) or [N, n_x].  The xs half of p is not read."""
import numpy as np

from oracle import nlp_ref as R


def rows(cfg, ref):
    """[N, n_x] per-stage view of a reference given as [n_x] or [N, n_x]"""
    r = np.asarray(ref, dtype=np.float64)
    if r.ndim == 1:
        r = np.broadcast_to(r, (cfg.N,) + r.shape)
    assert r.shape == (cfg.N, cfg.nx), r.shape
    return r


def objective(cfg, w, ref) -> float:
    X, U = R.unpack(cfg, w)
    qd = np.tile(np.asarray(cfg.q, float), cfg.m)
    rd = np.tile(np.asarray(cfg.r, float), cfg.m)
    e = X[: cfg.N] - rows(cfg, ref)
    return float(np.sum(e * e * qd) + np.sum(U * U * rd))


def grad_objective(cfg, w, ref) -> np.ndarray:
    X, U = R.unpack(cfg, w)
    qd = np.tile(np.asarray(cfg.q, float), cfg.m)
    rd = np.tile(np.asarray(cfg.r, float), cfg.m)
    gX = np.zeros_like(X)
    gX[: cfg.N] = 2.0 * qd * (X[: cfg.N] - rows(cfg, ref))
    return R.pack(cfg, gX, 2.0 * rd * U)


def kkt_report(cfg, w, p, ref, tol_active=1e-6):
    """R.kkt_report with this gradient: least-squares multipliers on the active set -> inf-norms of the stationarity residual, equality
    violation, inequality violation, bound violation (g and J do not depend on the reference)"""
    from scipy.optimize import lsq_linear
    w = np.asarray(w, float).reshape(-1)
    lbx, ubx, lbg, ubg = R.bounds(cfg)
    g = R.constraints(cfg, w, p)
    J = R.jacobian(cfg, w, p)
    gf = grad_objective(cfg, w, ref)
    eq = np.where(lbg == ubg)[0]
    ineq = np.where(lbg != ubg)[0]
    act_g = ineq[(g[ineq] - lbg[ineq]) <= tol_active]
    act_lb = np.where(w - lbx <= tol_active)[0]
    act_ub = np.where(ubx - w <= tol_active)[0]
    E = np.zeros((w.size, act_lb.size + act_ub.size))
    for c, i in enumerate(act_lb): E[i, c] = -1.0
    for c, i in enumerate(act_ub): E[i, act_lb.size + c] = 1.0
    A = np.concatenate([J[eq].T, J[act_g].T, E], axis=1)
    lo = np.concatenate([np.full(eq.size, -np.inf), np.full(act_g.size, -np.inf), np.zeros(E.shape[1])])
    hi = np.concatenate([np.full(eq.size, np.inf), np.zeros(act_g.size), np.full(E.shape[1], np.inf)])
    res = lsq_linear(A, -gf, bounds=(lo, hi), method="bvls", tol=1e-14)      # exact active-set solve (a few hundred columns)
    stat = float(np.max(np.abs(A @ res.x + gf))) if A.shape[1] else float(np.max(np.abs(gf)))
    return dict(stat=stat, eq=float(np.max(np.abs(g[eq] - lbg[eq]))),
                ineq=float(max(0.0, np.max(lbg[ineq] - g[ineq]))) if ineq.size else 0.0,
                bnd=float(max(0.0, np.max(lbx - w), np.max(w - ubx))))


def slsqp(cfg, p, ref, w0, maxiter=1000):
    """scipy-SLSQP on the restatement, by the recipe of tests/golden/gen_golden.py (ftol 1e-14)"""
    from scipy.optimize import Bounds, minimize
    lbx, ubx, lbg, ubg = R.bounds(cfg)
    eq = np.where(lbg == ubg)[0]; iq = np.where(lbg != ubg)[0]
    cons = [{"type": "eq", "fun": lambda w: R.constraints(cfg, w, p)[eq] - lbg[eq], "jac": lambda w: R.jacobian(cfg, w, p)[eq]}]
    if iq.size:
        cons.append({"type": "ineq", "fun": lambda w: R.constraints(cfg, w, p)[iq] - lbg[iq], "jac": lambda w: R.jacobian(cfg, w, p)[iq]})
    return minimize(lambda w: objective(cfg, w, ref), w0, jac=lambda w: grad_objective(cfg, w, ref), bounds=Bounds(lbx, ubx),
                    constraints=cons, method="SLSQP", options={"ftol": 1e-14, "maxiter": maxiter})


def line_path(cfg, start, vel, L, hold_from=None):
    """[L, n_x]: row t = start + min(t, hold_from) T vel (a constant-velocity path in (x, y, theta) per robot, held from row hold_from on)"""
    t = np.arange(L, dtype=np.float64)
    if hold_from is not None:
        t = np.minimum(t, float(hold_from))
    return np.asarray(start, float)[None, :] + (t * cfg.T)[:, None] * np.asarray(vel, float)[None, :]


# ---- the fixtures of tests/golden/slsqp_track.npz -------------------------------------------------------------------------------------------
OBSTACLES2 = [(0.45, 0.1, 0.15), (-0.3, 0.5, 0.125)]      # the two obstacles of helpers.cfg_mix3


def families():
    """name -> NLPConfig of the fixture families"""
    lit = dict(T=0.3, dmin=0.4, v_max=0.15, w_max=1.5)
    one = dict(m=1, T=0.2, dmin=0.0, v_max=0.2, w_max=1.0, pad_rows=False)
    return {"one": R.NLPConfig(N=8, **one),
            "two": R.NLPConfig(m=2, N=8, **lit),
            "three": R.NLPConfig(m=3, N=6, **lit),
            "one_obs": R.NLPConfig(N=8, obstacles=OBSTACLES2, rob_dim=0.2, margin=0.1, **one),
            "one_thb": R.NLPConfig(N=8, th_max=3.5, **one)}


def family_inputs(name, cfg, count=3):
    """(P [count, 2 n_x], REF [count, N, n_x], W0) of a family: starts as helpers.instance (clear of each other and of the obstacles); the
    path of every robot starts at an offset of up to 0.15 from the robot (heading up to 0.3 rad) and moves at a constant velocity of
    0.3 .. 0.8 v_max along its own heading, which it keeps.  The xs half of P is NaN: nothing may read it."""
    from tests import helpers as Hh
    rng = np.random.Generator(np.random.PCG64(Hh.SEED0 + 4242 + sum(map(ord, name))))
    P, REF = [], []
    for _ in range(count):
        x0 = Hh.instance(rng, cfg)[: cfg.nx].reshape(cfg.m, 3)
        s = x0 + np.concatenate([rng.uniform(-0.15, 0.15, (cfg.m, 2)), rng.uniform(-0.3, 0.3, (cfg.m, 1))], axis=1)
        if np.isfinite(cfg.th_max):
            s[:, 2] = np.clip(s[:, 2], -cfg.th_max + 0.5, cfg.th_max - 0.5)
        spd = rng.uniform(0.3, 0.8, cfg.m) * cfg.v_max
        vel = np.stack([spd * np.cos(s[:, 2]), spd * np.sin(s[:, 2]), np.zeros(cfg.m)], axis=1)
        REF.append(line_path(cfg, s.reshape(-1), vel.reshape(-1), cfg.N))
        P.append(np.concatenate([x0.reshape(-1), np.full(cfg.nx, np.nan)]))
    P = np.stack(P)
    return P, np.stack(REF), np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P])

