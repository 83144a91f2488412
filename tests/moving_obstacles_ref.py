"""Independent restatement of the NLP with a per-instance, per-stage obstacle field (the *_obs entry points): oracle.nlp_ref computes
everything, and only the obstacle rows of g and J are replaced — stage k's rows measure X_k against entry k of the field, (ox, oy, r) per
obstacle.  `obs` is [K, 3] (a static field) or [N, K, 3]."""
import numpy as np

from oracle import nlp_ref as R


def field(cfg, obs):
    """[N, K, 3] per-stage view of a field given as [K, 3] or [N, K, 3]"""
    o = np.asarray(obs, dtype=np.float64)
    if o.ndim == 2:
        o = np.broadcast_to(o, (cfg.N,) + o.shape)
    assert o.shape == (cfg.N, cfg.K, 3), o.shape
    return o


def obstacle_row(cfg, k, i, q):
    """row of g of obstacle q and robot i at stage k (robot-major inside the stage block, after the defect and pair rows)"""
    return cfg.rows0 + k * cfg.rows_k + cfg.nx + cfg.M + i * cfg.K + q


def constraints(cfg, w, p, obs):
    g = R.constraints(cfg, w, p)
    X, _ = R.unpack(cfg, w)
    o = field(cfg, obs)
    for k in range(cfg.N):
        st = X[k]
        for i in range(cfg.m):
            for q in range(cfg.K):
                ox, oy, orad = o[k, q]
                g[obstacle_row(cfg, k, i, q)] = np.sqrt((st[3 * i] - ox) ** 2 + (st[3 * i + 1] - oy) ** 2) - cfg.rob_dim - orad
    return g


def jacobian(cfg, w, p, obs):
    J = R.jacobian(cfg, w, p)
    X, _ = R.unpack(cfg, w)
    o = field(cfg, obs)
    for k in range(cfg.N):
        st, xc = X[k], k * cfg.nx
        for i in range(cfg.m):
            for q in range(cfg.K):
                ox, oy, _ = o[k, q]
                r = obstacle_row(cfg, k, i, q)
                dx = st[3 * i] - ox; dy = st[3 * i + 1] - oy
                rr = np.sqrt(dx * dx + dy * dy)
                J[r, :] = 0.0
                J[r, xc + 3 * i] = dx / rr; J[r, xc + 3 * i + 1] = dy / rr
    return J


def kkt_report(cfg, w, p, obs, tol_active=1e-6):
    """R.kkt_report with these g and J: least-squares multipliers on the active set -> inf-norms of the stationarity residual, equality
    violation, inequality violation, bound violation"""
    from scipy.optimize import lsq_linear
    w = np.asarray(w, float).reshape(-1)
    lbx, ubx, lbg, ubg = R.bounds(cfg)
    g = constraints(cfg, w, p, obs)
    J = jacobian(cfg, w, p, obs)
    gf = R.grad_objective(cfg, w, p)
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


def obstacle_values(cfg, w, obs):
    """[N, m, K] g of the obstacle rows (without the margin: the rows are bounded below by it)"""
    X = np.asarray(w, float).reshape(-1)[: cfg.nx * (cfg.N + 1)].reshape(cfg.N + 1, cfg.nx)
    o = field(cfg, obs)
    xy = X[: cfg.N].reshape(cfg.N, cfg.m, 3)[:, :, None, :2]
    return np.linalg.norm(xy - o[:, None, :, :2], axis=3) - cfg.rob_dim - o[:, None, :, 2]
