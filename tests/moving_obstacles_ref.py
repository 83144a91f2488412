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


def team_cfg(m, N, K, **kw):
    """a team of m robots with K obstacle rows (their values come from the field), at the literals of the scripts that have one: the third
    scenario's for one robot (T = 0.2), C6's for 2..6 (T = 0.3), C10's beyond (T = 0.1)"""
    base = dict(T=0.3, dmin=0.4, v_max=0.15, w_max=1.5) if m <= 6 else dict(T=0.1, dmin=0.3, v_max=0.22, w_max=2.84)
    if m == 1:
        base = dict(T=0.2, dmin=0.0, v_max=0.2, w_max=1.0, pad_rows=False)
    base.update(kw)
    return R.NLPConfig(m=m, N=N, obstacles=[(0.0, 0.0, 0.1)] * K, rob_dim=0.2, margin=0.1, **base)


def moving_batch(cfg, B, seed, L=None):
    """B instances of cfg (any m, K, N) among K obstacles of their own, crossing the workspace at constant velocity (speed <= v_max / 2) with
    the radius growing by <= 50 % over the L rows of the field (L = N: a per-stage solve field; L > N: closed-loop paths, row t = period t);
    starts clear of every obstacle's row 0 — at its largest radius — by more than the margin, goals likewise of its last row.
    Returns P [B, 2 n_x], the cold starts W0 [B, n_var] and the fields [B, L, K, 3]."""
    from tests import helpers as Hh
    rng = np.random.default_rng(seed)
    N, K, T = cfg.N, cfg.K, cfg.T
    L = N if L is None else L
    k = np.arange(L)[:, None]
    P, F = [], []
    for _ in range(B):
        c0 = rng.uniform(-1.5, 1.5, (K, 2))
        ang = rng.uniform(-np.pi, np.pi, K); spd = rng.uniform(0.2, 0.5, K) * cfg.v_max
        vel = np.stack([np.cos(ang), np.sin(ang)], axis=1) * spd[:, None]
        r0 = rng.uniform(0.1, 0.15, K); grow = rng.uniform(0.0, 0.5, K)
        f = np.empty((L, K, 3))
        f[:, :, :2] = c0[None] + (k * T)[:, :, None] * vel[None]
        f[:, :, 2] = r0[None] * (1.0 + grow[None] * k / max(L - 1, 1))
        clear = cfg.rob_dim + cfg.margin + 0.1
        s = Hh.sample_points(rng, cfg.m, cfg.dmin + 0.1, obstacles=[(x, y, r) for x, y, r in zip(f[0, :, 0], f[0, :, 1], f[-1, :, 2])], clear=clear)
        g = Hh.sample_points(rng, cfg.m, cfg.dmin + 0.1, obstacles=[(x, y, r) for x, y, r in f[-1]], clear=clear)
        x0 = np.concatenate([s, rng.uniform(-np.pi, np.pi, (cfg.m, 1))], axis=1).reshape(-1)
        xs = np.concatenate([g, rng.uniform(-np.pi, np.pi, (cfg.m, 1))], axis=1).reshape(-1)
        P.append(np.concatenate([x0, xs])); F.append(f)
    P = np.stack(P)
    return P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P]), np.stack(F)
