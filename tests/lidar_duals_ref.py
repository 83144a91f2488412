"""TEST INFRASTRUCTURE: numpy reference for the multipliers and the KKT certificate of the LIDAR NLP (nmpc_lidar_solve_batch_duals,
nmpc_lidar_kkt_batch; convention of include/nmpc_lidar.h: L = f + lam_g' g + lam_x' w + lam_p' p).

Everything is built from oracle/lidar_ref.py's grad_objective, jacobian, constraints and bounds: the Lagrangian gradient and the six
residuals, the stage-0 completion of lam_g, lam_p from its definition, least-squares multipliers on the active set (kkt_report's fit
returning its solution), and the derivative of the CPU oracle's optimal cost by central differences over re-solves: the check of lam_p
that needs no multiplier from anyone."""
import numpy as np

from oracle import lidar_ref as LR

NAMES = ("stat", "eq", "ineq", "bnd", "compl", "sign")
# rows (N, Nc, R, variant) of tests/lidar_variants.TABLE with B = 16, and the one two-wave row
ROWS = ((1, 1, 0, "base"), (3, 1, 2, "base"), (5, 2, 10, "base"), (9, 4, 5, "base"), (3, 1, 16, "lw0"), (9, 4, 5, "th2"), (9, 4, 5, "dmax_inf"),
        (9, 4, 5, "lw0_free"), (65, 32, 11, "base"), (64, 64, 10, "base"))
W2_ROW = (5, 2, 10, "base")
# the rows and instances on which the least-squares multipliers are unique and well conditioned and every re-solve converges
LSQ_ROWS = ((3, 1, 2, "base"), (5, 2, 10, "base"), (9, 4, 5, "base"), (9, 4, 5, "th2"))
LSQ_INSTANCES = (0, 2, 3)
FD_H = 1e-5


def row(key, two_wave=False):
    """the recipe of tests/lidar_variants.TABLE for (N, Nc, R, variant); two_wave: the row whose batch is the descriptor's threshold + 1"""
    from tests import lidar_variants as LV
    hits = [r for r in LV.TABLE if (r.N, r.Nc, r.R, r.over) == tuple(key) and (r.B is None) == two_wave]
    assert len(hits) == 1, (key, two_wave, hits)
    return hits[0]


def grad_lag(cfg, w, p, lam_g, lam_x):
    """grad f + J' lam_g + lam_x"""
    return LR.grad_objective(cfg, w, p) + LR.jacobian(cfg, w, p).T @ np.asarray(lam_g, float) + np.asarray(lam_x, float)


def residuals(cfg, w, p, lam_g, lam_x, lbx=None, ubx=None):
    """(res [6], grad_lag [n_var]) as include/nmpc_lidar.h defines them"""
    w = np.asarray(w, float).reshape(-1); lam_x = np.asarray(lam_x, float).reshape(-1)
    if lbx is None:
        lbx, ubx, _, _ = LR.bounds(cfg)
    gl = grad_lag(cfg, w, p, lam_g, lam_x)
    g = LR.constraints(cfg, w, p)
    has_lo, has_hi = np.isfinite(lbx), np.isfinite(ubx)
    neg, pos = np.where(lam_x > 0.0, 0.0, -lam_x), np.where(lam_x < 0.0, 0.0, lam_x)
    with np.errstate(invalid="ignore"):
        cl = np.where(has_lo, neg * (w - np.where(has_lo, lbx, 0.0)), 0.0)
        cu = np.where(has_hi, pos * (np.where(has_hi, ubx, 0.0) - w), 0.0)
    sg = np.concatenate([lam_x[has_lo & ~has_hi], -lam_x[has_hi & ~has_lo], [0.0]])
    top = lambda *a: float(np.max(np.concatenate([np.ravel(x) for x in a] + [[0.0]])))      # np.max: a NaN reaches the result
    res = np.array([top(np.abs(gl)), top(np.abs(g)), 0.0, top(lbx - w, w - ubx), top(cl, cu), top(sg)])
    return res, gl


def stage0_rows(cfg):
    """indices in g of the stage-0 rows: X_0[:3] - p[:3], then d_0 - scan"""
    return np.concatenate([np.arange(3), 3 * (cfg.N + 1) + np.arange(cfg.R)])


def complete_stage0(cfg, w, p, lam_g, lam_x=None):
    """lam_g with its stage-0 rows replaced by the values stationarity in X_0 gives them: the rows are an identity block in the 3 + R
    components of X_0, so they equal -(d f / d X_0 + sum over the other rows of lam_g,row d g_row / d X_0 + lam_x of X_0)"""
    out = np.array(lam_g, float)
    rows = stage0_rows(cfg)
    out[rows] = 0.0
    gl = grad_lag(cfg, w, p, out, np.zeros(cfg.n_var) if lam_x is None else lam_x)
    out[rows] = -gl[: cfg.ns]
    return out


def df_dp(cfg, w, p):
    X, _ = LR.unpack(cfg, w)
    out = np.zeros(cfg.n_p)
    out[3:6] = -2.0 * np.asarray(cfg.q) * (X[: cfg.N, :3] - np.asarray(p, float)[3:6]).sum(axis=0)
    return out


def dg_dp(cfg, w, p):
    """dense d g / d p, analytic (tests/test_lidar_duals_host.py holds it against central differences of lidar_ref.constraints)"""
    X, _ = LR.unpack(cfg, w)
    p = np.asarray(p, float).reshape(-1)
    N, R = cfg.N, cfg.R
    J = np.zeros((cfg.n_g, cfg.n_p))
    J[:3, :3] = -np.eye(3)
    go = 3 * (N + 1)
    po = LR.pobs(cfg, X[0], p)
    for m in range(R):
        J[go + m, 6 + m] = -1.0
        a = X[0, 2] + p[6 + R + m]
        for k in range(N):
            sx = np.sign(X[k + 1, 0] - po[m, 0]); sy = np.sign(X[k + 1, 1] - po[m, 1])
            J[go + R * (k + 1) + m, 6 + R + m] = sx * (-X[0, 3 + m] * np.sin(a)) + sy * (X[0, 3 + m] * np.cos(a))
    return J


def lam_p(cfg, w, p, lam_g):
    """-(d f / d p)' - (d g / d p)' lam_g"""
    return -df_dp(cfg, w, p) - dg_dp(cfg, w, p).T @ np.asarray(lam_g, float)


def lsq_multipliers(cfg, w, p, tol_active=1e-6):
    """lidar_ref.kkt_report's least-squares fit on the active set, returning its solution in the convention above: (lam_g, lam_x, stat)"""
    from scipy.optimize import lsq_linear
    w = np.asarray(w, float).reshape(-1)
    lbx, ubx, _, _ = LR.bounds(cfg)
    J = LR.jacobian(cfg, w, p); gf = LR.grad_objective(cfg, w, p)
    act_lb = np.where(w - lbx <= tol_active)[0]; act_ub = np.where(ubx - w <= tol_active)[0]
    E = np.zeros((w.size, act_lb.size + act_ub.size))
    for c, i in enumerate(act_lb): E[i, c] = -1.0
    for c, i in enumerate(act_ub): E[i, act_lb.size + c] = 1.0
    A = np.concatenate([J.T, E], axis=1)
    lo = np.concatenate([np.full(J.shape[0], -np.inf), np.zeros(E.shape[1])]); hi = np.full(A.shape[1], np.inf)
    sol = lsq_linear(A, -gf, bounds=(lo, hi), tol=1e-14, max_iter=500)
    lam_x = np.zeros(w.size)
    lam_x[act_lb] -= sol.x[J.shape[0]: J.shape[0] + act_lb.size]
    lam_x[act_ub] += sol.x[J.shape[0] + act_lb.size:]
    return sol.x[: J.shape[0]].copy(), lam_x, float(np.max(np.abs(A @ sol.x + gf)))


_ORACLE = {}


def oracle_points(key):
    """(cfg, P, W0, the CPU oracle's solve) of a row's recipe, once per process"""
    from tests import lidar_variants as LV
    if key not in _ORACLE:
        r = row(key)
        cfg, P, W0 = LV.inputs(r)
        _ORACLE[key] = (cfg, P, W0, LV.oracle_solve(cfg, P, W0, r.max_iter))
    return _ORACLE[key]


_DFDP = {}


def oracle_dfdp(key, b, h=FD_H):
    """d f* / d p [n_p] of instance b of a row: central differences of the CPU oracle's optimal cost under re-solves at p +- h e_i, warm-started
    at the oracle's own solution; every re-solve must converge.  Once per process."""
    from tests import lidar_variants as LV
    if (key, b, h) not in _DFDP:
        cfg, P, W0, sol = oracle_points(key)
        assert sol["status"][b] == 0
        n = cfg.n_p
        Pp = np.repeat(P[b][None], 2 * n, axis=0)
        Pp[np.arange(n), np.arange(n)] += h; Pp[n + np.arange(n), np.arange(n)] -= h
        out = LV.oracle_solve(cfg, Pp, np.repeat(sol["x"][b][None], 2 * n, axis=0), row(key).max_iter)
        assert (out["status"] == 0).all(), (key, b, out["status"])
        _DFDP[(key, b, h)] = (out["f"][:n] - out["f"][n:]) / (2.0 * h)
    return _DFDP[(key, b, h)]
