"""numpy side of the multiplier checks: the KKT residuals of a point w WITH GIVEN multipliers (lam_g, lam_x) in CasADi's convention
L = f + lam_g' g + lam_x' w (include/nmpc.h), built from oracle.nlp_ref (and tests.moving_obstacles_ref with an obstacle field).  Nothing is
fitted here: the multipliers are held to account as they are.  Shared by tests/test_duals_host.py and tests/test_gpu_duals.py."""
import numpy as np

from oracle import nlp_ref as R
from tests import moving_obstacles_ref as MO

NAMES = ("stat", "eq", "ineq", "bnd", "compl", "sign")


def functions(cfg, w, p, obs=None):
    """(g, J) of the NLP, with the per-stage obstacle field `obs` ([K, 3] or [N, K, 3]) when one is given"""
    if obs is None:
        return R.constraints(cfg, w, p), R.jacobian(cfg, w, p)
    return MO.constraints(cfg, w, p, obs), MO.jacobian(cfg, w, p, obs)


def residuals(cfg, w, p, lam_g, lam_x, obs=None):
    """(res [6], grad_lag [n_var]): grad_lag = grad f + J' lam_g + lam_x and
      stat   inf-norm of grad_lag
      eq     largest |g - lbg| over the equality rows                       (as nlp_ref.kkt_report)
      ineq   largest violation lbg - g of an inequality row, at least 0     (as nlp_ref.kkt_report)
      bnd    largest violation of a variable bound, at least 0              (as nlp_ref.kkt_report)
      compl  largest of |lam_g_i| (g_i - lbg_i) over the inequality rows, max(-lam_x_j, 0) (w_j - lbx_j) and max(lam_x_j, 0) (ubx_j - w_j)
             over the finite variable bounds, at least 0
      sign   largest positive lam_g on an inequality row (they are all bounded below only), at least 0"""
    w = np.asarray(w, float).reshape(-1); lam_g = np.asarray(lam_g, float).reshape(-1); lam_x = np.asarray(lam_x, float).reshape(-1)
    assert w.size == cfg.n_var and lam_g.size == cfg.n_g and lam_x.size == cfg.n_var
    lbx, ubx, lbg, ubg = R.bounds(cfg)
    g, J = functions(cfg, w, p, obs)
    grad = R.grad_objective(cfg, w, p) + J.T @ lam_g + lam_x
    eq = lbg == ubg
    ineq = ~eq
    assert np.isinf(ubg[ineq]).all()
    c = 0.0
    if ineq.any():
        c = max(0.0, float(np.max(np.abs(lam_g[ineq]) * (g[ineq] - lbg[ineq]))))
    fl, fu = np.isfinite(lbx), np.isfinite(ubx)
    c = max(c, float(np.max(np.maximum(-lam_x[fl], 0.0) * (w[fl] - lbx[fl]))), float(np.max(np.maximum(lam_x[fu], 0.0) * (ubx[fu] - w[fu]))))
    res = np.array([np.max(np.abs(grad)),
                    np.max(np.abs(g[eq] - lbg[eq])),
                    max(0.0, float(np.max(lbg[ineq] - g[ineq]))) if ineq.any() else 0.0,
                    max(0.0, float(np.max(lbx - w)), float(np.max(w - ubx))),
                    c,
                    max(0.0, float(np.max(lam_g[ineq]))) if ineq.any() else 0.0])
    return res, grad


def row_kinds(cfg):
    """index arrays of the rows of g: dict(init, pad, defect, pair0, obs0, pair, obs) — pair0 / obs0 are the pair / obstacle rows of stage 0
    (they act on the pinned X_0), pair / obs those of stages 1..N-1"""
    nx, M, mK = cfg.nx, cfg.M, cfg.m * cfg.K
    k = np.arange(cfg.N)[:, None] * cfg.rows_k + cfg.rows0
    defect = (k + np.arange(nx)[None]).reshape(-1)
    pair = k + nx + np.arange(M)[None]
    ob = k + nx + M + np.arange(mK)[None]
    return dict(init=np.arange(nx), pad=np.arange(nx, cfg.rows0), defect=defect, pair0=pair[0], obs0=ob[0],
                pair=pair[1:].reshape(-1), obs=ob[1:].reshape(-1))


def structural_zeros(cfg):
    """(rows of lam_g, entries of lam_x) that are zero by definition (include/nmpc.h): pad rows and the stage-0 pair / obstacle rows; X_0 and
    the headings without a bound"""
    rk = row_kinds(cfg)
    zg = np.concatenate([rk["pad"], rk["pair0"], rk["obs0"]]).astype(int)
    zx = list(range(cfg.nx))
    if not np.isfinite(cfg.th_max):
        zx += [k * cfg.nx + 3 * i + 2 for k in range(cfg.N + 1) for i in range(cfg.m)]
    return zg, np.array(sorted(set(zx)), dtype=int)


def lsq_multipliers(cfg, w, p, tol_active=1e-6, obs=None):
    """(lam_g, lam_x, active inequality rows): the least-squares multipliers of nlp_ref.kkt_report on the active set of w, scattered into
    CasADi's layout (inactive rows and bounds: 0)"""
    from scipy.optimize import lsq_linear
    w = np.asarray(w, float).reshape(-1)
    lbx, ubx, lbg, ubg = R.bounds(cfg)
    g, J = functions(cfg, w, p, obs)
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
    lo = np.concatenate([np.full(eq.size + act_g.size, -np.inf), np.zeros(E.shape[1])])
    hi = np.concatenate([np.full(eq.size, np.inf), np.zeros(act_g.size), np.full(E.shape[1], np.inf)])
    x = lsq_linear(A, -gf, bounds=(lo, hi), method="bvls", tol=1e-14).x
    lam_g = np.zeros(cfg.n_g); lam_x = np.zeros(cfg.n_var)
    lam_g[eq] = x[: eq.size]
    lam_g[act_g] = x[eq.size: eq.size + act_g.size]
    z = x[eq.size + act_g.size:]
    np.add.at(lam_x, act_lb, -z[: act_lb.size])
    np.add.at(lam_x, act_ub, z[act_lb.size:])
    return lam_g, lam_x, act_g
