"""numpy side of the plan-sensitivity checks (nmpc_sens_batch, include/nmpc.h): the linearisation of the solver's barrier KKT system at a given
primal-dual point (p, w, lam_g, lam_x), built from oracle.nlp_ref (and tests.moving_obstacles_ref with an obstacle field).

  kkt_system       dense W and the linearised equality rows, by the definition in include/nmpc.h
  dense_sens       one dense solve (LU, refined) of the bordered system (the whole horizon, or the tail from stage k0 with X_k0 given)
  dense_gains      G_k = dU_k / dX_k of every tail problem, from dense_sens
  stage_recursion  the same by the stage recursion the kernel runs: gains, affine terms, dw, info
  spread           the recursion against itself with w, lam_g, lam_x moved by +-4 ulp: the conditioning of the definition at that point

Shared by tests/test_sens_host.py, tests/test_gpu_sens.py and tests/golden/gen_sens_cases.py."""
import numpy as np

from oracle import nlp_ref as R
from tests import moving_obstacles_ref as MO

INFO_OK, INFO_INDEFINITE, INFO_INFEASIBLE = 0, 1, 2


def ineq_rows(cfg):
    """rows of g that carry a barrier term: the pair and obstacle rows of stages 1..N-1"""
    k = np.arange(1, cfg.N)[:, None] * cfg.rows_k + cfg.rows0 + cfg.nx
    return (k + np.arange(cfg.M + cfg.m * cfg.K)[None]).reshape(-1)


def eq_rows(cfg):
    """the initial block, then the defects of stages 0..N-1"""
    k = np.arange(cfg.N)[:, None] * cfg.rows_k + cfg.rows0
    return np.concatenate([np.arange(cfg.nx), (k + np.arange(cfg.nx)[None]).reshape(-1)])


def kkt_system(cfg, p, w, lam_g, lam_x, obs=None):
    """(W [n_var, n_var], A [n_x (N+1), n_var], infeasible): W = exact Lagrangian Hessian + sum over the inequality rows of stages 1..N-1 of
    grad g (z / s) grad g' with z = max(-lam_g, 0), s = g - lbg + the bound terms max(lam_x, 0) / (ub - w) + max(-lam_x, 0) / (w - lb) of
    X_1..X_N and U; the stage-0 pair / obstacle rows, the pad rows and X_0 carry nothing.  A: the initial block and the defects, linearised.
    infeasible: a row or bound with a positive multiplier has s <= 0 (its term is left out of W)."""
    w = np.asarray(w, float).reshape(-1); lam_g = np.asarray(lam_g, float).reshape(-1); lam_x = np.asarray(lam_x, float).reshape(-1)
    assert w.size == cfg.n_var and lam_g.size == cfg.n_g and lam_x.size == cfg.n_var
    lbx, ubx, lbg, _ = R.bounds(cfg)
    if obs is None:
        g, J = R.constraints(cfg, w, p), R.jacobian(cfg, w, p)
    else:
        g, J = MO.constraints(cfg, w, p, obs), MO.jacobian(cfg, w, p, obs)
    rows = ineq_rows(cfg)
    lam = np.zeros(cfg.n_g)
    eq = eq_rows(cfg)
    lam[eq] = lam_g[eq]
    lam[rows] = lam_g[rows]
    # Hessian: nlp_ref's terms; the obstacle blocks from the field when there is one
    field = MO.field(cfg, cfg.obstacles if obs is None else obs) if cfg.K else None
    lam_h = lam.copy()
    X, _ = R.unpack(cfg, w)
    if cfg.K:
        ob_rows = np.array([MO.obstacle_row(cfg, k, i, q) for k in range(cfg.N) for i in range(cfg.m) for q in range(cfg.K)])
        lam_h[ob_rows] = 0.0
        W = R.hess_lagrangian(cfg, w, p, lam_h)
        for k in range(1, cfg.N):
            for i in range(cfg.m):
                for q in range(cfg.K):
                    l = lam[MO.obstacle_row(cfg, k, i, q)]
                    dx = X[k, 3 * i] - field[k, q, 0]; dy = X[k, 3 * i + 1] - field[k, q, 1]
                    rr = np.sqrt(dx * dx + dy * dy)
                    n = np.array([dx, dy]) / rr
                    a = k * cfg.nx + 3 * i
                    W[a: a + 2, a: a + 2] += l * (np.eye(2) - np.outer(n, n)) / rr
    else:
        W = R.hess_lagrangian(cfg, w, p, lam_h)
    bad = False
    z = np.maximum(-lam_g[rows], 0.0)
    s = g[rows] - lbg[rows]
    for r, zi, si in zip(rows, z, s):
        if zi > 0.0:
            if si <= 0.0:
                bad = True
            else:
                W += np.outer(J[r], J[r]) * (zi / si)
    for j in range(cfg.nx, cfg.n_var):
        if np.isfinite(ubx[j]) and lam_x[j] > 0.0:
            if ubx[j] - w[j] <= 0.0:
                bad = True
            else:
                W[j, j] += lam_x[j] / (ubx[j] - w[j])
        if np.isfinite(lbx[j]) and lam_x[j] < 0.0:
            if w[j] - lbx[j] <= 0.0:
                bad = True
            else:
                W[j, j] += -lam_x[j] / (w[j] - lbx[j])
    return W, J[eq], bad


def _cost_rhs(cfg, dxs, k0=0):
    """the linear term of the objective: +2 Q dxs on X_k, k0 <= k < N (the minimiser of 1/2 dw' W dw - c' dw)"""
    c = np.zeros(cfg.n_var)
    qd = np.tile(np.asarray(cfg.q, float), cfg.m)
    for k in range(k0, cfg.N):
        c[k * cfg.nx: (k + 1) * cfg.nx] = 2.0 * qd * dxs
    return c


def dense_sens(cfg, W, A, dP, k0=0):
    """dw [n_var, n] for the columns of dP [n_p, n] = [dx; dxs]: the minimiser of 1/2 dw' W dw - sum_k (2 Q dxs)' dX_k over stages k >= k0 subject to
    dX_k0 = dx and the linearised defects of stages >= k0 (k0 = 0: the definition; entries of stages < k0 are returned as 0)"""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    dP = np.asarray(dP, float).reshape(2 * nx, -1)
    vx = np.arange(k0 * nx, (N + 1) * nx); vu = nx * (N + 1) + np.arange(k0 * nu, N * nu)
    v = np.concatenate([vx, vu])
    rows = np.concatenate([np.arange(nx), nx + np.arange(k0 * nx, N * nx)])      # "X_k0 = dx", then the defects k >= k0
    Ak = A[rows][:, v].copy()
    Ak[:nx] = 0.0
    Ak[:nx, :nx] = np.eye(nx)
    n, me = v.size, rows.size
    K = np.zeros((n + me, n + me))
    K[:n, :n] = W[np.ix_(v, v)]; K[:n, n:] = Ak.T; K[n:, :n] = Ak
    rhs = np.zeros((n + me, dP.shape[1]))
    for c in range(dP.shape[1]):
        rhs[:n, c] = _cost_rhs(cfg, dP[nx:, c], k0)[v]
        rhs[n: n + nx, c] = dP[:nx, c]
    # LU with two steps of iterative refinement, the residual in extended precision: with Sigma up to 1e9 on the diagonal the plain solve
    # carries eps * cond(K) of its own, more than the definition moves under a last-bit change of its inputs (spread below)
    from scipy.linalg import lu_factor, lu_solve
    lu = lu_factor(K)
    sol = lu_solve(lu, rhs)
    Kl, rl = K.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(2):
        sol = sol + lu_solve(lu, (rl - Kl @ sol.astype(np.longdouble)).astype(np.float64))
    out = np.zeros((cfg.n_var, dP.shape[1]))
    out[v] = sol[:n]
    return out


def dense_gains(cfg, W, A):
    """G [N, n_u, n_x]: G_k = dU_k / dX_k of the tail problem that starts at stage k, each from one dense solve"""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    G = np.zeros((N, nu, nx))
    dP = np.concatenate([np.eye(nx), np.zeros((nx, nx))])
    for k in range(N):
        dw = dense_sens(cfg, W, A, dP, k0=k)
        G[k] = dw[nx * (N + 1) + k * nu: nx * (N + 1) + (k + 1) * nu]
    return G


def stage_recursion(cfg, p, w, lam_g, lam_x, obs=None, dp=None):
    """dict(gains [N, n_u, n_x], aff [N, n_u], dw [n_var] (dp given), info, min_eig): P_N = the bound terms of X_N,
    F = W_k + [B A]' P_{k+1} [B A] in the order [U_k; X_k], G_k = -F_uu^-1 F_ux, no inertia shift.  info: 2 when a row or bound with a positive
    multiplier has s <= 0, else 1 when the elimination of some F_uu meets a pivot <= 0, else 0; gains, aff and dw are zeros unless info == 0.
    min_eig: the smallest eigenvalue of any F_uu before the first bad pivot."""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    W, A, bad = kkt_system(cfg, p, w, lam_g, lam_x, obs)
    uo = nx * (N + 1)
    dp = None if dp is None else np.asarray(dp, float).reshape(-1)
    dxs = np.zeros(nx) if dp is None else dp[nx:]
    qd = np.tile(np.asarray(cfg.q, float), cfg.m)
    P = W[N * nx: (N + 1) * nx, N * nx: (N + 1) * nx].copy()
    pv = np.zeros(nx)
    G = np.zeros((N, nu, nx)); ga = np.zeros((N, nu))
    info, min_eig = (INFO_INFEASIBLE if bad else INFO_OK), np.inf
    for k in range(N - 1, -1, -1):
        ix = np.arange(k * nx, (k + 1) * nx); iu = uo + np.arange(k * nu, (k + 1) * nu)
        iz = np.concatenate([iu, ix])
        d = A[nx + k * nx: nx + (k + 1) * nx]                  # defect k: dX_{k+1} - A dX_k - B dU_k
        BA = -d[:, iz]
        F = W[np.ix_(iz, iz)] + BA.T @ P @ BA
        f = BA.T @ pv
        f[nu:] += -2.0 * qd * dxs
        Fuu = F[:nu, :nu]
        min_eig = min(min_eig, float(np.linalg.eigvalsh(0.5 * (Fuu + Fuu.T)).min()))
        M = np.concatenate([F, f[:, None]], axis=1)
        indef = False
        for i in range(nu):                                     # the kernel's elimination: pivots in their natural order
            if not M[i, i] > 0.0:
                indef = True
                break
            M[i + 1:] -= np.outer(M[i + 1:, i] / M[i, i], M[i])
        if indef:
            info = info or INFO_INDEFINITE
            break
        sol = -np.linalg.solve(np.triu(M[:nu, :nu]), M[:nu, nu:])
        G[k], ga[k] = sol[:, :nx], sol[:, nx]
        P = M[nu:, nu: nu + nx]; P = 0.5 * (P + P.T)
        pv = M[nu:, nu + nx]
    out = dict(info=info, min_eig=min_eig)
    if info != INFO_OK:
        G[:] = 0.0; ga[:] = 0.0
    out["gains"], out["aff"] = G, ga
    if dp is not None:
        dw = np.zeros(cfg.n_var)
        if info == INFO_OK:
            x = dp[:nx].copy()
            for k in range(N):
                dw[k * nx: (k + 1) * nx] = x
                u = G[k] @ x + ga[k]
                dw[uo + k * nu: uo + (k + 1) * nu] = u
                d = A[nx + k * nx: nx + (k + 1) * nx]
                x = -d[:, k * nx: (k + 1) * nx] @ x - d[:, uo + k * nu: uo + (k + 1) * nu] @ u
            dw[N * nx: (N + 1) * nx] = x
        out["dw"] = dw
    return out


def _ulp_move(a, rng, ulps=4, sign=None):
    """every entry moved by +-ulps units in its last place: all one way (sign = +-1) or each entry its own way (sign = None)"""
    a = np.asarray(a, float)
    return a + (rng.choice([-1.0, 1.0], a.shape) if sign is None else sign) * ulps * np.spacing(np.abs(a))


def spread(cfg, p, w, lam_g, lam_x, obs=None, dp=None, draws=6, seed=0):
    """(spread of the gains, spread of dw): the largest deviation of the recursion from itself over `draws` copies of (w, lam_g, lam_x) moved by
    +-4 ulp (the first two all up and all down — a slack of 1e-9 under a bound of 6 moves by 4e-6 of itself either way, which random signs over
    few draws can miss — the others entry by entry), relative to max|G| and max|dw| — how far two correct evaluations of the definition at this point may lie apart.  (0, 0) when the
    point's info is not 0."""
    a = stage_recursion(cfg, p, w, lam_g, lam_x, obs, dp)
    if a["info"] != INFO_OK:
        return 0.0, 0.0
    rng = np.random.default_rng(seed)
    sg = sw = 0.0
    ng = max(np.abs(a["gains"]).max(), 1e-300); nw = max(np.abs(a["dw"]).max(), 1e-300) if dp is not None else 1.0
    for n in range(draws):
        sign = (1.0, -1.0)[n] if n < 2 else None
        b = stage_recursion(cfg, p, _ulp_move(w, rng, sign=sign), _ulp_move(lam_g, rng, sign=sign), _ulp_move(lam_x, rng, sign=sign), obs, dp)
        if b["info"] != INFO_OK:
            continue
        sg = max(sg, float(np.abs(a["gains"] - b["gains"]).max() / ng))
        if dp is not None:
            sw = max(sw, float(np.abs(a["dw"] - b["dw"]).max() / nw))
    return sg, sw


def recursion_against_dense(cfg, p, w, lam_g, lam_x, obs=None, dp=None):
    """(error of the gains, their spread, error of dw, its spread): the stage recursion against the dense solve, relative to max|G| and max|dw|,
    next to the spread that bounds them (x 100, + 1e-12) in the tests and in the fixture's screen"""
    r = stage_recursion(cfg, p, w, lam_g, lam_x, obs, dp)
    W, A, _ = kkt_system(cfg, p, w, lam_g, lam_x, obs)
    G = dense_gains(cfg, W, A)
    dwd = dense_sens(cfg, W, A, dp)[:, 0]
    sg, sw = spread(cfg, p, w, lam_g, lam_x, obs, dp)
    return (float(np.abs(r["gains"] - G).max() / np.abs(G).max()), sg, float(np.abs(r["dw"] - dwd).max() / np.abs(dwd).max()), sw)


def prediction_errors(w0, dw, w_h, w_h2, h):
    """(e_h, e_h/2, ratio): |w0 + h dw - w*(p + h d)|_inf, the same at h / 2, and their ratio (4 for a first-order prediction)"""
    e1 = float(np.abs(w0 + h * dw - w_h).max()); e2 = float(np.abs(w0 + 0.5 * h * dw - w_h2).max())
    return e1, e2, e1 / max(e2, 1e-300)


def linearised_defect(cfg, w, dw):
    """largest |dX_{k+1} - A_k dX_k - B_k dU_k| over the horizon"""
    J = R.jacobian(cfg, w, np.zeros(2 * cfg.nx))
    rows = eq_rows(cfg)[cfg.nx:]
    return float(np.abs(J[rows] @ dw).max())


# ---- the fixtures of tests/golden/sens_cases.npz (tests/golden/gen_sens_cases.py) and the two bad points the verdict tests share
def case_configs():
    """name -> (oracle NLPConfig, obstacle field kind: None / "static" [K, 3] / "moving" [N, K, 3]): row-paired and one-row team sizes, pad rows,
    pair rows, obstacle rows, a heading bound, the shortest horizon the config check admits"""
    from tests import helpers as Hh
    three = R.NLPConfig(m=3, N=3, T=0.3, dmin=0.4, v_max=0.15, w_max=1.5)
    eight = R.NLPConfig(m=8, N=4, T=0.1, dmin=0.3, v_max=0.22, w_max=2.84)
    bounded = R.NLPConfig(m=1, N=6, T=0.2, dmin=0.0, v_max=0.2, w_max=1.0, th_max=2 * np.pi, pad_rows=False)      # the obstacle scripts' heading bound
    return {"one2": (R.cfg_one(2), None), "two8": (R.cfg_two(8), None), "three3": (three, None),
            "mix3_static": (Hh.cfg_mix3(10), "static"), "mix3_moving": (Hh.cfg_mix3(10), "moving"),
            "six5": (R.cfg_six(5), None), "six20": (R.cfg_six(20), None), "eight4": (eight, None), "ten6": (R.cfg_ten(6), None),
            "heading1": (bounded, None)}


def load_cases():
    """{name: dict(cfg, kind, h, p, d, w, w_h, w_h2, lam_g, lam_x, obs or None)} with the instance index leading every array"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sens_cases.npz"))
    out = {}
    for name, (cfg, kind) in case_configs().items():
        c = dict(cfg=cfg, kind=kind, h=float(z["h"]), obs=None)
        for k in ("p", "d", "w", "w_h", "w_h2", "lam_g", "lam_x") + (("obs",) if kind else ()):
            c[k] = z[name + "/" + k]
        out[name] = c
    return out


def indefinite_point(cfg, w, lam_g, value=-60.0, robot=0):
    """lam_g with the defect multipliers of robot `robot` at the last stage k >= 1 where it moves set so that the heading curvature
    T v (l_x cos th + l_y sin th) of that stage is `value` (the theta-v cross term T (l_x sin th - l_y cos th) stays 0): P_k gets a negative
    heading entry and F_uu of stage k-1 turns negative through the omega -> theta coupling, T^2 P_k[th, th] (the pivot of that robot's turn
    rate: lane 2 robot + 1).  Returns (lam_g, k)."""
    X, U = R.unpack(cfg, w)
    k = max(k for k in range(1, cfg.N) if abs(U[k, 2 * robot]) > 1e-3)
    th, v = X[k, 3 * robot + 2], U[k, 2 * robot]
    out = np.array(lam_g, float)
    o = cfg.rows0 + k * cfg.rows_k + 3 * robot
    out[o] = value * np.cos(th) / (cfg.T * v); out[o + 1] = value * np.sin(th) / (cfg.T * v)
    return out, k


def infeasible_point(cfg, w, lam_x):
    """(w, lam_x) with the speed of robot 0 at stage 1 beyond its upper bound while its multiplier is positive: z > 0 on s <= 0"""
    w2, l2 = np.array(w, float), np.array(lam_x, float)
    j = cfg.nx * (cfg.N + 1) + cfg.nu
    w2[j] = cfg.v_max + 1e-3; l2[j] = 1.0
    return w2, l2
