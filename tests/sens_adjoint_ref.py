"""numpy side of the adjoint plan-sensitivity checks (nmpc_sens_adjoint_batch, include/nmpc.h), on top of tests/sens_ref.kkt_system: the
transposes of S_p : dp -> dw (nmpc_sens_batch) and of the obstacle map S_o : dobs -> dw applied to a cotangent wbar of the plan.

  obstacle_block   the 2 x 3 block of M_o of one obstacle row, by the formulas of include/nmpc.h
  obstacle_matrix  M_o [n_var, S K 3] for a field given as [K, 3] (S = 1) or [N, K, 3] (S = N)
  dense_s_p / dense_s_o   the forward maps by one dense solve each (LU, refined as sens_ref.dense_sens)
  dense_adjoint    pbar, obsbar from one dense solve with right-hand side [wbar; 0]
  stage_adjoint    the same by the stage recursion the kernel runs: -wbar as the affine column, the forward pass from v_X0 = 0
  spread           the recursion against itself with w, lam_g, lam_x moved by +-4 ulp
  load_obs_cases   the fixtures of tests/golden/sens_obs_cases.npz (tests/golden/gen_sens_obs_cases.py); obs_mismatch: the end-to-end measure on them

`drop` names a term left out on purpose (the visibility checks): "sigma_nn" the Sigma n n' part of the (ox, oy) columns, "r_column" the radius
column, "first_entry" entry 0 of a per-stage field read at every stage.

Shared by tests/test_sens_adjoint_host.py, tests/test_gpu_sens_adjoint.py and tests/golden/gen_sens_obs_cases.py."""
import os

import numpy as np

from oracle import nlp_ref as R
from tests import moving_obstacles_ref as MO
from tests import sens_ref as S


def field_stages(cfg, obs):
    """S of a field: 1 for [K, 3], N for [N, K, 3]"""
    return 1 if np.ndim(obs) == 2 else cfg.N


def obstacle_block(cfg, xy, l, e, drop=None):
    """the block of M_o in rows (x, y) of a robot at xy, columns (ox, oy, r) of the obstacle entry e, with the row's multiplier l"""
    ex, ey = xy[0] - e[0], xy[1] - e[1]
    rr = np.sqrt(ex * ex + ey * ey)
    n = np.array([ex, ey]) / rr
    s = rr - cfg.rob_dim - e[2] - cfg.margin
    sg = max(-l, 0.0) / s if -l > 0.0 else 0.0
    nn = np.outer(n, n)
    blk = np.zeros((2, 3))
    blk[:, :2] = -l * (np.eye(2) - nn) / rr - (0.0 if drop == "sigma_nn" else sg) * nn
    blk[:, 2] = 0.0 if drop == "r_column" else -sg * n
    return blk


def _entry(cfg, obs, k, drop=None):
    """(index of the entry stage k reads, the entry [K, 3])"""
    if np.ndim(obs) == 2:
        return 0, np.asarray(obs, float)
    return (k, np.asarray(obs, float)[0 if drop == "first_entry" else k])


def obstacle_matrix(cfg, w, lam_g, obs, drop=None):
    """M_o [n_var, S K 3]: one block per obstacle row (k, robot, o) of stages 1..N-1; the rows of stage 0 carry nothing"""
    K, Sn = cfg.K, field_stages(cfg, obs)
    X, _ = R.unpack(cfg, np.asarray(w, float).reshape(-1))
    M = np.zeros((cfg.n_var, Sn * K * 3))
    for k in range(1, cfg.N):
        ei, e = _entry(cfg, obs, k, drop)
        for i in range(cfg.m):
            for q in range(K):
                a = k * cfg.nx + 3 * i
                c = (ei * K + q) * 3
                M[a: a + 2, c: c + 3] += obstacle_block(cfg, X[k, 3 * i: 3 * i + 2], lam_g[MO.obstacle_row(cfg, k, i, q)], e[q], drop)
    return M


def _bordered(cfg, W, A):
    nx, n, me = cfg.nx, cfg.n_var, A.shape[0]
    Ak = A.copy()
    Ak[:nx] = 0.0
    Ak[:nx, :nx] = np.eye(nx)
    K = np.zeros((n + me, n + me))
    K[:n, :n] = W; K[:n, n:] = Ak.T; K[n:, :n] = Ak
    return K


def _solve(K, rhs):
    """LU with two steps of iterative refinement, the residual in extended precision (as sens_ref.dense_sens)"""
    from scipy.linalg import lu_factor, lu_solve
    lu = lu_factor(K)
    sol = lu_solve(lu, rhs)
    Kl, rl = K.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(2):
        sol = sol + lu_solve(lu, (rl - Kl @ sol.astype(np.longdouble)).astype(np.float64))
    return sol


def dense_s_p(cfg, W, A, dP):
    """dw [n_var, n] = S_p dP for the columns of dP [n_p, n]"""
    return S.dense_sens(cfg, W, A, dP)


def dense_s_o(cfg, W, A, Mo, dobs):
    """dw [n_var, n] = S_o dobs for the columns of dobs [S K 3, n]: the minimiser of 1/2 dw' W dw + (M_o dobs)' dw on the homogeneous equalities"""
    dobs = np.asarray(dobs, float).reshape(Mo.shape[1], -1)
    rhs = np.zeros((cfg.n_var + A.shape[0], dobs.shape[1]))
    rhs[: cfg.n_var] = -Mo @ dobs
    return _solve(_bordered(cfg, W, A), rhs)[: cfg.n_var]


def _pbar_xs(cfg, v):
    qd = np.tile(np.asarray(cfg.q, float), cfg.m)
    return 2.0 * qd * v[: cfg.N * cfg.nx].reshape(cfg.N, cfg.nx).sum(axis=0)


def dense_adjoint(cfg, W, A, Mo, wbar):
    """(pbar [n_p], obsbar [S K 3] or None): [v; nu] solves the bordered system with [wbar; 0]; pbar_x0 = nu of the initial block,
    pbar_xs = sum_k 2 Q v_Xk, obsbar = -M_o' v"""
    rhs = np.zeros(cfg.n_var + A.shape[0])
    rhs[: cfg.n_var] = wbar
    sol = _solve(_bordered(cfg, W, A), rhs[:, None])[:, 0]
    v = sol[: cfg.n_var]
    pbar = np.concatenate([sol[cfg.n_var: cfg.n_var + cfg.nx], _pbar_xs(cfg, v)])
    return pbar, (None if Mo is None else -(Mo.T @ v))


def stage_adjoint(cfg, p, w, lam_g, lam_x, obs, wbar, want_obsbar=None, drop=None):
    """dict(pbar [n_p], obsbar [S, K, 3] or None, info, v): the kernel's order — P_N = the bound terms of X_N, p_N = -wbar_XN, the affine column of
    stage k is [B A]' p_{k+1} - wbar on (U_k, X_k), the pivots in their natural order, no inertia shift; pbar_x0 = -p_0; the forward pass from
    v_X0 = 0 sums 2 Q v_Xk and, at stages 1..N-1, contracts v_Xk with the obstacle blocks, robots in index order, stages in stage order.
    info as sens_ref.stage_recursion; the outputs are zeros unless info == 0."""
    nx, nu, N, K = cfg.nx, cfg.nu, cfg.N, cfg.K
    w = np.asarray(w, float).reshape(-1); lam_g = np.asarray(lam_g, float).reshape(-1); wbar = np.asarray(wbar, float).reshape(-1)
    want_obsbar = (obs is not None) if want_obsbar is None else want_obsbar
    assert not (want_obsbar and obs is None)
    Sn = field_stages(cfg, obs) if obs is not None else 0
    W, A, bad = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    uo = nx * (N + 1)
    P = W[N * nx: (N + 1) * nx, N * nx: (N + 1) * nx].copy()
    pv = -wbar[N * nx: (N + 1) * nx]
    G = np.zeros((N, nu, nx)); ga = np.zeros((N, nu))
    info = S.INFO_INFEASIBLE if bad else S.INFO_OK
    for k in range(N - 1, -1, -1):
        ix = np.arange(k * nx, (k + 1) * nx); iu = uo + np.arange(k * nu, (k + 1) * nu)
        iz = np.concatenate([iu, ix])
        BA = -A[nx + k * nx: nx + (k + 1) * nx][:, iz]
        F = W[np.ix_(iz, iz)] + BA.T @ P @ BA
        f = BA.T @ pv - wbar[iz]
        M = np.concatenate([F, f[:, None]], axis=1)
        indef = False
        for i in range(nu):
            if not M[i, i] > 0.0:
                indef = True
                break
            M[i + 1:] -= np.outer(M[i + 1:, i] / M[i, i], M[i])
        if indef:
            info = info or S.INFO_INDEFINITE
            break
        sol = -np.linalg.solve(np.triu(M[:nu, :nu]), M[:nu, nu:])
        G[k], ga[k] = sol[:, :nx], sol[:, nx]
        P = M[nu:, nu: nu + nx]; P = 0.5 * (P + P.T)
        pv = M[nu:, nu + nx]
    out = dict(info=info, pbar=np.zeros(2 * nx), obsbar=np.zeros((Sn, K, 3)) if want_obsbar else None, v=np.zeros(cfg.n_var))
    if info != S.INFO_OK:
        return out
    v = out["v"]
    x = np.zeros(nx)
    X, _ = R.unpack(cfg, w)
    for k in range(N):
        v[k * nx: (k + 1) * nx] = x
        if want_obsbar and k > 0:
            ei, e = _entry(cfg, obs, k, drop)
            for q in range(K):
                t = np.zeros(3)
                for i in range(cfg.m):
                    t -= obstacle_block(cfg, X[k, 3 * i: 3 * i + 2], lam_g[MO.obstacle_row(cfg, k, i, q)], e[q], drop).T @ x[3 * i: 3 * i + 2]
                out["obsbar"][ei, q] += t
        u = G[k] @ x + ga[k]
        v[uo + k * nu: uo + (k + 1) * nu] = u
        d = A[nx + k * nx: nx + (k + 1) * nx]
        x = -d[:, k * nx: (k + 1) * nx] @ x - d[:, uo + k * nu: uo + (k + 1) * nu] @ u
    v[N * nx: (N + 1) * nx] = x
    out["pbar"] = np.concatenate([-pv, _pbar_xs(cfg, v)])
    return out


def dense_reference(cfg, p, w, lam_g, lam_x, obs, wbar):
    """(pbar, obsbar [S, K, 3] or None) by the dense solve"""
    W, A, _ = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    Mo = obstacle_matrix(cfg, w, np.asarray(lam_g, float).reshape(-1), obs) if obs is not None else None
    pbar, ob = dense_adjoint(cfg, W, A, Mo, np.asarray(wbar, float).reshape(-1))
    return pbar, (None if ob is None else ob.reshape(-1, cfg.K, 3))


def rel(a, b):
    """largest |a - b| relative to max|b| (0 when b is None or empty)"""
    if b is None or np.size(b) == 0:
        return 0.0
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def spread(cfg, p, w, lam_g, lam_x, obs, wbar, draws=6, seed=0):
    """(spread of pbar, spread of obsbar): the largest deviation of the recursion from itself over `draws` copies of (w, lam_g, lam_x) moved by
    +-4 ulp (the first two all up and all down, the others entry by entry, as sens_ref.spread), relative to max|pbar| and max|obsbar|.
    (0, 0) when the point's info is not 0."""
    a = stage_adjoint(cfg, p, w, lam_g, lam_x, obs, wbar)
    if a["info"] != S.INFO_OK:
        return 0.0, 0.0
    rng = np.random.default_rng(seed)
    sp = so = 0.0
    for n in range(draws):
        sign = (1.0, -1.0)[n] if n < 2 else None
        b = stage_adjoint(cfg, p, S._ulp_move(w, rng, sign=sign), S._ulp_move(lam_g, rng, sign=sign), S._ulp_move(lam_x, rng, sign=sign), obs, wbar)
        if b["info"] != S.INFO_OK:
            continue
        sp = max(sp, rel(b["pbar"], a["pbar"]))
        so = max(so, rel(b["obsbar"], a["obsbar"]))
    return sp, so


def cotangent(cfg, seed):
    """a seeded wbar [n_var] with weight on every entry, X_0 and X_N included"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, cfg.n_var) * rng.choice([-1.0, 1.0], cfg.n_var)


def row_cotangent(r, n):
    """the cotangent of point n of the row r of tests/sens_points.SENS_TABLE (host and GPU tests use the same)"""
    return cotangent(r.cfg, 1000 * r.seed + n)


# ---- the fixtures of tests/golden/sens_obs_cases.npz (tests/golden/gen_sens_obs_cases.py)
H_OBS = 2e-3


def obs_case_configs():
    """name -> (oracle NLPConfig, field kind): one robot between two moving obstacles, two robots beside a static one, three robots and a
    moving field; N <= 8"""
    return {"one_moving": (MO.team_cfg(1, 6, 2), "moving"), "two_static": (MO.team_cfg(2, 8, 1), "static"),
            "three_moving": (MO.team_cfg(3, 5, 2), "moving")}


def load_obs_cases():
    """{name: dict(cfg, kind, h, p, obs, d, w, w_h, w_h2, lam_g, lam_x)} with the instance index leading every array; d: the unit direction of
    the field's change, in the shape of obs"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sens_obs_cases.npz"))
    out = {}
    for name, (cfg, kind) in obs_case_configs().items():
        c = dict(cfg=cfg, kind=kind, h=float(z["h"]))
        for k in ("p", "obs", "d", "w", "w_h", "w_h2", "lam_g", "lam_x"):
            c[k] = z[name + "/" + k]
        out[name] = c
    return out


def obs_prediction(cfg, p, w, lam_g, lam_x, obs, d):
    """dw = S_o d by the dense solve"""
    W, A, _ = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    return dense_s_o(cfg, W, A, obstacle_matrix(cfg, w, lam_g, obs), np.asarray(d, float).reshape(-1))[:, 0]


def extrapolated_quotient(w, w_h, w_h2, h):
    """the difference quotient of the re-solves, extrapolated to second order: (4 (w_h/2 - w) - (w_h - w)) / h"""
    return (4.0 * (w_h2 - w) - (w_h - w)) / h


def obs_mismatch(c, b, obsbar, wbar):
    """|<obsbar, d> - <wbar, dq>| / (|wbar| |dq|) for instance b of a fixture case c, dq the extrapolated difference quotient of its re-solves"""
    dq = extrapolated_quotient(c["w"][b], c["w_h"][b], c["w_h2"][b], c["h"])
    return float(abs(np.sum(np.asarray(obsbar).reshape(c["d"][b].shape) * c["d"][b]) - wbar @ dq) / (np.linalg.norm(wbar) * np.linalg.norm(dq)))
