"""numpy side of the forward plan-update checks (nmpc_sens_update_batch, include/nmpc.h), on top of tests/sens_ref.kkt_system and
tests/sens_adjoint_ref.obstacle_block / _bordered / _solve: dw minimises 1/2 dw' W dw + c' dw on dX_0 = dx0 and the linearised defects with
c = -2 Q dxs on X_k (k < N) + M_o dobs - rhs, and alpha is the largest step in (0, 1] along (dw, dobs) that keeps every linearised slack >= 0.

  linear_term     c [n_var], its terms added per entry in the kernel's order: goal, rhs, the obstacles in index order
  dense_update    dw by one bordered solve (LU, refined)
  stage_update    the kernel's recursion and forward pass: dict(dw, alpha, info)
  alpha_items     (s, ds) of every item alpha runs over; alpha_of(s, ds) = min(1, min s / -ds over s > 0, ds < 0)
  spread          the recursion against itself with w, lam_g, lam_x moved by +-4 ulp: (spread of dw, spread of alpha)
  row_dobs / row_rhs   the seeded inputs of point n of a row of tests/sens_points.SENS_TABLE, with weight on every entry
  load_cases      the fixtures of tests/golden/sens_update_cases.npz (tests/golden/gen_sens_update_cases.py); screen: what they must pass

`drop` names a term of M_o left out on purpose (the visibility checks), as in tests/sens_adjoint_ref: "sigma_nn", "r_column", "first_entry".

Shared by tests/test_sens_update_host.py, tests/test_gpu_sens_update.py and tests/golden/gen_sens_update_cases.py."""
import os

import numpy as np

from oracle import nlp_ref as R
from tests import moving_obstacles_ref as MO
from tests import sens_adjoint_ref as AR
from tests import sens_ref as S


def _vec(a, n):
    return np.zeros(n) if a is None else np.asarray(a, float).reshape(-1)


def linear_term(cfg, w, lam_g, obs, dp=None, dobs=None, rhs=None, drop=None):
    """c [n_var]: -2 Q dxs on X_k, k < N, then -rhs, then the blocks of M_o against dobs, robot by robot and obstacle by obstacle"""
    nx, N, K = cfg.nx, cfg.N, cfg.K
    w = np.asarray(w, float).reshape(-1); lam_g = np.asarray(lam_g, float).reshape(-1)
    c = -S._cost_rhs(cfg, _vec(dp, 2 * nx)[nx:])
    c = c - _vec(rhs, cfg.n_var)
    if dobs is not None:
        assert obs is not None, "dobs without a per-instance field"
        d = np.asarray(dobs, float).reshape(-1, K, 3)
        assert d.shape[0] == AR.field_stages(cfg, obs)
        X, _ = R.unpack(cfg, w)
        for k in range(1, N):
            ei, e = AR._entry(cfg, obs, k, drop)
            for i in range(cfg.m):
                a = k * nx + 3 * i
                for q in range(K):
                    c[a: a + 2] += AR.obstacle_block(cfg, X[k, 3 * i: 3 * i + 2], lam_g[MO.obstacle_row(cfg, k, i, q)], e[q], drop) @ d[ei, q]
    return c


def dense_update(cfg, p, w, lam_g, lam_x, obs, dp=None, dobs=None, rhs=None):
    """dw [n_var] by one solve of the bordered system with [-c; dx0; 0]"""
    W, A, _ = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    b = np.zeros(cfg.n_var + A.shape[0])
    b[: cfg.n_var] = -linear_term(cfg, w, lam_g, obs, dp, dobs, rhs)
    b[cfg.n_var: cfg.n_var + cfg.nx] = _vec(dp, 2 * cfg.nx)[: cfg.nx]
    return AR._solve(AR._bordered(cfg, W, A), b[:, None])[: cfg.n_var, 0]


def alpha_items(cfg, w, obs, dw, dobs=None):
    """(s, ds): the pair and obstacle rows of stages 1..N-1 and both sides of every finite bound of X_1..X_N and U, in that order; obs None:
    the config's own field (no dobs)"""
    nx, N, K = cfg.nx, cfg.N, cfg.K
    w = np.asarray(w, float).reshape(-1); dw = np.asarray(dw, float).reshape(-1)
    X, _ = R.unpack(cfg, w); dX, _ = R.unpack(cfg, dw)
    s, ds = [], []
    d = None if dobs is None else np.asarray(dobs, float).reshape(-1, K, 3)
    field = MO.field(cfg, cfg.obstacles if obs is None else obs) if K else None
    for k in range(1, N):
        if cfg.M:
            for (i, a) in cfg.pairs():
                e = X[k, 3 * i: 3 * i + 2] - X[k, 3 * a: 3 * a + 2]
                s.append(e @ e - cfg.dmin ** 2)
                ds.append(2.0 * e @ (dX[k, 3 * i: 3 * i + 2] - dX[k, 3 * a: 3 * a + 2]))
        for i in range(cfg.m):
            for q in range(K):
                e = X[k, 3 * i: 3 * i + 2] - field[k, q, :2]
                rr = np.sqrt(e @ e)
                do = np.zeros(3) if d is None else d[k if d.shape[0] == N else 0, q]
                s.append(rr - cfg.rob_dim - field[k, q, 2] - cfg.margin)
                ds.append((e / rr) @ (dX[k, 3 * i: 3 * i + 2] - do[:2]) - do[2])
    lbx, ubx, _, _ = R.bounds(cfg)
    for j in range(nx, cfg.n_var):
        if np.isfinite(ubx[j]):
            s.append(ubx[j] - w[j]); ds.append(-dw[j])
        if np.isfinite(lbx[j]):
            s.append(w[j] - lbx[j]); ds.append(dw[j])
    return np.array(s), np.array(ds)


def alpha_of(s, ds):
    m = (s > 0.0) & (ds < 0.0)
    with np.errstate(over="ignore"):      # a denormal ds: the ratio is +inf, which limits nothing
        return float(min(1.0, (s[m] / -ds[m]).min())) if m.any() else 1.0


def stage_update(cfg, p, w, lam_g, lam_x, obs, dp=None, dobs=None, rhs=None, drop=None):
    """dict(dw [n_var], alpha, info): the kernel's order — P_N = the bound terms of X_N, p_N = c_XN, the affine column of stage k is
    [B A]' p_{k+1} + c on (U_k, X_k), the pivots in their natural order, no inertia shift; the forward pass from dX_0 = dx0; alpha over
    alpha_items.  info as sens_ref.stage_recursion; with info != 0, dw = 0 and alpha = 0."""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    w = np.asarray(w, float).reshape(-1); lam_g = np.asarray(lam_g, float).reshape(-1)
    W, A, bad = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    c = linear_term(cfg, w, lam_g, obs, dp, dobs, rhs, drop)
    uo = nx * (N + 1)
    P = W[N * nx: (N + 1) * nx, N * nx: (N + 1) * nx].copy()
    pv = c[N * nx: (N + 1) * nx].copy()
    G = np.zeros((N, nu, nx)); ga = np.zeros((N, nu))
    info = S.INFO_INFEASIBLE if bad else S.INFO_OK
    for k in range(N - 1, -1, -1):
        ix = np.arange(k * nx, (k + 1) * nx); iu = uo + np.arange(k * nu, (k + 1) * nu)
        iz = np.concatenate([iu, ix])
        BA = -A[nx + k * nx: nx + (k + 1) * nx][:, iz]
        F = W[np.ix_(iz, iz)] + BA.T @ P @ BA
        f = BA.T @ pv + c[iz]
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
    out = dict(info=info, dw=np.zeros(cfg.n_var), alpha=0.0)
    if info != S.INFO_OK:
        return out
    dw = out["dw"]
    x = _vec(dp, 2 * nx)[:nx].copy()
    for k in range(N):
        dw[k * nx: (k + 1) * nx] = x
        u = G[k] @ x + ga[k]
        dw[uo + k * nu: uo + (k + 1) * nu] = u
        d = A[nx + k * nx: nx + (k + 1) * nx]
        x = -d[:, k * nx: (k + 1) * nx] @ x - d[:, uo + k * nu: uo + (k + 1) * nu] @ u
    dw[N * nx: (N + 1) * nx] = x
    out["alpha"] = alpha_of(*alpha_items(cfg, w, obs, dw, dobs))
    return out


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def spread(cfg, p, w, lam_g, lam_x, obs, dp=None, dobs=None, rhs=None, draws=6, seed=0):
    """(spread of dw, spread of alpha): the largest deviation of the recursion from itself over `draws` copies of (w, lam_g, lam_x) moved by
    +-4 ulp (the first two all up and all down, the others entry by entry, as sens_ref.spread), relative to max|dw| and to alpha.  (0, 0) when
    the point's info is not 0."""
    a = stage_update(cfg, p, w, lam_g, lam_x, obs, dp, dobs, rhs)
    if a["info"] != S.INFO_OK:
        return 0.0, 0.0
    rng = np.random.default_rng(seed)
    sw = sa = 0.0
    for n in range(draws):
        sign = (1.0, -1.0)[n] if n < 2 else None
        b = stage_update(cfg, p, S._ulp_move(w, rng, sign=sign), S._ulp_move(lam_g, rng, sign=sign), S._ulp_move(lam_x, rng, sign=sign), obs, dp, dobs, rhs)
        if b["info"] != S.INFO_OK:
            continue
        sw = max(sw, rel(b["dw"], a["dw"]))
        sa = max(sa, abs(b["alpha"] - a["alpha"]) / a["alpha"])
    return sw, sa


def _weights(rng, shape):
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def row_dobs(r, n):
    """the change of the field at point n of the row r of tests/sens_points.SENS_TABLE, in the field's own shape ([K, 3] or [N, K, 3]); None for a
    row without a per-instance field.  Weight on every entry, centimetres: of the size of a change between a solve and its use."""
    if r.kind not in ("static", "moving"):
        return None
    cfg = r.cfg
    shape = (cfg.K, 3) if r.kind == "static" else (cfg.N, cfg.K, 3)
    return 0.02 * _weights(np.random.default_rng(3000 * r.seed + n), shape)


def row_rhs(r, n):
    """the general linear term at point n of the row r: weight on every entry, X_0 and X_N included"""
    return _weights(np.random.default_rng(5000 * r.seed + n), r.cfg.n_var)


# ---- the fixtures of tests/golden/sens_update_cases.npz (tests/golden/gen_sens_update_cases.py)
H_UPD = 2e-3


def load_cases():
    """{name: dict(cfg, kind, h, p, obs, dx, d, w, w_h, w_h2, lam_g, lam_x)} with the instance index leading every array.  The simultaneous move
    is x0 + h dx, obs + h d; w_h and w_h2 are the oracle's re-solves at h and h / 2."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sens_update_cases.npz"))
    out = {}
    for name, (cfg, kind) in AR.obs_case_configs().items():
        c = dict(cfg=cfg, kind=kind, h=float(z["h"]))
        for k in ("p", "obs", "dx", "d", "w", "w_h", "w_h2", "lam_g", "lam_x"):
            c[k] = z[name + "/" + k]
        out[name] = c
    return out


def case_dp(cfg, dx):
    """dp = [dx; 0]: the state moves, the goal stays"""
    return np.concatenate([np.asarray(dx, float), np.zeros(cfg.nx)])


def screen(cfg, p, w, lam_g, lam_x, obs, dx, d, w_h, w_h2, h):
    """dict(ok, info, min_eig, ratio, alpha_h, e_u, e_u0, e1, e2) of one instance, on the reference alone: info 0, every F_uu with its smallest
    eigenvalue >= 1e-6, the prediction-error ratio of w + h dw against the re-solves in [3.8, 4.2], alpha(h) == 1 for the step h (dw, d), and
    |U_0 + h dU_0 - U_0(h)| < |U_0 - U_0(h)|"""
    r = S.stage_recursion(cfg, p, w, lam_g, lam_x, obs)
    out = dict(ok=False, info=r["info"], min_eig=r["min_eig"], ratio=0.0, alpha_h=0.0, e_u=0.0, e_u0=0.0, e1=0.0, e2=0.0)
    if r["info"] != S.INFO_OK or r["min_eig"] < 1e-6:
        return out
    dp = case_dp(cfg, dx)
    u = stage_update(cfg, p, w, lam_g, lam_x, obs, dp=h * dp, dobs=h * np.asarray(d))
    dw = dense_update(cfg, p, w, lam_g, lam_x, obs, dp=dp, dobs=d)
    e1, e2, ratio = S.prediction_errors(w, dw, w_h, w_h2, h)
    uo = cfg.nx * (cfg.N + 1); sl = slice(uo, uo + cfg.nu)
    e_u = float(np.abs(w[sl] + h * dw[sl] - w_h[sl]).max()); e_u0 = float(np.abs(w[sl] - w_h[sl]).max())
    out.update(ratio=ratio, alpha_h=u["alpha"], e_u=e_u, e_u0=e_u0, e1=e1, e2=e2)
    out["ok"] = bool(3.8 <= ratio <= 4.2 and u["alpha"] == 1.0 and e_u < e_u0)
    return out
