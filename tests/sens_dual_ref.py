"""numpy side of the multiplier-update checks (nmpc_sens_update_batch_duals, include/nmpc.h), on top of tests/sens_ref.kkt_system and
tests/sens_update_ref: (dw, dlam_g, dlam_x) solve the linearised barrier KKT system at fixed complementarity products, and alpha_dual is the
largest step in (0, 1] along (dlam_g, dlam_x) that keeps every multiplier's sign.

  dense_duals     (dw, dlam_g, dlam_x) from ONE bordered solve: its lower block is dlam_g on the initial block and the defect rows
  stage_duals     the kernel's order: dw of sens_update_ref.stage_update, then the backward walk r_k = W_k [dU_k; dX_k] + c_k,
                  dnu_{k-1} = A_k' dnu_k - r_Xk; dict(dw, alpha, info, dlam_g, dlam_x, alpha_dual)
  ineq_duals / bound_duals   (c) and (d) of the definition from a given dw — shared by the two above
  dual_items / alpha_dual_of (z, dz) of every item alpha_dual runs over
  spread          stage_duals against itself with w, lam_g, lam_x moved by +-4 ulp: (dlam_g, dlam_x, alpha_dual, identity), whole and per stage
  parity          an output pair against the reference in every measure the bounds hold: whole outputs and stage blocks (stage_blocks)
  identity        the residual of stationarity (a), with oracle.nlp_ref's exact Hessian and Jacobian and central differences of grad_lag
  kkt_growth      max(stat, eq) of tests/duals_ref.residuals along a step h: the certificate's measure
  correct_ref     AdvancedStepController.correct(update_duals=True) in numpy; screen_certificate / screen_chain: what the end-to-end GPU checks
                  keep of tests/golden/sens_update_cases.npz

`drop` as in tests/sens_update_ref.  Shared by tests/test_sens_dual_host.py and tests/test_gpu_sens_dual.py."""
import numpy as np

from oracle import nlp_ref as R
from tests import duals_ref as D
from tests import moving_obstacles_ref as MO
from tests import sens_adjoint_ref as AR
from tests import sens_ref as S
from tests import sens_update_ref as UR


def _flat(a):
    return np.asarray(a, float).reshape(-1)


def _sigma(cfg, w, p, lam_g, obs):
    """(rows, Sigma) over the inequality rows of stages 1..N-1: Sigma_i = max(-lam_g,i, 0) / s_i, 0.0 where lam_g,i >= 0"""
    g = R.constraints(cfg, w, p) if obs is None else MO.constraints(cfg, w, p, obs)
    _, _, lbg, _ = R.bounds(cfg)
    rows = S.ineq_rows(cfg)
    z = np.maximum(-lam_g[rows], 0.0)
    s = g[rows] - lbg[rows]
    return rows, np.where(z > 0.0, z / np.where(z > 0.0, s, 1.0), 0.0)


def _beta(cfg, w, lam_x):
    """the bound term of W's diagonal per variable (0.0 on X_0, on an unbounded heading and where lam_x == 0)"""
    lbx, ubx, _, _ = R.bounds(cfg)
    b = np.zeros(cfg.n_var)
    for j in range(cfg.nx, cfg.n_var):
        if np.isfinite(ubx[j]) and lam_x[j] > 0.0:
            b[j] = lam_x[j] / (ubx[j] - w[j])
        if np.isfinite(lbx[j]) and lam_x[j] < 0.0:
            b[j] = -lam_x[j] / (w[j] - lbx[j])
    return b


def ineq_duals(cfg, p, w, lam_g, obs, dw, dobs=None):
    """(rows, dlam_g on them) = Sigma_i ds_i with the ds of sens_update_ref.alpha_items (its first len(rows) items, in row order); exactly 0.0
    where lam_g,i >= 0"""
    rows, sg = _sigma(cfg, w, p, lam_g, obs)
    _, ds = UR.alpha_items(cfg, w, obs, dw, dobs)
    ds = ds[: rows.size]
    return rows, np.where(sg > 0.0, sg * ds, 0.0)


def bound_duals(cfg, w, lam_x, dw):
    """dlam_x [n_var] = beta_j dw_j; exactly 0.0 where beta_j == 0"""
    b = _beta(cfg, w, lam_x)
    return np.where(b > 0.0, b * dw, 0.0)


def dual_items(cfg, lam_g, lam_x, dlam_g, dlam_x):
    """(z, dz): the inequality rows of stages 1..N-1 (z = -lam_g, dz = -dlam_g), then every variable from X_1 on (z = |lam_x|,
    dz = sign(lam_x) dlam_x)"""
    rows = S.ineq_rows(cfg)
    j = np.arange(cfg.nx, cfg.n_var)
    return (np.concatenate([-lam_g[rows], np.abs(lam_x[j])]), np.concatenate([-dlam_g[rows], np.sign(lam_x[j]) * dlam_x[j]]))


def alpha_dual_of(z, dz):
    m = (z > 0.0) & (dz < 0.0)
    with np.errstate(over="ignore"):
        return float(min(1.0, (z[m] / -dz[m]).min())) if m.any() else 1.0


def _finish(cfg, p, w, lam_g, lam_x, obs, dw, dobs, nu):
    """dlam_g, dlam_x, alpha_dual from dw and the equality-row multipliers nu [n_x (N + 1)] in the order of sens_ref.eq_rows"""
    dlam_g = np.zeros(cfg.n_g)
    dlam_g[S.eq_rows(cfg)] = nu
    rows, v = ineq_duals(cfg, p, w, lam_g, obs, dw, dobs)
    dlam_g[rows] = v
    dlam_x = bound_duals(cfg, w, lam_x, dw)
    return dlam_g, dlam_x, alpha_dual_of(*dual_items(cfg, lam_g, lam_x, dlam_g, dlam_x))


def dense_duals(cfg, p, w, lam_g, lam_x, obs, dp=None, dobs=None, rhs=None):
    """dict(dw, dlam_g, dlam_x, alpha_dual): one solve of the bordered system [W A'; A 0] [dw; nu] = [-c; dx0; 0]"""
    w, lam_g, lam_x = _flat(w), _flat(lam_g), _flat(lam_x)
    W, A, _ = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    b = np.zeros(cfg.n_var + A.shape[0])
    b[: cfg.n_var] = -UR.linear_term(cfg, w, lam_g, obs, dp, dobs, rhs)
    b[cfg.n_var: cfg.n_var + cfg.nx] = UR._vec(dp, 2 * cfg.nx)[: cfg.nx]
    sol = AR._solve(AR._bordered(cfg, W, A), b[:, None])[:, 0]
    dw = sol[: cfg.n_var]
    dlam_g, dlam_x, ad = _finish(cfg, p, w, lam_g, lam_x, obs, dw, dobs, sol[cfg.n_var:])
    return dict(dw=dw, dlam_g=dlam_g, dlam_x=dlam_x, alpha_dual=ad)


def stage_duals(cfg, p, w, lam_g, lam_x, obs, dp=None, dobs=None, rhs=None, drop=None):
    """sens_update_ref.stage_update's dict plus dlam_g, dlam_x, alpha_dual: the backward walk over the stages with r_k = W_k [dU_k; dX_k] + c_k,
    dnu_{N-1} = -r_XN, dnu_{k-1} = A_k' dnu_k - r_Xk, dnu_init = A_0' dnu_0 - r_X0.  With info != 0 everything is zero."""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    w, lam_g, lam_x = _flat(w), _flat(lam_g), _flat(lam_x)
    out = UR.stage_update(cfg, p, w, lam_g, lam_x, obs, dp, dobs, rhs, drop)
    out.update(dlam_g=np.zeros(cfg.n_g), dlam_x=np.zeros(cfg.n_var), alpha_dual=0.0)
    if out["info"] != S.INFO_OK:
        return out
    dw = out["dw"]
    W, A, _ = S.kkt_system(cfg, p, w, lam_g, lam_x, obs)
    c = UR.linear_term(cfg, w, lam_g, obs, dp, dobs, rhs, drop)
    uo = nx * (N + 1)
    eq = np.zeros((N + 1, nx))      # row 0: the initial block; row k + 1: the defects of stage k
    iN = np.arange(N * nx, (N + 1) * nx)
    eq[N] = -(W[np.ix_(iN, iN)] @ dw[iN] + c[iN])
    for k in range(N - 1, -1, -1):
        ix = np.arange(k * nx, (k + 1) * nx); iu = uo + np.arange(k * nu, (k + 1) * nu)
        iz = np.concatenate([iu, ix])
        r = W[np.ix_(iz, iz)] @ dw[iz] + c[iz]
        Ak = -A[nx + k * nx: nx + (k + 1) * nx][:, ix]
        eq[k] = Ak.T @ eq[k + 1] - r[nu:]
    out["dlam_g"], out["dlam_x"], out["alpha_dual"] = _finish(cfg, p, w, lam_g, lam_x, obs, dw, dobs, eq.reshape(-1))
    return out


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


# ---- stationarity (a), with nothing of the W restatement in it
def _masked(cfg, lam_g):
    """lam_g with the entries that carry nothing by definition (pad rows, the pair / obstacle rows of stage 0) at zero"""
    zg, _ = D.structural_zeros(cfg)
    out = lam_g.copy()
    out[zg] = 0.0
    return out


def _grad_lag(cfg, p, w, lam_g, lam_x, obs):
    J = R.jacobian(cfg, w, p) if obs is None else MO.jacobian(cfg, w, p, obs)
    return R.grad_objective(cfg, w, p) + J.T @ lam_g + lam_x


def _hessian(cfg, p, w, lam, obs):
    """the exact Lagrangian Hessian with the obstacle blocks at the field's own entries"""
    if obs is None:
        return R.hess_lagrangian(cfg, w, p, lam)
    f = MO.field(cfg, obs)
    X, _ = R.unpack(cfg, w)
    rows = [(k, i, q, MO.obstacle_row(cfg, k, i, q)) for k in range(cfg.N) for i in range(cfg.m) for q in range(cfg.K)]
    lh = lam.copy()
    lh[[r[3] for r in rows]] = 0.0
    H = R.hess_lagrangian(cfg, w, p, lh)
    for k, i, q, row in rows:
        e = X[k, 3 * i: 3 * i + 2] - f[k, q, :2]
        rr = np.sqrt(e @ e); n = e / rr
        a = k * cfg.nx + 3 * i
        H[a: a + 2, a: a + 2] += lam[row] * (np.eye(2) - np.outer(n, n)) / rr
    return H


FD_STEP = 1e-3      # central differences of grad_lag along (dp, dobs), two steps extrapolated: error O(t^4)
FD_TOL = 1e-10      # their rounding: eps |grad_lag| / t relative to a first-order term of |lam_g| |dobs| / rr, 1e-16 / 1e-3 / 2.5e-3 with margin


def identity(cfg, p, w, lam_g, lam_x, obs, dw, dlam_g, dlam_x, dp=None, dobs=None, rhs=None):
    """(largest entry of H dw + J' dlam_g + dlam_x + (d_p grad_lag) dp + (d_obs grad_lag) dobs - rhs, the largest entry of any of its terms)"""
    p, w, lam_x = _flat(p), _flat(w), _flat(lam_x)
    lam = _masked(cfg, _flat(lam_g))
    J = R.jacobian(cfg, w, p) if obs is None else MO.jacobian(cfg, w, p, obs)
    terms = [_hessian(cfg, p, w, lam, obs) @ dw, J.T @ dlam_g, dlam_x, -UR._vec(rhs, cfg.n_var)]

    def along(t):
        pp = p + t * UR._vec(dp, 2 * cfg.nx)
        oo = obs if dobs is None else np.asarray(obs, float) + t * np.asarray(dobs, float)
        return _grad_lag(cfg, pp, w, lam, lam_x, oo)
    t = FD_STEP
    d1 = (along(t) - along(-t)) / (2 * t); d2 = (along(0.5 * t) - along(-0.5 * t)) / t
    terms.append((4.0 * d2 - d1) / 3.0)
    return float(np.abs(np.sum(terms, axis=0)).max()), float(max(np.abs(x).max() for x in terms))


def stage_blocks(cfg):
    """(blocks of dlam_g, blocks of dlam_x): the index sets of one stage each — for dlam_g the initial block with its pad rows, then the rows of
    stage k = 0..N-1; for dlam_x [X_k; U_k] of k = 0..N-1, then X_N.  The walk runs backward and everything it meets adds up on the way, so the
    entries of the last stages are small beside max|dlam|: an error there shows only against its own stage."""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    uo = nx * (N + 1)
    g = [np.arange(cfg.rows0)] + [cfg.rows0 + k * cfg.rows_k + np.arange(cfg.rows_k) for k in range(N)]
    x = [np.concatenate([np.arange(k * nx, (k + 1) * nx), uo + np.arange(k * nu, (k + 1) * nu)]) for k in range(N)] + [np.arange(N * nx, uo)]
    return g, x


def block_rel(a, b, blocks):
    """rel(a, b) of every block, each relative to the block's own max|b|"""
    return np.array([rel(a[i], b[i]) for i in blocks])


def spread(cfg, p, w, lam_g, lam_x, obs, dp=None, dobs=None, rhs=None, draws=6, seed=0):
    """dict(g, x, a, ident, gk, xk): the largest deviation of stage_duals from itself over `draws` copies of (w, lam_g, lam_x) moved by +-4 ulp (as
    sens_update_ref.spread), relative to max|dlam_g|, max|dlam_x| and alpha_dual; ident: the residual of (a) at the unmoved point with the moved
    point's (dw, dlam_g, dlam_x), relative to its largest term; gk, xk: the same as g, x per block of stage_blocks, each relative to the block's own
    maximum.  Zeros when the point's info is not 0."""
    a = stage_duals(cfg, p, w, lam_g, lam_x, obs, dp, dobs, rhs)
    bg, bx = stage_blocks(cfg)
    out = dict(g=0.0, x=0.0, a=0.0, ident=0.0, gk=np.zeros(len(bg)), xk=np.zeros(len(bx)))
    if a["info"] != S.INFO_OK:
        return out
    rng = np.random.default_rng(seed)
    for n in range(draws):
        sign = (1.0, -1.0)[n] if n < 2 else None
        b = stage_duals(cfg, p, S._ulp_move(w, rng, sign=sign), S._ulp_move(lam_g, rng, sign=sign), S._ulp_move(lam_x, rng, sign=sign), obs, dp, dobs, rhs)
        if b["info"] != S.INFO_OK:
            continue
        out["g"] = max(out["g"], rel(b["dlam_g"], a["dlam_g"]))
        out["x"] = max(out["x"], rel(b["dlam_x"], a["dlam_x"]))
        out["a"] = max(out["a"], abs(b["alpha_dual"] - a["alpha_dual"]) / a["alpha_dual"])
        out["gk"] = np.maximum(out["gk"], block_rel(b["dlam_g"], a["dlam_g"], bg))
        out["xk"] = np.maximum(out["xk"], block_rel(b["dlam_x"], a["dlam_x"], bx))
        r, sc = identity(cfg, p, w, lam_g, lam_x, obs, b["dw"], b["dlam_g"], b["dlam_x"], dp, dobs, rhs)
        out["ident"] = max(out["ident"], r / sc)
    return out


def bounds(sp):
    """the project's parity bound per output, 100 x spread + 1e-12, and the same per stage block (gk, xk: arrays); the identity's carries the
    rounding of its central differences as well"""
    out = {k: 100.0 * sp[k] + 1e-12 for k in ("g", "x", "a", "gk", "xk")}
    out["ident"] = 100.0 * sp["ident"] + 1e-12 + FD_TOL
    return out


def parity(cfg, got_g, got_x, ref, bd):
    """dict(g, x, gk, xk, worst): dlam_g and dlam_x against the reference's, relative to max|dlam| of the output and per stage block relative to
    the block's own; worst: the largest of them in units of its bound.  A pair of outputs is within parity when worst <= 1."""
    bg, bx = stage_blocks(cfg)
    e = dict(g=rel(got_g, ref["dlam_g"]), x=rel(got_x, ref["dlam_x"]), gk=block_rel(got_g, ref["dlam_g"], bg), xk=block_rel(got_x, ref["dlam_x"], bx))
    e["worst"] = float(max(e["g"] / bd["g"], e["x"] / bd["x"], (e["gk"] / bd["gk"]).max(), (e["xk"] / bd["xk"]).max()))
    return e


# ---- the certificate: how max(stat, eq) of the KKT residuals grows along the step
def kkt_growth(cfg, p, obs, w, lam_g, lam_x, dp, d, dw, dlam_g, dlam_x, h):
    """max(stat, eq) of tests/duals_ref.residuals at (p + h dp, obs + h d) with (w + h dw, lam + h dlam), minus its value at h = 0"""
    r0, _ = D.residuals(cfg, w, p, lam_g, lam_x, obs)
    r1, _ = D.residuals(cfg, w + h * dw, p + h * dp, lam_g + h * dlam_g, lam_x + h * dlam_x, np.asarray(obs) + h * np.asarray(d))
    return float(max(r1[0], r1[1]) - max(r0[0], r0[1]))


# ---- the controller's correction on the reference, and the screens of the end-to-end checks on tests/golden/sens_update_cases.npz
def correct_ref(cfg, p, obs, w, lam_g, lam_x, dp, d, tau=0.99):
    """nmpc_amd.AdvancedStepController.correct(update_duals=True) in numpy: (p, obs, w, lam_g, lam_x) moved by
    step = min(1 if alpha == 1 else tau alpha, 1 if alpha_dual == 1 else tau alpha_dual) along (dp, d, dw, dlam_g, dlam_x), and the step; None
    where the verdict is not 0"""
    st = stage_duals(cfg, p, w, lam_g, lam_x, obs, dp=dp, dobs=d)
    if st["info"] != S.INFO_OK:
        return None
    lim = lambda a: 1.0 if a == 1.0 else tau * a
    s = min(lim(st["alpha"]), lim(st["alpha_dual"]))
    return p + s * dp, obs + s * d, w + s * st["dw"], lam_g + s * st["dlam_g"], lam_x + s * st["dlam_x"], s


RATIO_WINDOW = (3.5, 4.5)      # the certificate's screen: instances whose reference ratio r(h) / r(h/2) lies in it are kept


def screen_certificate(c, b):
    """dict(ratio, r_h, r_h2, r_old, keep) of instance b of a fixture case on the reference, at the oracle's point and its least-squares
    multipliers: r(h) with the updated multipliers, at h and h / 2, and with the old ones"""
    cfg, h = c["cfg"], c["h"]
    a = (cfg, c["p"][b], c["obs"][b], c["w"][b], c["lam_g"][b], c["lam_x"][b])
    dp, d = UR.case_dp(cfg, c["dx"][b]), c["d"][b]
    st = stage_duals(cfg, a[1], a[3], a[4], a[5], a[2], dp=dp, dobs=d)
    r1 = kkt_growth(*a, dp, d, st["dw"], st["dlam_g"], st["dlam_x"], h)
    r2 = kkt_growth(*a, dp, d, st["dw"], st["dlam_g"], st["dlam_x"], 0.5 * h)
    ro = kkt_growth(*a, dp, d, st["dw"], np.zeros(cfg.n_g), np.zeros(cfg.n_var), h)
    ratio = r1 / r2
    return dict(ratio=ratio, r_h=r1, r_h2=r2, r_old=ro, keep=bool(st["info"] == 0 and RATIO_WINDOW[0] <= ratio <= RATIO_WINDOW[1]))


def screen_chain(c, b, tau=0.99):
    """dict(single, chained, keep): |w - w(h)| of one correction to h and of a correction to h / 2 followed by one from there to h, on the
    reference; keep: both went through and the chained plan is closer"""
    cfg, h = c["cfg"], c["h"]
    p, obs = c["p"][b], c["obs"][b]
    dp, d = UR.case_dp(cfg, c["dx"][b]), c["d"][b]
    one = correct_ref(cfg, p, obs, c["w"][b], c["lam_g"][b], c["lam_x"][b], h * dp, h * d, tau)
    half = correct_ref(cfg, p, obs, c["w"][b], c["lam_g"][b], c["lam_x"][b], 0.5 * h * dp, 0.5 * h * d, tau)
    two = None if half is None else correct_ref(cfg, *half[:5], (p + h * dp) - half[0], (obs + h * d) - half[1], tau)
    if one is None or two is None:
        return dict(single=np.inf, chained=np.inf, keep=False)
    e1, e2 = float(np.abs(one[2] - c["w_h"][b]).max()), float(np.abs(two[2] - c["w_h"][b]).max())
    return dict(single=e1, chained=e2, keep=bool(e2 < e1))
