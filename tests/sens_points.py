"""Constructed primal-dual points for nmpc_sens_batch, and one table row per instantiation of sens_kernel<MS> (csrc/nmpc_sens.hip).

include/nmpc.h defines the call for any (w, lam_g, lam_x), so the kernel can be held against tests/sens_ref.py at points built so that every
term of the barrier KKT system has a weight of order one: binding pair and obstacle rows at every stage, controls at both bounds, an x or y
bound, heading bounds, the bounds of X_N, defect multipliers that make the curvature terms show.  Nothing is solved and nothing is stored:
points(row) computes the row's points from its seed.

  SENS_TABLE       20 rows (m, field), MS = m + 16 field: the row's oracle NLPConfig, its field kind and its points
  points(row)      [Point]: p, w, lam_g, lam_x, obs (None: the config's own field), dp
  zero_class       a term class's multipliers zeroed (the visibility condition of the host test)
  reverse_pairs    the pair multipliers of every stage read in reverse order (an emulated wrong pair index)
  null_masks       the entries that carry nothing by definition: stage-0 pair / obstacle rows, the initial block and its pad rows, lam_x of X_0,
                   lam_x of an unbounded heading
  verdict_cases    one point turned into the instances of the verdict batch

The geometry of one stage: the team is a chain, robot i+1 at gap_i from robot i along a direction within 0.12 rad of the stage's own, so that
neighbours are exactly gap_i apart (binding links: sqrt(dmin^2 + s)) and every other pair is further than 1.9 gaps.  A free obstacle (moving
field, one entry per stage) is put beside the chain at its contact distance from the robot it presses on.  Fixed obstacles (a static field or
the config's own) stay where they are and the chain is placed on them: its origin, direction and link angles solve the contact equations
(two fixed discs overlap and press on the same robot, which stands where their contact circles cross).
Under an x or y bound the extreme robot of that coordinate is shifted to the bound's slack (free), or that equation joins the others (one
fixed disc: it takes one end of the chain, the other end reaches the wall; with two the bound is at X_N, which has no obstacle rows).
Every stage has its own layout: w need not satisfy the dynamics, the definition linearises where it is told to."""
import functools
from collections import namedtuple

import numpy as np

from oracle import nlp_ref as R
from tests import moving_obstacles_ref as MO
from tests import sens_ref as S

Point = namedtuple("Point", "p w lam_g lam_x obs dp")
Row = namedtuple("Row", "m field cfg kind seed")      # kind: None (no obstacle rows), "own" (the config's field, (NULL, 0)), "static", "moving"
NPOINTS = 5


def _team(m, N, K=0, **kw):
    base = dict(T=0.3, dmin=0.4, v_max=0.15, w_max=1.5) if m <= 6 else dict(T=0.1, dmin=0.3, v_max=0.22, w_max=2.84)
    if m == 1:
        base = dict(T=0.2, dmin=0.0, v_max=0.2, w_max=1.0, pad_rows=False)
    base.update(kw)
    return R.NLPConfig(m=m, N=N, obstacles=[(0.0, 0.0, 0.1)] * K, **base)


def _own(cfg, obstacles, xy_max):
    cfg.obstacles = list(obstacles); cfg.xy_max = xy_max
    return cfg


HB = 2 * np.pi      # the obstacle scripts' heading bound
NOPAIR = dict(pad_rows=False, pair_rows=False)

# One row per instantiation.  Horizons 2..4 (an interior stage, a first and a last one), N = 12 once: the workspace's [N][KTS] region moves with
# k.  Fixed obstacles need the walls within reach of the chain that leans on them: those rows have a small xy_max.
SENS_TABLE = [
    Row(1, 0, _own(_team(1, 4, th_max=HB), [(0.03, -0.02, 0.15)], 0.40), "own", 101),
    Row(2, 0, _team(2, 2, T=0.05, dmin=0.15, v_max=0.22, w_max=2.84), None, 102),
    Row(3, 0, _team(3, 12, pad_rows=False), None, 103),
    Row(4, 0, _own(_team(4, 3), [(0.04, 0.02, 0.12), (-0.10, -0.05, 0.118)], 2.0), "own", 104),
    Row(5, 0, _team(5, 3, th_max=HB, **NOPAIR), None, 105),
    Row(6, 0, _own(_team(6, 4, pad_rows=False), [(-0.05, 0.08, 0.14)], 1.9), "own", 106),
    Row(7, 0, _team(7, 2, th_max=3.0), None, 107),
    Row(8, 0, _team(8, 3, **NOPAIR), None, 108),
    Row(9, 0, _team(9, 3), None, 109),
    Row(10, 0, _team(10, 4, xy_max=4.0), None, 110),
    Row(1, 1, _team(1, 3, 2, th_max=HB), "moving", 201),
    Row(2, 1, _team(2, 4, 2, xy_max=1.2), "static", 202),
    Row(3, 1, _team(3, 4, 2, th_max=HB), "moving", 203),
    Row(4, 1, _team(4, 3, 8, **NOPAIR), "moving", 204),
    Row(5, 1, _team(5, 2, 1, pad_rows=False, xy_max=1.5), "static", 205),
    Row(6, 1, _team(6, 3, 1), "moving", 206),
    Row(7, 1, _team(7, 3, 2, pad_rows=False, th_max=HB, xy_max=3.0), "static", 207),
    Row(8, 1, _team(8, 2, 2), "moving", 208),
    Row(9, 1, _team(9, 4, 1, xy_max=1.6, **NOPAIR), "static", 209),
    Row(10, 1, _team(10, 3, 8, th_max=HB), "moving", 210),
]


def row_id(r):
    return "m%d_%s" % (r.m, r.kind or "none") + ("_field" if r.field else "")


def _logu(rng, lo, hi, size=None):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


def _tiny(rng, size, negative_only=False):
    """multipliers of rows and bounds that do not bind: exact zeros on some, 1e-10 .. 1e-4 on the rest (of either sign for a bound)"""
    v = _logu(rng, 1e-10, 1e-4, size) * (-1.0 if negative_only else rng.choice([-1.0, 1.0], size))
    return np.where(rng.random(size) < 0.35, 0.0, v)


def _chain(p0, theta, dev, gaps):
    pts = [np.asarray(p0, float)]
    for g, d in zip(gaps, dev):
        pts.append(pts[-1] + g * np.array([np.cos(theta + d), np.sin(theta + d)]))
    return np.array(pts)


def _place_on_fixed(rng, m, gaps, contacts, wall, A, clear):
    """the chain's positions [m, 2] with |pos[i] - c| = D for every contact (i, c, D) and pos[j][coord] = value for wall = (j, coord, value),
    every other coordinate strictly inside +-A and clear(pos) true.  The unknowns are the origin, the direction and the link angles, started
    from a chain that is tangent to the first contact's circle and, with a wall, leans towards it."""
    from scipy.optimize import least_squares
    lo = np.concatenate([[-2 * A, -2 * A, -np.inf], np.full(m - 1, -0.12)]); hi = np.concatenate([[2 * A, 2 * A, np.inf], np.full(m - 1, 0.12)])

    def res(x):
        pos = _chain(x[:2], x[2], x[3:], gaps)
        r = [np.hypot(*(pos[i] - c)) - D for (i, c, D) in contacts]
        if wall is not None:
            r.append(pos[wall[0], wall[1]] - wall[2])
        return np.array(r)
    i0, c0, D0 = contacts[0]
    for _ in range(100):
        th = rng.uniform(-np.pi, np.pi)
        if wall is not None and wall[0] != i0:      # the direction from robot i0 to the wall's robot: towards the wall, as steep as the reach asks
            reach = gaps[min(i0, wall[0]): max(i0, wall[0])].sum()
            phi = np.arccos(min(1.0, abs(wall[2]) / reach)) * rng.choice([-1.0, 1.0]) * rng.uniform(0.7, 1.0)
            th = (0.0 if wall[1] == 0 else 0.5 * np.pi) + (0.0 if wall[2] > 0 else np.pi) + phi + (np.pi if wall[0] < i0 else 0.0)
        a = th + rng.choice([-0.5, 0.5]) * np.pi
        p0 = c0 + D0 * np.array([np.cos(a), np.sin(a)]) - gaps[:i0].sum() * np.array([np.cos(th), np.sin(th)])
        if len(contacts) > 1:      # two discs on one robot: it stands where their contact circles cross, the chain parallel to the line of centres
            c1, D1 = contacts[1][1], contacts[1][2]
            d = np.linalg.norm(c1 - c0); e = (c1 - c0) / d
            x = (d * d + D0 * D0 - D1 * D1) / (2 * d)
            th = np.arctan2(e[1], e[0]) + rng.choice([0.0, np.pi])
            p0 = c0 + x * e + rng.choice([-1.0, 1.0]) * np.sqrt(D0 * D0 - x * x) * np.array([-e[1], e[0]]) - gaps[:i0].sum() * np.array([np.cos(th), np.sin(th)])
        x0 = np.concatenate([p0, [th], rng.uniform(-0.05, 0.05, m - 1)])
        sol = least_squares(res, x0, bounds=(lo, hi), xtol=1e-15, ftol=1e-15, gtol=1e-15)
        pos = _chain(sol.x[:2], sol.x[2], sol.x[3:], gaps)
        if np.abs(res(sol.x)).max() > 1e-12:
            continue
        inside = np.abs(pos) < A - 1e-3
        if wall is not None:
            inside[wall[0], wall[1]] = True
        if inside.all() and clear(pos):
            return pos
    raise RuntimeError("no placement of the chain on its fixed obstacles")


def make_point(cfg, kind, rng, idx):
    """one constructed point of the recipe (cfg, kind); idx picks the bound (x / y, lower / upper) and whether its stage is N"""
    m, N, K, nx, nu = cfg.m, cfg.N, cfg.K, cfg.nx, cfg.nu
    A = cfg.xy_max
    pairs = cfg.pairs()
    g0 = cfg.dmin if (cfg.pair_rows and cfg.dmin > 0) else 0.2      # the scale of a link
    hb = np.isfinite(cfg.th_max)
    coord, sgn = idx % 2, (1.0 if (idx // 2) % 2 == 0 else -1.0)
    kb = N if idx in (0, 1) else int(rng.integers(1, N))      # the stage of the x / y bound: N on two points of every recipe
    fixed = None
    if kind == "own":
        fixed = np.array(cfg.obstacles, float)
    elif kind == "static":
        fixed = np.concatenate([rng.uniform(-0.12, 0.12, (K, 2)), rng.uniform(0.08, 0.16, (K, 1))], axis=1)
        if K > 1:      # two discs press on one robot: centres closer than half a link, radii alike (the neighbours stay clear of both)
            a = rng.uniform(-np.pi, np.pi)
            fixed[1] = fixed[0] + np.array([0.16 * np.cos(a), 0.16 * np.sin(a), rng.uniform(-0.004, 0.004)])
    if fixed is not None and K > 1:
        kb = N      # two fixed contacts leave the chain no freedom for a wall: the x / y bound of such a recipe is at X_N on every point
    field = np.zeros((N, K, 3)) if kind == "moving" else None
    X = np.zeros((N + 1, m, 3)); U = np.zeros((N, m, 2))
    lam_g = np.zeros(cfg.n_g); lxX = np.zeros((N + 1, m, 3)); lxU = np.zeros((N, m, 2))

    def stage_rows(k):
        o = cfg.rows0 + k * cfg.rows_k
        return o, o + nx, o + nx + cfg.M      # defects, pair rows, obstacle rows

    for k in range(N + 1):
        inner = 1 <= k < N
        # ---- the links: binding ones carry the slack, the others are clear
        gaps = g0 * rng.uniform(1.15, 1.2 if kind in ("own", "static") else 1.4, max(m - 1, 0))
        bind = np.zeros(max(m - 1, 0), bool)
        if inner and cfg.pair_rows and m > 1:
            bind = rng.random(m - 1) < 0.6
            bind[rng.choice(m - 1, min(2, m - 1), replace=False)] = True
            gaps[bind] = np.sqrt(cfg.dmin ** 2 + _logu(rng, 1e-6, 1e-1, int(bind.sum())) * cfg.dmin ** 2)
        if k == 0 and cfg.pair_rows and m > 1:
            gaps[0] = 0.6 * cfg.dmin      # a violated stage-0 row, with a multiplier below
        wall = (coord, sgn * (A - _logu(rng, 1e-5, 1e-2))) if k == kb else None
        # ---- the obstacles of the stage: the robot each presses on changes with the stage and the obstacle; under a wall a fixed one
        #      takes one end of the chain while the other end reaches the wall
        press = [((3 * k + q + idx) % m) for q in range(K)]
        if fixed is not None:
            press = [(3 * k + idx) % m] * K      # ... fixed ones all on one robot
            jw = 0
            if wall is not None and inner:
                press = [int(rng.choice([0, m - 1]))]
                jw = m - 1 - press[0]
        oslack = _logu(rng, 1e-6, 1e-1, K) * 0.1
        if fixed is not None and inner:
            contacts = [(press[q], fixed[q, :2], cfg.rob_dim + fixed[q, 2] + cfg.margin + oslack[q]) for q in range(K)]
            def clear(pos):
                d = np.linalg.norm(pos[:, None] - fixed[None, :, :2], axis=2) - cfg.rob_dim - fixed[None, :, 2] - cfg.margin
                d[press, np.arange(K)] = 1.0
                return bool((d > 1e-3).all())
            pos = _place_on_fixed(rng, m, gaps, contacts, (jw,) + wall if wall is not None else None, A, clear)
        else:
            theta = rng.uniform(-np.pi, np.pi)
            for _ in range(50):
                pos = _chain(np.zeros(2), theta, rng.uniform(-0.12, 0.12, max(m - 1, 0)), gaps)
                cen = np.zeros((K, 3))
                for q in range(K):
                    side = theta + (0.5 * np.pi if (q + k) % 2 == 0 else -0.5 * np.pi) + rng.uniform(-0.08, 0.08)
                    cen[q, 2] = rng.uniform(0.08, 0.16)
                    cen[q, :2] = pos[press[q]] + (cfg.rob_dim + cen[q, 2] + cfg.margin + oslack[q]) * np.array([np.cos(side), np.sin(side)])
                d = np.linalg.norm(pos[:, None] - cen[None, :, :2], axis=2) - cfg.rob_dim - cen[None, :, 2] - cfg.margin
                if K:
                    d[press, np.arange(K)] = 1.0
                if (d > 1e-3).all():
                    break
            else:
                raise RuntimeError("free obstacles violated by the rest of the chain")
            if wall is not None:
                j = int(np.argmax(sgn * pos[:, coord]))
                shift = np.zeros(2)
                shift[coord] = wall[1] - pos[j, coord]
                other = pos[:, 1 - coord]
                shift[1 - coord] = rng.uniform(-0.1 * A, 0.1 * A) - other.mean()
            else:
                shift = rng.uniform(-0.1 * A, 0.1 * A, 2) - pos.mean(axis=0)
            if fixed is not None:      # stage 0 / N of a fixed field: no contact; stage 0 puts robot 0 inside obstacle 0 (a violated row that carries nothing)
                if k == 0:
                    shift = fixed[0, :2] + np.array([0.03, 0.02]) - pos[0]
            pos = pos + shift
            assert (np.abs(pos) < A).all() or k == 0, "team outside its bounds"
            if field is not None and k < N:
                cen[:, :2] += shift
                if k == 0 and K:
                    cen[0, :2] = pos[0] + np.array([0.03, 0.02])
                field[k] = cen
        X[k, :, :2] = pos
        # ---- headings: one per stage 1..N under +-th_max when there is such a bound
        tmax = min(cfg.th_max, np.pi)
        X[k, :, 2] = rng.uniform(-0.9 * tmax, 0.9 * tmax, m)
        lxX[k] = _tiny(rng, (m, 3))
        if not hb:
            lxX[k, :, 2] = rng.uniform(0.1, 0.5, m) * rng.choice([-1.0, 1.0], m)      # an unbounded heading: its multiplier carries nothing
        elif k >= 1:
            i = int(rng.integers(m)); s = rng.choice([-1.0, 1.0])
            X[k, i, 2] = s * (cfg.th_max - _logu(rng, 1e-6, 1e-2)); lxX[k, i, 2] = s * rng.uniform(0.01, 0.5)
        if wall is not None:
            j = int(np.argmin(np.abs(pos[:, coord] - wall[1])))
            X[k, j, coord] = wall[1]
            lxX[k, j, coord] = sgn * rng.uniform(0.01, 0.5)
        if k == 0:
            lxX[0] = rng.uniform(0.1, 0.5, (m, 3)) * rng.choice([-1.0, 1.0], (m, 3))
        if k == N:
            break
        # ---- controls: about a third at a bound
        ub = np.array([cfg.v_max, cfg.w_max])
        U[k] = rng.uniform(-0.8, 0.8, (m, 2)) * ub
        U[k, :, 0] = np.where(np.abs(U[k, :, 0]) < 0.1 * cfg.v_max, 0.1 * cfg.v_max, U[k, :, 0])      # a speed of size: the heading terms show
        lxU[k] = _tiny(rng, (m, 2))
        at = rng.random((m, 2)) < 1.0 / 3.0
        sg = rng.choice([-1.0, 1.0], (m, 2))
        U[k] = np.where(at, sg * (ub - _logu(rng, 1e-7, 1e-2, (m, 2))), U[k])
        lxU[k] = np.where(at, sg * rng.uniform(0.01, 0.5, (m, 2)), lxU[k])
        # ---- multipliers of the stage's rows
        od, op, oo = stage_rows(k)
        lam_g[od: od + nx] = rng.normal(0.0, 0.05, nx)
        if cfg.M:
            lp = _tiny(rng, cfg.M, negative_only=True)
            if k == 0:
                lp = -rng.uniform(0.005, 0.05, cfg.M)
            for i in np.flatnonzero(bind):
                lp[pairs.index((i, i + 1))] = -rng.uniform(0.005, 0.05)
            lam_g[op: op + cfg.M] = lp
        if K:
            lo_ = _tiny(rng, (m, K), negative_only=True)
            if k == 0:
                lo_ = -rng.uniform(0.005, 0.05, (m, K))
            elif inner:
                lo_[press, np.arange(K)] = -rng.uniform(0.005, 0.05, K)
            lam_g[oo: oo + m * K] = lo_.reshape(-1)
    # both signs of a control bound occur in every point
    ub = np.array([cfg.v_max, cfg.w_max])
    for s, (k, i, c) in ((1.0, (0, 0, 1)), (-1.0, (N - 1, m - 1, 0))):
        U[k, i, c] = s * (ub[c] - _logu(rng, 1e-7, 1e-2)); lxU[k, i, c] = s * rng.uniform(0.01, 0.5)
    lam_g[: cfg.rows0] = rng.uniform(0.1, 0.5, cfg.rows0) * rng.choice([-1.0, 1.0], cfg.rows0)      # the initial block and its pad rows carry nothing
    w = R.pack(cfg, X.reshape(N + 1, nx), U.reshape(N, nu))
    lam_x = R.pack(cfg, lxX.reshape(N + 1, nx), lxU.reshape(N, nu))
    p = np.concatenate([X[0].reshape(-1), rng.uniform(-1.0, 1.0, nx)])
    dp = rng.normal(size=2 * nx); dp /= np.linalg.norm(dp)
    obs = field if kind == "moving" else (fixed if kind == "static" else None)
    return Point(p, w, lam_g, lam_x, obs, dp)


@functools.lru_cache(maxsize=None)
def _points(i):
    r = SENS_TABLE[i]
    rng = np.random.default_rng(r.seed)
    return tuple(make_point(r.cfg, r.kind, rng, n) for n in range(NPOINTS))


def points(r):
    """the row's points, computed once per process; callers do not change them"""
    return list(_points(SENS_TABLE.index(r)))


# ---- what the host test zeroes, reverses and compares
def class_entries(cfg, cls):
    """(indices into lam_g, indices into lam_x) of a term class"""
    nx, nu, N = cfg.nx, cfg.nu, cfg.N
    k = np.arange(N)[:, None] * cfg.rows_k + cfg.rows0      # the first row of every stage block
    none = np.zeros(0, int)
    xs = np.arange(nx, (N + 1) * nx)
    if cls == "pair":
        return (k[1:] + nx + np.arange(cfg.M)[None]).reshape(-1), none
    if cls == "obstacle":
        return (k[1:] + nx + cfg.M + np.arange(cfg.m * cfg.K)[None]).reshape(-1), none
    if cls == "defect":
        return (k + np.arange(nx)[None]).reshape(-1), none
    if cls == "control":
        return none, np.arange((N + 1) * nx, cfg.n_var)
    if cls == "xy":
        return none, xs[xs % 3 != 2]
    if cls == "heading":
        return none, (xs[xs % 3 == 2] if np.isfinite(cfg.th_max) else none)
    if cls == "xN":
        return none, np.arange(N * nx, (N + 1) * nx)
    raise ValueError(cls)


def classes_of(cfg):
    """the term classes the configuration has"""
    out = ["defect", "control", "xy", "xN"]
    if cfg.M:
        out.append("pair")
    if cfg.K:
        out.append("obstacle")
    if np.isfinite(cfg.th_max):
        out.append("heading")
    return out


def zero_class(cfg, pt, cls):
    ig, ix = class_entries(cfg, cls)
    lg, lx = pt.lam_g.copy(), pt.lam_x.copy()
    lg[ig] = 0.0; lx[ix] = 0.0
    return pt._replace(lam_g=lg, lam_x=lx)


def reverse_pairs(cfg, pt):
    """the pair multipliers of every stage 1..N-1 in reverse order: what a kernel with a wrong pair index would weight the rows with"""
    lg = pt.lam_g.copy()
    for k in range(1, cfg.N):
        o = cfg.rows0 + k * cfg.rows_k + cfg.nx
        lg[o: o + cfg.M] = lg[o: o + cfg.M][::-1].copy()
    return pt._replace(lam_g=lg)


def null_masks(cfg):
    """(mask of lam_g, mask of lam_x): the entries that carry nothing by definition"""
    mg = np.zeros(cfg.n_g, bool); mx = np.zeros(cfg.n_var, bool)
    mg[: cfg.rows0] = True
    mg[cfg.rows0 + cfg.nx: cfg.rows0 + cfg.rows_k] = True      # the pair and obstacle rows of stage 0
    mx[: cfg.nx] = True
    if not np.isfinite(cfg.th_max):
        mx[2: (cfg.N + 1) * cfg.nx: 3] = True
    return mg, mx


def zero_nulls(cfg, pt):
    mg, mx = null_masks(cfg)
    return pt._replace(lam_g=np.where(mg, 0.0, pt.lam_g), lam_x=np.where(mx, 0.0, pt.lam_x))


def stage0_violation(cfg, pt):
    """whether a stage-0 pair or obstacle row is violated while it carries a multiplier (None for a configuration without such rows)"""
    if cfg.M == 0 and cfg.K == 0:
        return None
    g = R.constraints(cfg, pt.w, pt.p) if pt.obs is None else MO.constraints(cfg, pt.w, pt.p, pt.obs)
    _, _, lbg, _ = R.bounds(cfg)
    rows = np.arange(cfg.rows0 + cfg.nx, cfg.rows0 + cfg.rows_k)
    bad = rows[(g[rows] < lbg[rows]) & (pt.lam_g[rows] < 0.0)]
    return bad.size > 0


def reference(r, pt):
    return S.stage_recursion(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=pt.dp)


def deviation(a, b):
    """(gains, dw) of b against a, relative to max|G| and max|dw| of a"""
    return (float(np.abs(a["gains"] - b["gains"]).max() / np.abs(a["gains"]).max()), float(np.abs(a["dw"] - b["dw"]).max() / np.abs(a["dw"]).max()))


# ---- the verdict batch: one clean point turned into instances with a known verdict
def _xi(cfg, k, i, c):
    return k * cfg.nx + 3 * i + c


def _ui(cfg, k, i, c):
    return (cfg.N + 1) * cfg.nx + k * cfg.nu + 2 * i + c


def _quiet_heading(cfg, pt, rob):
    """the point with robot `rob` cleared of what would outweigh a negative heading curvature: no heading or turn-rate bound terms on it, no
    binding row on its position, and a speed of size at every stage"""
    w, lg, lx = pt.w.copy(), pt.lam_g.copy(), pt.lam_x.copy()
    for k in range(cfg.N + 1):
        j = _xi(cfg, k, rob, 2)
        w[j] = 0.3 + 0.1 * k; lx[j] = 0.0
        if k < cfg.N:
            j = _ui(cfg, k, rob, 1); w[j] = 0.0; lx[j] = 0.0
            j = _ui(cfg, k, rob, 0); w[j] = 0.5 * cfg.v_max; lx[j] = 0.0
    return pt._replace(w=w, lam_g=lg, lam_x=lx)


def verdict_cases(r, pt):
    """[(name, Point, expected verdict)] from one clean point of a row with pair rows, a per-stage obstacle field, a heading bound and N >= 3.
    Each case has one cause, named by the sigma / bterm call of the kernel it goes through."""
    cfg = r.cfg; m, N, K = cfg.m, cfg.N, cfg.K
    assert cfg.M and r.kind == "moving" and np.isfinite(cfg.th_max) and N >= 3
    pairs = cfg.pairs()
    out = [("clean", pt, 0)]

    def pair_case(k):      # the last link of the chain folded back to 0.6 dmin: one pair row without slack, with a multiplier
        w, lg = pt.w.copy(), pt.lam_g.copy()
        a, b = _xi(cfg, k, m - 2, 0), _xi(cfg, k, m - 1, 0)
        d = w[b: b + 2] - w[a: a + 2]
        w[b: b + 2] = w[a: a + 2] + 0.6 * cfg.dmin * d / np.linalg.norm(d)
        o = cfg.rows0 + k * cfg.rows_k + cfg.nx
        lg[o + pairs.index((m - 2, m - 1))] = -0.02
        lg[o + cfg.M + (m - 1) * K: o + cfg.M + m * K] = 0.0      # its obstacle rows moved with it: they carry nothing here
        return pt._replace(w=w, lam_g=lg)
    out.append(("pair row, stage N-1", pair_case(N - 1), 2))
    out.append(("pair row, stage 1", pair_case(1), 2))
    # an obstacle of stage 1 moved onto the robot it presses on
    k, q = 1, K - 1
    o = cfg.rows0 + k * cfg.rows_k + cfg.nx + cfg.M
    i = int(np.argmin(pt.lam_g[o: o + m * K].reshape(m, K)[:, q]))
    ob = pt.obs.copy(); ob[k, q, :2] = pt.w[_xi(cfg, k, i, 0): _xi(cfg, k, i, 0) + 2] + np.array([0.05, 0.0])
    out.append(("obstacle row", pt._replace(obs=ob), 2))
    w, lx = pt.w.copy(), pt.lam_x.copy()
    j = _xi(cfg, N, m - 1, 0); w[j] = cfg.xy_max; lx[j] = 0.2
    out.append(("x bound of X_N, w == xy_max", pt._replace(w=w, lam_x=lx), 2))
    w, lx = pt.w.copy(), pt.lam_x.copy()
    j = _ui(cfg, 1, m - 1, 0); w[j] = -cfg.v_max - 1e-3; lx[j] = -0.3
    out.append(("lower speed bound, last robot", pt._replace(w=w, lam_x=lx), 2))
    w, lx = pt.w.copy(), pt.lam_x.copy()
    j = _xi(cfg, 2, m - 1, 2); w[j] = cfg.th_max + 1e-3; lx[j] = 0.1
    out.append(("heading bound", pt._replace(w=w, lam_x=lx), 2))
    # verdict 1 through the heading of the last robot: the failing pivot belongs to a high lane
    q_ = _quiet_heading(cfg, pt, m - 1)
    lg, kk = S.indefinite_point(cfg, q_.w, q_.lam_g, value=-1e4, robot=m - 1)
    ind = q_._replace(lam_g=lg)
    out.append(("indefinite, heading of the last robot", ind, 1))
    w, lx = ind.w.copy(), ind.lam_x.copy()
    j = _ui(cfg, 0, 0, 1); w[j] = cfg.w_max + 1e-3; lx[j] = 0.3      # stage 0: looked at after the bad pivot of stage kk - 1 >= 1
    assert kk >= 2
    out.append(("no slack below the indefinite stage", ind._replace(w=w, lam_x=lx), 2))
    w, lx = ind.w.copy(), ind.lam_x.copy()
    j = _xi(cfg, N, 0, 1); w[j] = -cfg.xy_max - 1e-3; lx[j] = -0.3
    out.append(("no slack above the indefinite stage", ind._replace(w=w, lam_x=lx), 2))
    # a pair row with a positive multiplier has the wrong sign: no Sigma, its Hessian term stays in
    lg = pt.lam_g.copy()
    o = cfg.rows0 + 1 * cfg.rows_k + cfg.nx
    b = int(np.argmin(lg[o: o + cfg.M]))
    lg[o + b] = 0.03
    out.append(("pair row of the wrong sign", pt._replace(lam_g=lg), 0))
    return out


VERDICT_ROWS = [r for r in SENS_TABLE if r.field and r.m in (3, 10)]
