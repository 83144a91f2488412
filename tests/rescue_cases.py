"""Constructed inputs that take every solve-kernel instantiation (the rows of tests/kernel_variants.py) through the solver's rescue ladder:
barrier restarts after five tiny steps, the cold retry after a stall / a failed factorisation / 500 iterations, the elastic phase of the second
cold retry, and the statuses 0 and 4 it ends in.  The captured failures under tests/golden/ all come from one shape (six robots among eight
obstacles); closed loops of the other shapes do not fail, so the cases here are built, per family, from the row's own configuration:

  garbage_guess  (every row)                 helpers.batch / moving_batch inputs whose guess beyond x0 is 1e8 x standard normal.  The first
                                             attempt stalls, fails or runs into the 500-iteration watchdog; the cold retry returns status 0 at
                                             exactly the point of a solve from nlp_ref.cold_start (the retry keeps nothing of the attempt).
  overrun        (field rows with S = N)     an obstacle of radius 0.3 runs over robot 0 at stage 3, faster than the robot can leave its disc:
                                             locally infeasible.  Two attempts to the watchdog, then the elastic phase converges with an elastic
                                             variable open: status 4.
  outside_box    (every plain row)           robot 0 starts outside the position box; the states of stages 1..N are bounded, so the defects can
                                             never close: status 4 after two attempts and an elastic phase with stalls and barrier restarts of
                                             its own.  The only family that runs the elastic phase without obstacle rows, and the only one that
                                             reaches it on the element-per-lane and HBM-resident kernels.

A NaN in the guess (E0 NaN at iteration 0, then the cold retry) is not among the families: see DESIGN.md 3, rescue ladder.

The launch of a case is the row's recipe with two changes that keep a run of up to 1700 iterations short, both asserted through the
descriptor: a recipe that tiles its instances to TP_BATCH is pinned to the throughput shape (pin 3) with the small batch instead, and the ten
HBM-resident rows run pinned (pin 1) at N = 20 — their row (1, m, 0, 0, threads) does not depend on the horizon.

Every case has INSTANCES distinct instances, screened on the oracle alone (screen()): instances on which the oracle parts from itself under a
rounding-level perturbation are listed in REJECTED and replaced by the next ones drawn."""
import numpy as np

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO

INSTANCES = 8
MAX_ITER = 2500
FAMILIES = ("garbage_guess", "overrun", "outside_box")
SEED = 40          # first seed of every case; draw d of a case uses SEED + d
OVERRUN_R = 0.3    # radius of the obstacle that runs over robot 0
OVERRUN_STAGE = 3


def launch(r):
    """the recipe a rescue case of row r is launched with (see the module text): same row, small batch"""
    k, m = r.row[0], r.row[1]
    if k == 1:
        return r._replace(cfg=dict(r.cfg, N=20), B=INSTANCES, pin=1, near=None, max_iter=MAX_ITER)
    if k == 3 and r.B == KV.TP_BATCH.get(m):
        return r._replace(B=INSTANCES, pin=3, max_iter=MAX_ITER)
    # the element-per-lane kernel picks its thread count from the batch size: those recipes keep theirs and tile the instances
    return r._replace(B=r.B if r.B > 16 else INSTANCES, max_iter=MAX_ITER)


def applies(r, fam):
    if fam == "garbage_guess":
        return True
    if fam == "overrun":
        return r.obs_field == "N"
    return not r.obs_field


def cases():
    """[(row recipe, its launch recipe, family)] of every row and every family that applies to it"""
    return [(r, launch(r), fam) for r in KV.TABLE for fam in FAMILIES if applies(r, fam)]


def case_key(lr, fam):
    """rows that share a configuration (and a field kind) share a family's inputs and the oracle's answers"""
    c = lr.cfg
    return "%s-m%d-N%d-thb%d-K%d-pad%d-f%s" % (fam, c["m"], c["N"], int("th_max" in c), len(c.get("obstacles", ())), int(c["pad_rows"]), lr.obs_field)


# instances (draw, index in the draw) that find_rejected() rejects, by case key: the oracle alone would part from itself on them, or (overrun)
# the solve does not take the family's rungs (garbage_guess: the first attempt converges; overrun: an attempt ends before the watchdog; outside_box: it ends within 500 iterations of MAX_ITER)
REJECTED = {
    'garbage_guess-m1-N20-thb1-K2-pad0-f0': {(0, 1), (0, 4), (0, 7), (1, 0), (1, 1), (1, 4)},
    'garbage_guess-m1-N20-thb1-K2-pad0-f1': {(0, 0), (0, 4), (0, 6), (0, 7), (1, 0), (1, 1), (1, 2)},
    'garbage_guess-m1-N71-thb1-K2-pad0-f0': {(0, 1), (0, 7), (1, 0)},
    'garbage_guess-m1-N71-thb1-K2-pad0-f1': {(0, 0), (0, 2), (0, 3), (0, 4), (0, 5), (1, 0), (1, 1), (1, 2), (1, 6)},
    'garbage_guess-m2-N34-thb1-K2-pad1-f1': {(0, 2), (0, 5), (0, 7)},
    'garbage_guess-m2-N36-thb0-K2-pad0-fN': {(0, 5)},
    'garbage_guess-m3-N16-thb0-K0-pad1-f0': {(0, 7)},
    'garbage_guess-m3-N16-thb1-K2-pad0-f0': {(0, 6)},
    'garbage_guess-m5-N27-thb0-K8-pad0-fN': {(0, 4)},
    'garbage_guess-m6-N22-thb0-K8-pad0-fN': {(0, 3)},
    'garbage_guess-m6-N22-thb1-K8-pad1-f1': {(0, 3)},
    'garbage_guess-m9-N20-thb1-K2-pad0-f0': {(0, 4)},
    'outside_box-m2-N23-thb0-K0-pad1-f0': {(0, 7)},
    'outside_box-m3-N16-thb0-K0-pad1-f0': {(0, 2)},
    'outside_box-m3-N16-thb1-K2-pad0-f0': {(0, 2)},
    'outside_box-m3-N20-thb0-K0-pad1-f0': {(0, 2)},
    'outside_box-m3-N20-thb0-K2-pad0-f0': {(0, 2)},
    'outside_box-m3-N20-thb1-K2-pad0-f0': {(0, 2)},
    'outside_box-m3-N22-thb1-K2-pad0-f0': {(0, 2)},
    'outside_box-m5-N20-thb0-K0-pad1-f0': {(0, 1)},
    'overrun-m2-N22-thb0-K2-pad0-fN': {(0, 1)},
    'overrun-m2-N36-thb0-K2-pad0-fN': {(0, 3), (0, 6)},
    'overrun-m3-N23-thb0-K2-pad0-fN': {(0, 2)},
    'overrun-m4-N20-thb0-K2-pad0-fN': {(0, 3)},
    'overrun-m5-N20-thb0-K2-pad0-fN': {(0, 0), (0, 6)},
    'overrun-m5-N27-thb0-K8-pad0-fN': {(0, 4)},
    'overrun-m6-N22-thb0-K8-pad0-fN': {(0, 6)},
    'overrun-m9-N20-thb0-K2-pad0-fN': {(0, 6)},
}


# ---- one draw of INSTANCES instances per family: (P, W0, F or None) ------------------------------------------------------------------------
def _draw_garbage(cfg, obs_field, seed):
    if obs_field:
        P, W0, F = MO.moving_batch(cfg, INSTANCES, 900 + seed)
        if obs_field == 1:
            F = np.ascontiguousarray(F[:, :1])
    else:
        (P, W0), F = Hh.batch(cfg, INSTANCES, seed), None
    W0 = W0.copy()
    W0[:, cfg.nx:] = 1e8 * np.random.default_rng(7000 + seed).standard_normal((INSTANCES, cfg.n_var - cfg.nx))
    return P, W0, F


def _draw_overrun(cfg, obs_field, seed):
    """The field [N, K, 3]: obstacle 0 moves on a straight line whose closest point to robot 0's start, at a lateral offset of 0.05 .. 0.5 of
    the clearance rob_dim + r + margin (never through the centre: the row's gradient would be 0 / 0), is reached at stage OVERRUN_STAGE; its
    speed puts entry 0 at the clearance + 0.05 from that start, so x0 is feasible.  The robot cannot cover the distance to the disc's rim in
    three stages.  The other obstacles are parked at (5 + q, 5 + q).  Resampled until entry 0 clears every robot."""
    assert obs_field == "N"
    rng = np.random.default_rng(8000 + seed)
    N, K, T, m = cfg.N, cfg.K, cfg.T, cfg.m
    clear = cfg.rob_dim + OVERRUN_R + cfg.margin
    assert OVERRUN_STAGE * T * cfg.v_max < 0.5 * clear      # three stages at full speed do not reach the rim from the largest offset
    k = np.arange(N, dtype=np.float64)
    P, F = [], []
    while len(P) < INSTANCES:
        s = Hh.sample_points(rng, m, cfg.dmin + 0.1)
        g = Hh.sample_points(rng, m, cfg.dmin + 0.1)
        off = rng.uniform(0.05, 0.5) * clear
        a = rng.uniform(-np.pi, np.pi)
        d, n = np.array([np.cos(a), np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
        run = np.sqrt((clear + 0.05) ** 2 - off ** 2)       # along the path, from entry 0 to the closest point
        f = np.empty((N, K, 3))
        f[:, 0, :2] = s[0] + off * n + ((k - OVERRUN_STAGE) / OVERRUN_STAGE * run)[:, None] * d
        f[:, 0, 2] = OVERRUN_R
        for q in range(1, K):
            f[:, q] = (5.0 + q, 5.0 + q, 0.1)
        if (np.linalg.norm(s - f[0, 0, :2], axis=1) - cfg.rob_dim - OVERRUN_R < cfg.margin + 0.04).any():
            continue
        x0 = np.concatenate([s, rng.uniform(-np.pi, np.pi, (m, 1))], axis=1).reshape(-1)
        xs = np.concatenate([g, rng.uniform(-np.pi, np.pi, (m, 1))], axis=1).reshape(-1)
        P.append(np.concatenate([x0, xs])); F.append(f)
    P = np.stack(P)
    return P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P]), np.stack(F)


def _draw_outside(cfg, obs_field, seed):
    assert not obs_field
    P, _ = Hh.batch(cfg, INSTANCES, seed)
    P = P.copy()
    P[:, 0] = cfg.xy_max + np.random.default_rng(9000 + seed).uniform(0.05, 1.0, INSTANCES)
    return P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P]), None


_DRAW = {"garbage_guess": _draw_garbage, "overrun": _draw_overrun, "outside_box": _draw_outside}
_cache = {}


def draw(lr, fam, d):
    cfg = R.NLPConfig(**lr.cfg)
    return (cfg,) + _DRAW[fam](cfg, lr.obs_field, SEED + d)


def inputs(lr, fam):
    """(oracle config, P, W0, F or None, picks) of the INSTANCES distinct instances of a case: the draws SEED, SEED + 1, ... in order without
    the instances of REJECTED; picks = [(draw, index)].  Cached per case key."""
    key = case_key(lr, fam)
    if key not in _cache:
        rej = REJECTED.get(key, set())
        P, W0, F, picks, d = [], [], [], [], 0
        while len(picks) < INSTANCES:
            cfg, p, w, f = draw(lr, fam, d)
            for j in range(INSTANCES):
                if (d, j) not in rej and len(picks) < INSTANCES:
                    P.append(p[j]); W0.append(w[j]); F.append(f[j] if f is not None else None); picks.append((d, j))
            d += 1
            assert d < 50, key
        _cache[key] = (cfg, np.stack(P), np.stack(W0), np.stack(F) if F[0] is not None else None, picks)
    return _cache[key]


def tiled(lr, P, W0, F):
    """the instances repeated in order up to the launch's batch"""
    idx = np.arange(lr.B) % P.shape[0]
    return np.ascontiguousarray(P[idx]), np.ascontiguousarray(W0[idx]), (np.ascontiguousarray(F[idx]) if F is not None else None)


_ref = {}


def oracle(lr, fam):
    """the oracle's answer on a case's instances, with its ladder counters [INSTANCES, 3] (cold retries begun, barrier restarts, elastic
    iterations) under "ladder".  Computed once per case key; callers must not change it."""
    from oracle import oracle_lib as O
    key = case_key(lr, fam)
    if key not in _ref:
        cfg, P, W0, F, _ = inputs(lr, fam)
        a, lad = O.with_ladder_stats(P.shape[0], lambda: KV.oracle_solve(cfg, P, W0, F, MAX_ITER))
        a["ladder"] = lad
        for v in a.values():
            v.setflags(write=False)
        _ref[key] = a
    return _ref[key]


def cold_inputs(cfg, P):
    """the guess of nlp_ref.cold_start for every instance"""
    return np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P])


def screen_instances(cfg, fam, P, W0, F, a=None):
    """Per instance: the oracle holds its status under KV.SCREEN_DRAWS draws of KV.perturbed, and its point to KV.SCREEN_TOL; for the two
    status-4 families its iteration count as well (the length of a garbage_guess's failed attempt is rounding-sensitive; what it ends in is
    not)."""
    a = KV.oracle_solve(cfg, P, W0, F, MAX_ITER) if a is None else a
    n = P.shape[0]
    pert = [KV.perturbed(cfg, P, W0, seed=s) for s in range(KV.SCREEN_DRAWS)]      # the draws as one batch: one parallel oracle call
    b = KV.oracle_solve(cfg, np.concatenate([q[0] for q in pert]), np.concatenate([q[1] for q in pert]),
                        np.concatenate([F] * KV.SCREEN_DRAWS) if F is not None else None, MAX_ITER)
    ok = np.ones(n, dtype=bool)
    for s in range(KV.SCREEN_DRAWS):
        sl = slice(s * n, (s + 1) * n)
        ok &= (a["status"] == b["status"][sl]) & (np.max(np.abs(a["x"] - b["x"][sl]), axis=1) <= KV.SCREEN_TOL)
        if fam != "garbage_guess":
            ok &= a["iters"] == b["iters"][sl]
    return ok, a


def screen(lr, fam):
    """(every instance of the case holds, the oracle's statuses, its iteration counts)"""
    cfg, P, W0, F, _ = inputs(lr, fam)
    ok, a = screen_instances(cfg, fam, P, W0, F, oracle(lr, fam))
    return ok, a["status"], a["iters"]


def find_rejected(lr, fam):
    """how REJECTED is made: walk the draws, screen each, until INSTANCES instances hold; returns the set of (draw, index) that do not.  An
    instance must also end in the family's status after its number of cold retries (a garbage guess that the push into the bounds alone turns
    into a start from which the first attempt converges needs none), an overrun after two attempts that both reach the watchdog (one that stalls earlier is
    as valid a solve, but not the path the family is for)."""
    from oracle import oracle_lib as O
    want = 0 if fam == "garbage_guess" else 4
    rej, kept, d = set(), 0, 0
    while kept < INSTANCES:
        cfg, P, W0, F = draw(lr, fam, d)
        a, lad = O.with_ladder_stats(INSTANCES, lambda: KV.oracle_solve(cfg, P, W0, F, MAX_ITER))
        ok, a = screen_instances(cfg, fam, P, W0, F, a)
        ok &= (a["status"] == want) & (lad[:, 0] == (1 if fam == "garbage_guess" else 2))
        if fam == "outside_box":      # far from the cap, so that no status depends on MAX_ITER (the family ends after 1300 .. 1850 iterations)
            ok &= a["iters"] < MAX_ITER - 500
        if fam == "overrun":      # both attempts to the watchdog, an obstacle row left open
            ok &= (a["iters"] > 1000) & (a["iters"] < 1100)
            ok &= np.array([MO.obstacle_values(cfg, a["x"][j], F[j]).min() < cfg.margin - 1e-3 for j in range(INSTANCES)])
        for j in range(INSTANCES):
            if kept < INSTANCES:
                if ok[j]:
                    kept += 1
                else:
                    rej.add((d, j))
        d += 1
        assert d < 50, (case_key(lr, fam), sorted(rej))
    return rej
