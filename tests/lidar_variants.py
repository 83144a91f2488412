"""The table of every LIDAR solve-kernel instantiation of libnmpc_hip.so (csrc/nmpc_lidar.hip), and the recipes that walk each one along the
edges of its shape handling.

A row names the instantiation nmpc_debug_lidar_variant() must return for it: (rays, waves) = the template arguments in the mangled name of
lidar_solve_kernel<R_, W_>: <10, 1> and <10, 2> (the scripts' ray count; one or two resident waves per SIMD) and <-1, 1> (any other count:
loops unrolled to 16 rays, the surplus predicated off, loads clamped and issued in chunks of NMPC_LIDAR_CH = 5).
tests/test_lidar_variants_host.py holds the table against the symbols of the built code object and screens every recipe on the CPU;
tests/test_gpu_lidar_variants.py asserts that the descriptor returns the row's instantiation and solves it against the oracle.

What the recipes move, and why:
  * R: 0 (no ray term, zero-length per-ray arrays), 1, 2, the chunk edges 5 | 6, 9 | 11 next to the specialised 10, 15 | 16 (16: no surplus);
  * N: 1..5 and 9 (remainders of the recursions' unroll by NMPC_LIDAR_UNROLL = 4, a horizon shorter than one unrolled group), 63 | 64 | 65 and
    127 | 128 | 129 (the `k = lane; k < N; k += 64` strides of the stage-parallel phases);
  * Nc: 1 (one control held over the horizon, cnt = N - Nc + 1 on its cost terms), N / 2, N (no held control);
  * the bound branches (isfinite(), n_ineq) and lw = 0: VARIANTS;
  * the two-waves-per-SIMD build: batches one beyond the descriptor's threshold (B = None here: the GPU test reads the threshold).

Inputs: the generator of the LIDAR parity tests (batch(), aligned bounds), max_iter 600.  Instance 1 of every recipe is made infeasible at
stage 0 (a scan below d_min; without rays a pose beyond xy_max), so every shape also runs the kernel's early-return write-out.
A recipe's seed is the first of 5, 6, ... on which screen() holds; no recipe is exempt.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import lidar_ref as LR

INF = float("inf")
MAX_ITER = 600
SEED0 = 5
# distinct (screened) instances of a two-wave recipe, repeated in order by a larger batch.  1100: beyond one robot per SIMD of a 256-CU
# device, so every instance of such a batch is its own.  (65, 1): with one control held over 65 stages about one generator instance in 200
# reaches the iteration limit on the oracle (seeds 5..24 measured: never 1100 clean ones), so that shape repeats 64 screened instances.
W2_DISTINCT = 1100
W2_DISTINCT_BY_SHAPE = {(65, 1): 64}

Recipe = namedtuple("Recipe", "inst N Nc R over B seed max_iter")
# inst: (rays, waves) template arguments; over: overrides of oracle.lidar_ref.LidarConfig (a key of VARIANTS); B: batch, None = the
# descriptor's two-wave threshold + 1; seed: of batch()

VARIANTS = {
    "base": {},
    "lw0": dict(lw=0.0),                                           # V3's cost: no 1/d^2 term
    "dmax_inf": dict(d_max=INF),                                   # V3's distance bounds: lower only
    "th2": dict(th_max=2.0),                                       # a finite heading bound: both pose-angle branches live
    "lw0_free": dict(lw=0.0, d_max=INF, xy_max=INF),               # only d >= d_min left on the states
}
SHORT_N = (1, 2, 3, 4, 5, 9)
LANE_N = (63, 64, 65, 127, 128, 129)
VARIANT_SHAPES = ((3, 1, 16), (9, 4, 5), (65, 32, 11), (64, 64, 10))
W2_SHAPES = ((5, 2), (8, 4), (12, 6), (65, 1))
W2_VARIANT_SHAPE = (8, 4)


def _ncs(N):
    return sorted({1, max(1, N // 2), N})


def _inst(R, B):
    return (10, 2 if B is None else 1) if R == 10 else (-1, 1)


def _rows():
    out = []

    def add(N, Nc, R, over="base", B=16):
        out.append(Recipe(_inst(R, B), N, Nc, R, over, B, SEED0, MAX_ITER))
    for R in (0, 1, 2, 5, 6, 9, 11, 15, 16):
        for N in SHORT_N:
            for Nc in _ncs(N):
                add(N, Nc, R)
    for R in (0, 5, 11, 16):
        for N in LANE_N:
            for Nc in _ncs(N):
                add(N, Nc, R)
    for N in SHORT_N + LANE_N:
        for Nc in _ncs(N):
            add(N, Nc, 10)
    for (N, Nc) in W2_SHAPES:
        add(N, Nc, 10, B=None)
    for v in VARIANTS:
        if v != "base":
            for (N, Nc, R) in VARIANT_SHAPES:
                add(N, Nc, R, over=v)
            add(W2_VARIANT_SHAPE[0], W2_VARIANT_SHAPE[1], 10, over=v, B=None)
    return out


def row_key(r):
    return (r.inst, r.N, r.Nc, r.R, r.over)


def row_id(r):
    return "r%dw%d-N%d-Nc%d-R%d-%s" % (r.inst[0], r.inst[1], r.N, r.Nc, r.R, r.over)


# seeds other than SEED0, where screen() rejects it (an instance at the iteration limit, or the oracle parting from itself under the
# rounding-level perturbation): filled by running screen() over seeds SEED0, SEED0 + 1, ... on the CPU
SEEDS = {((-1, 1), 128, 128, 0, 'base'): 6, ((-1, 1), 128, 1, 11, 'base'): 6, ((-1, 1), 129, 1, 11, 'base'): 7, ((-1, 1), 127, 63, 16, 'base'): 6,
         ((10, 1), 127, 1, 10, 'base'): 6, ((10, 1), 128, 1, 10, 'base'): 6, ((10, 1), 129, 1, 10, 'base'): 6, ((-1, 1), 65, 32, 11, 'th2'): 6}
TABLE = [r._replace(seed=SEEDS.get(row_key(r), r.seed)) for r in _rows()]


def config(r):
    return LR.LidarConfig(N=r.N, Nc=r.Nc, R=r.R, aligned_bounds=True, **VARIANTS[r.over])


def world(rng):
    return [(float(rng.uniform(0.8, 2.6)), float(rng.uniform(0.3, 2.4)), float(rng.uniform(0.15, 0.3))) for _ in range(3)] + \
           [(float(rng.uniform(-1.5, 0.5)), float(rng.uniform(-1.5, -0.5)), 0.2)]


def batch(cfg, B, seed, goal=(3.0, 2.5, 0.0)):
    """robots near the origin looking into the first quadrant (the script's start, V4:184), synthetic scans of a random world of
    circular obstacles, the script's first goal (V4:221).  Instance b does not depend on B: a shorter batch is a prefix of a longer one."""
    rng = np.random.Generator(np.random.PCG64(20210141 + seed))
    P, W0 = [], []
    for _ in range(B):
        if cfg.aligned_bounds:
            pose = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 1.2)])
        else:       # the script's misaligned bounds force x, y, theta >= d_min from stage ~24 (V4) / ~29 (V3) on: start where that is reachable
            pose = np.array([rng.uniform(0.0, 0.15), rng.uniform(0.0, 0.15), rng.uniform(0.4, 1.1)])
        scan = LR.scan_of_world(pose, world(rng), cfg.R)
        xs = np.array(goal) + rng.uniform(-0.3, 0.3, 3)
        P.append(LR.make_p(cfg, pose, xs, scan)); W0.append(LR.cold_start(cfg, np.concatenate([pose, scan])))
    return np.stack(P), np.stack(W0)


def distinct(r):
    """number of distinct instances of a recipe"""
    return W2_DISTINCT_BY_SHAPE.get((r.N, r.Nc), W2_DISTINCT) if r.B is None else r.B


def inputs(r, B=None):
    """(oracle config, P [B, n_p], W0 [B, n_var]) of a recipe; B: the batch of a two-wave recipe (beyond W2_DISTINCT the instances repeat in
    order).  Instance 1 is infeasible at stage 0: its first ray reads 0.05 < d_min, or (no rays) its pose lies one metre beyond xy_max; its
    guess stays the cold start of the feasible reading."""
    cfg = config(r)
    n = distinct(r)
    P, W0 = batch(cfg, n, r.seed)
    if cfg.R > 0:
        P[1, 6] = 0.05
    else:
        assert math.isfinite(cfg.xy_max)
        P[1, 0] = cfg.xy_max + 1.0
    B = n if B is None else B
    if B != n:
        idx = np.arange(B) % n
        P, W0 = P[idx], W0[idx]
    return cfg, np.ascontiguousarray(P), np.ascontiguousarray(W0)


def perturbed(cfg, P, W0, seed=0):
    """the inputs with the goal and w0 (stages 1.., controls) moved by a few ulp: relative 2.2e-16 x {-2..2}, absolute 1e-17, seeded; the
    pose, the scan and stage 0 of w0 stay (they are pinned)"""
    rng = np.random.default_rng(1000 + seed)

    def pert(a):
        return a * (1.0 + 2.2e-16 * rng.integers(-2, 3, a.shape)) + 1e-17 * rng.choice([-1.0, 1.0], a.shape)
    P2, W2 = P.copy(), pert(W0)
    P2[:, 3:6] = pert(P[:, 3:6])
    W2[:, : cfg.ns] = W0[:, : cfg.ns]
    return P2, W2


def oracle_solve(cfg, P, W0, max_iter):
    from oracle import oracle_lib as O
    return O.lidar_solve_batch(cfg, P, W0, max_iter=max_iter)


SCREEN_TOL = 1e-8      # as kernel_variants.SCREEN_TOL: two decades below the parity tolerance of 1e-6
SCREEN_DRAWS = 2
Screen = namedtuple("Screen", "status_equal converged held spread iters")
_SCREENED = {}


def screen(r):
    """The oracle against itself on a recipe's distinct instances under SCREEN_DRAWS draws of `perturbed`: status vectors equal on every
    draw; every instance but instance 1 (status 3 by construction) converged; every instance holds its point to SCREEN_TOL and its
    iteration count.  spread: the largest distance of the oracle's point from itself over the draws (the rounding-level spread the
    budget-independence tolerance is taken from); iters: the longest solve.  Computed once per recipe and process."""
    key = (row_key(r), r.seed)
    if key not in _SCREENED:
        cfg, P, W0 = inputs(r)
        a = oracle_solve(cfg, P, W0, r.max_iter)
        want = np.zeros(P.shape[0], dtype=np.int32); want[1] = 3
        status_equal, conv, held, spread = True, bool((a["status"] == want).all()), True, 0.0
        for s in range(SCREEN_DRAWS):
            P2, W2 = perturbed(cfg, P, W0, seed=s)
            b = oracle_solve(cfg, P2, W2, r.max_iter)
            status_equal = status_equal and bool((a["status"] == b["status"]).all())
            conv = conv and bool((b["status"] == want).all())
            ok = a["status"] == 0
            d = float(np.max(np.abs(a["x"][ok] - b["x"][ok]))) if ok.any() else 0.0
            spread = max(spread, d)
            held = held and d <= SCREEN_TOL and bool((a["iters"] == b["iters"]).all())
        _SCREENED[key] = Screen(status_equal, conv, held, spread, int(a["iters"].max()))
    return _SCREENED[key]


def budget_tolerance(spread):
    """the spread -> tolerance rule of tests/kernel_variants.PATHS: 100 x the oracle's own spread (two fp64 builds of one kernel differ by
    summation order and contraction, two decades cover that without admitting a wrong term), at least 1e-12"""
    return max(100.0 * spread, 1e-12)
