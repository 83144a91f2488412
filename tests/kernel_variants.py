"""The table of every solve-kernel instantiation of libnmpc_hip.so, and for each the recipe that makes the library launch it.

A row is the tuple of nmpc_debug_variant(): (kernel, m, thb, flags, threads) = the template arguments in the mangled name of
solve_kernel<M, TPB> (kernel 1, HBM-resident), solve_lds_kernel<M, THB, TPB> (2, element-per-lane) or solve_col_kernel<M, THB, DL, TPB>
(3, column-per-lane).  tests/test_kernel_variants_host.py holds the table against the symbols of the built code object;
tests/test_gpu_kernel_variants.py asserts that the descriptor returns the row for its recipe and solves it against the oracle.

The rows are written from the instantiation rules of the sources:
  * column kernel (csrc/nmpc_solve_col.hip, ColInst / select3_mt), per heading flag and per field flag (DL | 4):
      throughput shape, 64 threads: DL = 0 (duals in the workspace) for every team size, DL = 1 (duals in LDS) up to four robots,
                                    DL = 2 (stage factors in LDS too) for two robots;
      latency shape, 128 threads:   DL = 1 up to six robots, DL = 0 beyond;   256 threads: DL = 1, five and six robots only;
  * element-per-lane kernel (csrc/nmpc_solve_lds.hip, lds_threads): 64 threads up to six robots, 128 for seven and eight, 256 for nine and
    ten, per heading flag; five and six robots also at 128 and 256 threads (latency shapes);
  * HBM-resident kernel (csrc/nmpc_kernels.hip, solve_threads): 64 threads up to six robots, 128 beyond; no heading flag in its name.

The horizons at which a flag flips were read once from the descriptor on an MI355X (it makes no launch) and are literals here: the shortest
horizon with the duals out of LDS (DUALS_OUT), with the stage factors out of LDS (FACTORS_OUT, two robots), and the shortest one the
library runs on the HBM-resident kernel (KERNEL1); they depend on (m, heading flag, number of obstacles).  A pin (nmpc_options_t.kernel) is
used only where the library's own choice cannot reach the row:
  * the latency shape up to three robots (pin 4): the library's own choice for them is the throughput shape at every batch size;
  * every element-per-lane row (pin 2): the library's own choice never launches that kernel.  solve_plan() takes it where the column
    kernel's latency shape does not fit the LDS and the element-per-lane kernel does, but for every team size, heading flag and obstacle
    count the element-per-lane kernel outgrows the 160 KB first (five robots, no obstacles: N = 113 against N = 120; six: 89 against 97;
    from seven robots on the latency shape is the throughput shape's size and the handle leaves the column kernel with it).
    test_own_choice_never_launches_the_element_kernel holds this.
The throughput shape from four robots on is the library's choice beyond twice the instances the latency shape holds at once (B = 2049 up to
six robots, 1025 beyond, on the 256 compute units of an MI355X): those recipes tile their 16 screened instances to that batch.
No instantiation is unreachable.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import moving_obstacles_ref as MO

TH_MAX = 3.5          # finite heading bound of the THB = 1 rows: above pi, so every sampled heading is feasible
OBSTACLES2 = [(0.45, 0.1, 0.15), (-0.3, 0.5, 0.125)]      # the two obstacles of helpers.cfg_mix3


def obstacles8():
    """the eight obstacles of the synthetic composite (tests/test_gpu_parity._composite_cfg)"""
    rng = np.random.default_rng(7)
    return [(float(x), float(y), float(r)) for x, y, r in zip(rng.uniform(-1.5, 1.5, 8), rng.uniform(-1.5, 1.5, 8), rng.uniform(0.125, 0.2, 8))]


# shortest horizon with the slacks and duals of the throughput shape out of LDS, by (m, thb, K)
DUALS_OUT = {(1, 0, 0): 85, (1, 0, 2): 75, (1, 1, 0): 80, (1, 1, 2): 71, (2, 0, 0): 41, (2, 0, 2): 36, (2, 1, 0): 39, (2, 1, 2): 34,
             (3, 0, 0): 26, (3, 0, 2): 23, (3, 1, 0): 25, (3, 1, 2): 22, (4, 0, 0): 19, (4, 0, 2): 17, (4, 1, 0): 18, (4, 1, 2): 16}
# two robots: shortest horizon with the stage factors out of LDS (the duals still in it)
FACTORS_OUT = {(2, 0, 0): 23, (2, 0, 2): 22, (2, 1, 0): 23, (2, 1, 2): 21}
# shortest horizon the library runs on the HBM-resident kernel (the column kernel's iterate no longer fits 160 KB of LDS), by m
KERNEL1 = {1: 1137, 2: 568, 3: 379, 4: 284, 5: 227, 6: 189, 7: 162, 8: 142, 9: 126, 10: 113}
# shortest horizon at which five / six robots among eight obstacles have more than 1000 obstacle items (N - 1) m K: four wavefronts
WAVES4 = {5: 27, 6: 22}
# smallest batch the library runs in the column kernel's throughput shape from four robots on (twice the latency shape's slots, plus one)
TP_BATCH = {4: 2049, 5: 2049, 6: 2049, 7: 1025, 8: 1025, 9: 1025, 10: 1025}

Recipe = namedtuple("Recipe", "row cfg B pin ordered obs_field seed near max_iter")
# row: (kernel, m, thb, flags, threads); cfg: keywords of oracle.nlp_ref.NLPConfig (= the ProblemConfig literals); B: batch (beyond 16: the 16
# instances tiled); pin: nmpc_options_t.kernel; ordered: solve with a dispatch-order hint; obs_field: 0 plain call, 1 an *_obs call with a
# static field per instance (S = 1), "N" with a moving field (S = N); seed: of the inputs; near: None = starts and goals as helpers.instance,
# else goals within that distance of the starts (the long horizons, which would otherwise solve for hundreds of iterations)


def literals(m):
    """the scripts' literals by team size, as moving_obstacles_ref.team_cfg"""
    if m == 1:
        return dict(T=0.2, dmin=0.0, v_max=0.2, w_max=1.0)
    return dict(T=0.3, dmin=0.4, v_max=0.15, w_max=1.5) if m <= 6 else dict(T=0.1, dmin=0.3, v_max=0.22, w_max=2.84)


def _cfg(m, N, thb, K, pad):
    d = dict(m=m, N=N, rob_dim=0.2, margin=0.1, pad_rows=bool(pad and m > 1), **literals(m))
    if thb:
        d["th_max"] = TH_MAX
    if K:
        d["obstacles"] = obstacles8() if K == 8 else OBSTACLES2[:K]
    return d


def _column_rows():
    out = []
    for thb in (0, 1):
        for ob in (0, 4):
            # obstacles: the field rows need them; the plain rows carry two with the heading bound and none without.  pad_rows: off on the
            # plain rows with the heading bound and on the field rows without, on elsewhere.  The field is static (S = 1) with the heading
            # bound and moving (S = N) without.
            K = 2 if (ob or thb) else 0
            pad = (thb == 0) if not ob else (thb == 1)
            fld = 0 if not ob else (1 if thb else "N")
            for m in range(1, 11):
                own_tp = m <= 3      # the library's own choice is the throughput shape at every batch size
                tpB, tp_pin = (16, 0) if own_tp else (TP_BATCH[m], 0)
                if m <= 4:
                    short = {1: 20, 2: 16, 3: 16, 4: 12}[m]      # duals (and, two robots, factors) in LDS
                    out.append(Recipe((3, m, thb, (2 if m == 2 else 1) | ob, 64), _cfg(m, short, thb, K, pad), tpB, tp_pin, 0, fld, 5, None, 400))
                    if m == 2:
                        out.append(Recipe((3, m, thb, 1 | ob, 64), _cfg(m, FACTORS_OUT[(m, thb, K)], thb, K, pad), tpB, tp_pin, 0, fld, 5, None, 400))
                    out.append(Recipe((3, m, thb, 0 | ob, 64), _cfg(m, DUALS_OUT[(m, thb, K)], thb, K, pad), tpB, tp_pin, 0, fld, 5, None, 400))
                else:
                    out.append(Recipe((3, m, thb, 0 | ob, 64), _cfg(m, 20, thb, K, pad), tpB, tp_pin, 0, fld, 5, None, 400))
                lat = 1 if m <= 6 else 0
                # latency shape, two wavefronts: pinned up to three robots, the library's own choice for a small batch beyond (with a
                # dispatch-order hint on the rows with the heading bound)
                out.append(Recipe((3, m, thb, lat | ob, 128), _cfg(m, 20, thb, K, pad), 16, 4 if m <= 3 else 0, int(m >= 4 and thb == 1), fld, 5, None, 400))
                if m in (5, 6):      # four wavefronts: the library's own choice with more than 1000 obstacle items
                    out.append(Recipe((3, m, thb, lat | ob, 256), _cfg(m, WAVES4[m], thb, 8, pad), 16, 0, 0, fld, 5, None, 600))
    return out


def _element_rows():
    out = []
    for thb in (0, 1):
        K, pad = (2, False) if thb else (0, True)
        for m in range(1, 11):
            tp = 64 if m <= 6 else (128 if m <= 8 else 256)
            # five and six robots: 256 threads up to B = 256, 128 up to 512, the throughput shape's 64 beyond
            out.append(Recipe((2, m, thb, 0, tp), _cfg(m, 20, thb, K, pad), 513 if m in (5, 6) else 16, 2, 0, 0, 5, None, 400))
            if m in (5, 6):
                out.append(Recipe((2, m, thb, 0, 128), _cfg(m, 20, thb, K, pad), 257, 2, 0, 0, 5, None, 400))
                out.append(Recipe((2, m, thb, 0, 256), _cfg(m, 20, thb, K, pad), 16, 2, 0, 0, 5, None, 400))
    return out


def _hbm_rows():
    """the library's own choice at the shortest horizon beyond the LDS; the heading bound on the even team sizes, two obstacles up to six robots
    and on eight, pad_rows on the even team sizes; goals near the starts so that the solves stay short"""
    return [Recipe((1, m, 0, 0, 64 if m <= 6 else 128), _cfg(m, KERNEL1[m], int(m % 2 == 0), 2 if (m <= 6 or m == 8) else 0, m % 2 == 0),
                   4, 0, 0, 0, 5, 0.3, 400) for m in range(1, 11)]


TABLE = _column_rows() + _element_rows() + _hbm_rows()

# seeds other than 5, where the screening below rejects 5 (the oracle alone would part from itself under a rounding-level perturbation, or
# the longest solve takes more than 100 iterations)
SEEDS = {(1, 1, 0, 0, 64): 17, (2, 3, 0, 0, 64): 6, (2, 6, 0, 0, 64): 6, (2, 6, 0, 0, 128): 6, (2, 6, 0, 0, 256): 6,
         (2, 8, 1, 0, 128): 6, (2, 9, 0, 0, 256): 7, (2, 10, 0, 0, 256): 6, (3, 1, 0, 4, 64): 9, (3, 3, 0, 1, 128): 6,
         (3, 5, 0, 1, 256): 6, (3, 5, 1, 1, 256): 6, (3, 5, 1, 5, 256): 6, (3, 6, 0, 0, 64): 6, (3, 6, 0, 1, 128): 6,
         (3, 6, 0, 1, 256): 6, (3, 6, 1, 1, 256): 6, (3, 7, 1, 4, 64): 6, (3, 7, 1, 4, 128): 6, (3, 8, 1, 0, 64): 6,
         (3, 8, 1, 0, 128): 6, (3, 9, 0, 0, 64): 7, (3, 9, 0, 0, 128): 7, (3, 10, 0, 0, 64): 6, (3, 10, 0, 0, 128): 6,
         (3, 10, 1, 4, 64): 6, (3, 10, 1, 4, 128): 6}
TABLE = [r._replace(seed=SEEDS.get(r.row, r.seed)) for r in TABLE]


def row_id(r):
    return "k%d-m%d-thb%d-dl%d-t%d" % r.row


def c_config(cfg, max_iter):
    """the nmpc_config_t of an oracle config"""
    return Hh.to_product_cfg(cfg, max_iter=max_iter).to_c()


def variant_of_config(cc, pin, cus, B, ordered, obs_field):
    """nmpc_debug_variant_of_config on an nmpc_config_t: (return code, (kernel, m, thb, flags, threads), LDS bytes, kernel code 1..4) of the
    launch a handle with that pin makes on a device with `cus` compute units; needs no handle and no device"""
    import ctypes as C
    import nmpc_amd
    lib = nmpc_amd._lib
    v, k = lib.CDebugVariant(), C.c_int32(0)
    rc = lib.load().nmpc_debug_variant_of_config(C.byref(cc), C.byref(lib.COptions(kernel=pin, trace_instance=-1)), cus, B, int(ordered), int(bool(obs_field)),
                                                C.byref(v), C.byref(k))
    return rc, (v.kernel, v.m, v.thb, v.flags, v.threads), int(v.lds_bytes), k.value


def near_batch(cfg, B, seed, radius):
    """starts as helpers.instance; each goal within `radius` (per axis) of its robot's start, heading within 0.3 rad, the goals as far apart
    as the starts must be"""
    rng = np.random.Generator(np.random.PCG64(Hh.SEED0 + seed))
    P = []
    for _ in range(B):
        p = Hh.instance(rng, cfg)
        x0 = p[: cfg.nx].reshape(cfg.m, 3)
        while True:
            g = x0 + np.concatenate([rng.uniform(-radius, radius, (cfg.m, 2)), rng.uniform(-0.3, 0.3, (cfg.m, 1))], axis=1)
            d = [np.hypot(*(g[i, :2] - g[j, :2])) for i in range(cfg.m) for j in range(i + 1, cfg.m)]
            clear = all(np.hypot(g[i, 0] - ox, g[i, 1] - oy) >= cfg.rob_dim + cfg.margin + 0.05 + orad for i in range(cfg.m) for (ox, oy, orad) in cfg.obstacles)
            if (not d or min(d) >= cfg.dmin + 0.1) and clear:
                break
        P.append(np.concatenate([x0.reshape(-1), g.reshape(-1)]))
    P = np.stack(P)
    return P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P])


def inputs(r):
    """(oracle config, P [B, 2 nx], W0 [B, nvar], field [B, S, K, 3] or None) of a recipe.  At most 16 distinct instances: a larger batch
    repeats them in order."""
    cfg = R.NLPConfig(**r.cfg)
    nb = min(r.B, 16)
    F = None
    if r.obs_field:
        P, W0, F = MO.moving_batch(cfg, nb, 900 + r.seed)
        if r.obs_field == 1:
            F = np.ascontiguousarray(F[:, :1])      # the field of stage 0, held: S = 1
    elif r.near is not None:
        P, W0 = near_batch(cfg, nb, r.seed, r.near)
    else:
        P, W0 = Hh.batch(cfg, nb, r.seed)
    if r.B > nb:
        idx = np.arange(r.B) % nb
        P, W0 = P[idx], W0[idx]
        F = F[idx] if F is not None else None
    return cfg, np.ascontiguousarray(P), np.ascontiguousarray(W0), F


def perturbed(cfg, P, W0, seed=0):
    """the inputs with w0 and the goals moved at rounding level: relative 2.2e-16, absolute 1e-17, random signs (x0 stays: it is pinned)"""
    rng = np.random.default_rng(1000 + seed)

    def pert(a):
        return a * (1.0 + 2.2e-16 * rng.choice([-1.0, 1.0], a.shape)) + 1e-17 * rng.choice([-1.0, 1.0], a.shape)
    P2 = P.copy()
    P2[:, cfg.nx:] = pert(P[:, cfg.nx:])
    W2 = pert(W0)
    W2[:, : cfg.nx] = W0[:, : cfg.nx]
    return P2, W2


def oracle_solve(cfg, P, W0, F, max_iter):
    from oracle import oracle_lib as O
    oc = O.make_config(cfg, max_iter=max_iter)
    return O.solve_batch_obs(oc, P, F, W0) if F is not None else O.solve_batch(oc, P, W0)


SCREEN_TOL = 1e-8      # two decades below the parity tolerance of 1e-6: what two fp64 summation orders may add to the oracle's own spread
SCREEN_DRAWS = 4


def screen(r):
    """The oracle against itself on a recipe's distinct instances under SCREEN_DRAWS draws of the rounding-level perturbation: (all converged,
    every instance holds its point to SCREEN_TOL and its iteration count on every draw, largest iteration count).  A recipe whose inputs fail
    this would let the oracle alone use the one-instance allowance of the parity check — an instance on which the oracle parts from itself by
    6e-7 (nine robots, seed 5) cannot be asked to meet another summation order within 1e-6 — so its seed is changed instead."""
    cfg, P, W0, F = inputs(r._replace(B=min(r.B, 16)))
    a = oracle_solve(cfg, P, W0, F, r.max_iter)
    conv, hold = bool((a["status"] == 0).all()), True
    for s in range(SCREEN_DRAWS):
        P2, W2 = perturbed(cfg, P, W0, seed=s)
        b = oracle_solve(cfg, P2, W2, F, r.max_iter)
        conv = conv and bool((b["status"] == 0).all())
        hold = hold and bool((np.max(np.abs(a["x"] - b["x"]), axis=1) <= SCREEN_TOL).all() and (a["iters"] == b["iters"]).all())
    return conv, hold, int(a["iters"].max())


# ---- long horizons on the HBM-resident kernel: bounded-iteration path comparison ----------------------------------------------------------
# Solves there take hundreds of iterations and fork late, so the path is compared, not the end: max_iter = K on both sides, status and
# iteration count equal, iterate and reported kkt within a tolerance measured on the reference side only.
# name: m, N (at least 1.5 x KERNEL1[m]), obstacles, heading flag, near (None: helpers.batch inputs), B, K, sample time (None: the script's),
# then the oracle's spread and the tolerance.  The spread is the largest deviation (path_deviation) of the oracle from itself under
# `perturbed`, four draws, after K iterations, measured on the CPU (path_spread); the tolerance is 100 x the spread — both sides are fp64 with
# different summation orders, two decades cover the reorderings without admitting a wrong term — at least 1e-12, never above 1e-6.
Path = namedtuple("Path", "m N K_obs thb near B max_iter T spread tol")
PATHS = {   # measured spread (rounded up)                                 -> tolerance
    "one_N1706": Path(1, 1706, 2, 0, None, 4, 5, None, 1.2e-12, 1.2e-10),      # K = 12: one instance ends with status 2 at iteration 11
    "two_N852": Path(2, 852, 0, 1, None, 4, 5, None, 4.0e-10, 4.0e-8),         # K = 12: spread 1.1e-5
    "three_N569": Path(3, 569, 2, 0, None, 4, 5, None, 5.3e-12, 5.3e-10),      # K = 12: spread 2.2e-5
    "four_N426": Path(4, 426, 0, 1, None, 4, 5, None, 2.4e-12, 2.4e-10),       # K = 12: spread 9.5e-8, tolerance above 1e-6
    "six_N284": Path(6, 284, 2, 1, None, 4, 12, None, 2.0e-10, 2.0e-8),
    "eight_N213": Path(8, 213, 0, 1, None, 4, 12, None, 9.4e-10, 9.4e-8),
    "ten_N170": Path(10, 170, 0, 1, None, 4, 12, None, 4.0e-9, 4.0e-7),
    # the ABI's longest horizon.  One robot: goals within 0.3 of the starts (with helpers.batch goals the oracle's spread is 0.35 after five
    # iterations); K = 5: spread 4.4e-12.  Ten robots: N = 4096 is also the longest horizon whose workspace for B = 2 stays under 1 GB (140 MB:
    # the ABI's limit on N comes first); goals within 0.02 of the starts (within 0.05 the spread is 4e-2 after five iterations); K = 12: 5.3e-8.
    "one_N4096": Path(1, 4096, 0, 0, 0.3, 2, 12, None, 3.3e-12, 3.3e-10),
    "ten_N4096": Path(10, 4096, 0, 0, 0.02, 2, 5, None, 2.1e-12, 2.1e-10),
}
for _p in PATHS.values():
    assert math.isclose(_p.tol, max(100.0 * _p.spread, 1e-12)) and _p.tol <= 1e-6 and _p.N >= 1.5 * KERNEL1[_p.m] and _p.max_iter <= 12


def path_inputs(p):
    d = _cfg(p.m, p.N, p.thb, p.K_obs, p.m % 2 == 0)
    if p.T is not None:
        d["T"] = p.T
    cfg = R.NLPConfig(**d)
    P, W0 = near_batch(cfg, p.B, 31, p.near) if p.near is not None else Hh.batch(cfg, p.B, 5)
    return cfg, P, W0


def path_deviation(a, b):
    """largest difference of the iterates, and of the reported kkt relative to max(1, kkt)"""
    return max(float(np.max(np.abs(a["x"] - b["x"]))), float(np.max(np.abs(a["kkt"] - b["kkt"]) / np.maximum(1.0, np.abs(b["kkt"])))))


def path_spread(p, draws=4):
    """(spread of the oracle against itself, whether status and iteration count held on every draw, statuses)"""
    cfg, P, W0 = path_inputs(p)
    a = oracle_solve(cfg, P, W0, None, p.max_iter)
    dev, held = 0.0, True
    for s in range(draws):
        P2, W2 = perturbed(cfg, P, W0, seed=s)
        b = oracle_solve(cfg, P2, W2, None, p.max_iter)
        held = held and bool((a["status"] == b["status"]).all() and (a["iters"] == b["iters"]).all())
        dev = max(dev, path_deviation(a, b))
    return dev, held, a["status"], a["iters"]
