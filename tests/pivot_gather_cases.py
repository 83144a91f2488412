"""Inputs of tests/test_gpu_pivot_gather.py: the clusters of tests/pivot_step_cases.py (cold starts whose backward sweeps reject pivots) for
every team size of the row-paired sweep, with and without the heading bound, at N = 6 and N = 11: the sweep saves the cost-to-go entering
one stage, and two (NMPC_CKPT_EVERY = 5), so a resumed sweep restarts from a saved cost-to-go with no earlier pivot row in flight.

The B instances of a case are chosen on the oracle alone, as pivot_step_cases.select does: those on which it converges and holds its point
and its iteration count under rounding-level perturbations (pivot_step_cases.holds, the screen of tests/kernel_variants.py with more
draws), the ones whose first sweep rejects a pivot first."""
import numpy as np

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import pivot_step_cases as PC

B = 16
POOL = 40
TEAMS = (2, 3, 4, 5, 6)
HORIZONS = (6, 11)


def candidates(m, N, thb, n=POOL):
    cfg = R.NLPConfig(**KV._cfg(m, N, thb, 0, True))
    rng = np.random.Generator(np.random.PCG64(Hh.SEED0 + 91000 + 1000 * m + 10 * N + thb))
    P = []
    for i in range(n):
        s = PC.cluster(rng, cfg, PC.KINDS[i % len(PC.KINDS)])
        g = Hh.sample_points(rng, cfg.m, cfg.dmin + 0.1)
        P.append(np.concatenate([np.concatenate([s, rng.uniform(-np.pi, np.pi, (cfg.m, 1))], axis=1).reshape(-1),
                                 np.concatenate([g, rng.uniform(-np.pi, np.pi, (cfg.m, 1))], axis=1).reshape(-1)]))
    P = np.stack(P)
    return cfg, P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P])


_CASES = {}


def select(m, N, thb):
    """(config, P, W0, the oracle's solve, rejected stages of the first sweeps, of the whole solves); computed once per case, read-only"""
    if (m, N, thb) not in _CASES:
        cfg, P, W0 = candidates(m, N, thb)
        ref = KV.oracle_solve(cfg, P, W0, None, PC.MAX_ITER)
        ok = PC.holds(cfg, P, W0, ref)
        fs = PC.first_sweep(cfg, P, W0)
        idx = np.flatnonzero(ok)
        idx = np.concatenate([idx[fs[idx, 0] > 0], idx[fs[idx, 0] == 0]])[:B]
        assert len(idx) == B, "the pool holds %d screened instances, fewer than B" % len(idx)
        P, W0 = np.ascontiguousarray(P[idx]), np.ascontiguousarray(W0[idx])
        ref = {k: (v[idx].copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        whole = PC.counters(cfg, P, W0, PC.MAX_ITER)[:, 1]
        for v in [P, W0, whole] + [v for v in ref.values() if isinstance(v, np.ndarray)]:
            v.setflags(write=False)
        _CASES[(m, N, thb)] = (cfg, P, W0, ref, fs[idx, 0], whole)
    return _CASES[(m, N, thb)]
