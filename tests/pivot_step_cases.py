"""Inputs of tests/test_gpu_pivot_step.py: cold starts whose backward sweeps reject pivots, and what the oracle's own counters say about
where it rejects.

A pivot of the backward sweep is rejected where the control block of a stage is not positive definite, and what makes it indefinite is the
curvature of the pair rows (-2 z on the relative position of two robots) in the cost-to-go.  An instance here is a CLUSTER: every robot
stands dmin + gap away from an earlier one and no closer to the others, gap drawn from GAPS[kind], with headings and goals as
tests/helpers.instance draws them, and the reference's cold start X_k = x0, U = 0: every pair row of the cluster starts at its bound (the
solver pushes its slack to the bound push) at every stage 1 .. N - 1.

Where the oracle rejects is read from its counters (nmpc_oracle_stats: stage factorisations and rejected stages of the accepted sweeps since
the last reset).  A sweep that rejects at stages kf_1, kf_2, ... resumes each time at kr(kf) = NMPC_RESUME_STAGE(kf, N) >= kf, so it factors
N + sum_t (kr(kf_t) - kf_t + 1) stages.  For N <= 6 kr(kf) = N - 1 for every kf: a rejection at stage kf costs N - kf stages more, between
1 (stage N - 1) and N (stage 0), and `excess == N * rejections` says that EVERY rejection of those sweeps, the first included, was at stage 0.

Stage N - 1 cannot reject: its control block is B' P_N B + R + the control bounds' barrier terms, and P_N, the states of stage N, carries
the state bounds' barrier terms only (no cost and no pair row: the pair rows live on stages 1 .. N - 1), so the block is positive definite
whatever the start.  The highest stage that can reject is N - 2; first_sweep() finds none that rejects ONLY there at these sizes (the
excess would be 2 per rejection), the starts found reject at stage 0 or at several stages."""
import ctypes as C

import numpy as np

from oracle import nlp_ref as R
from oracle import oracle_lib as O
from tests import helpers as Hh
from tests import kernel_variants as KV

B = 64
POOL = 96                             # candidates drawn per case; the B kept are chosen on the oracle alone (select)
SCREEN_DRAWS = 12                     # of tests/kernel_variants.perturbed.  Its own 4 let through a cluster of three at N = 6 on which the oracle parts
                                      # from itself (iteration count) on 13 of 32 further draws: starts at the bound sit on rounding forks more often
MAX_ITER = 400
ITER_LIMIT = 100
GAPS = {"near": (0.005, 0.03), "tight": (0.0002, 0.002)}
KINDS = ("near", "tight")


def cfg_of(m, N):
    return R.NLPConfig(**KV._cfg(m, N, 0, 0, True))


def cluster(rng, cfg, kind):
    lo, hi = cfg.dmin + GAPS[kind][0], cfg.dmin + GAPS[kind][1]
    pts = [rng.uniform(-1.0, 1.0, 2)]
    while len(pts) < cfg.m:
        a, d = rng.uniform(-np.pi, np.pi), rng.uniform(lo, hi)
        c = pts[rng.integers(len(pts))] + d * np.array([np.cos(a), np.sin(a)])
        if all(np.hypot(*(c - q)) >= lo for q in pts):
            pts.append(c)
    return np.array(pts)


def candidates(m, N, n=POOL, seed=5):
    """n candidates, the kinds in turn: (config, P, W0)"""
    cfg = cfg_of(m, N)
    rng = np.random.Generator(np.random.PCG64(Hh.SEED0 + 7000 + 100 * m + N + 10000 * seed))
    P = []
    for i in range(n):
        s = cluster(rng, cfg, KINDS[i % len(KINDS)])
        g = Hh.sample_points(rng, cfg.m, cfg.dmin + 0.1)
        P.append(np.concatenate([np.concatenate([s, rng.uniform(-np.pi, np.pi, (cfg.m, 1))], axis=1).reshape(-1),
                                 np.concatenate([g, rng.uniform(-np.pi, np.pi, (cfg.m, 1))], axis=1).reshape(-1)]))
    P = np.stack(P)
    return cfg, P, np.stack([R.cold_start(cfg, p[: cfg.nx]) for p in P])


def counters(cfg, P, W0, max_iter):
    """per instance, over the accepted sweeps of a solve of at most max_iter iterations: (iterations counted, rejected stages, stages
    factored beyond N per iteration)"""
    L = O.lib()
    oc = O.make_config(cfg, max_iter=max_iter)
    out, st = [], (C.c_double * 4)()
    for p, w in zip(P, W0):
        L.nmpc_oracle_stats(st, 1)
        O.solve_batch(oc, p[None], w[None], nthreads=1)
        L.nmpc_oracle_stats(st, 1)
        out.append((int(st[1]), int(st[2]), int(st[0]) - int(st[3])))
    return np.array(out)


def first_sweep(cfg, P, W0):
    """per instance: (rejected stages, excess stages) of the first iteration's sweep"""
    return counters(cfg, P, W0, 1)[:, 1:]


def holds(cfg, P, W0, ref):
    """per instance: the oracle converges in under ITER_LIMIT iterations and holds its point (tests/kernel_variants.SCREEN_TOL) and its
    iteration count under SCREEN_DRAWS rounding-level perturbations (tests/kernel_variants.perturbed)"""
    ok = (ref["status"] == 0) & (ref["iters"] < ITER_LIMIT)
    for s in range(SCREEN_DRAWS):
        P2, W2 = KV.perturbed(cfg, P, W0, seed=s)
        b = KV.oracle_solve(cfg, P2, W2, None, MAX_ITER)
        ok &= (b["status"] == 0) & (b["iters"] == ref["iters"]) & (np.max(np.abs(b["x"] - ref["x"]), axis=1) <= KV.SCREEN_TOL)
    return ok


_CASES = {}


def select(m, N):
    """The B instances of a case, chosen from the pool on the oracle alone: those that pass holds(), the ones whose FIRST sweep rejects
    first, then in the order drawn.  Returns (config, P, W0, the oracle's solve, first_sweep of the kept, rejected stages of their whole
    solves); computed once per case and left unchanged."""
    if (m, N) not in _CASES:
        cfg, P, W0 = candidates(m, N)
        ref = KV.oracle_solve(cfg, P, W0, None, MAX_ITER)
        ok = holds(cfg, P, W0, ref)
        fs = first_sweep(cfg, P, W0)
        idx = np.flatnonzero(ok)
        idx = np.concatenate([idx[fs[idx, 0] > 0], idx[fs[idx, 0] == 0]])[:B]
        assert len(idx) == B, "the pool holds fewer than B screened instances"
        P, W0 = np.ascontiguousarray(P[idx]), np.ascontiguousarray(W0[idx])
        ref = {k: (v[idx].copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        whole = counters(cfg, P, W0, MAX_ITER)[:, 1]
        for v in [P, W0, whole] + [v for v in ref.values() if isinstance(v, np.ndarray)]:
            v.setflags(write=False)
        _CASES[(m, N)] = (cfg, P, W0, ref, fs[idx], whole)
    return _CASES[(m, N)]
