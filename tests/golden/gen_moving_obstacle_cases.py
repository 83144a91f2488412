"""Generator of tests/golden/moving_obstacle_cases.npz: the rescue paths of the solver met with MOVING obstacles.

A CPU closed-loop soak of the six-robot composite (N = 25) among eight obstacles of their own per swarm, crossing the workspace at constant
velocity with growing radii (tests/moving_obstacles_ref.moving_batch, paths of max_steps + N rows): 256 swarms x 40 periods for each of the
seeds 31 and 7, driven by the
shipping oracle through nmpc_oracle_solve_batch_obs, the solve of period t seeing rows t .. t+N-1 of its swarm's paths.  Captured per solve
(p, the warm-started guess and the [N, K, 3] field window), once per swarm (its first; its later failures follow from it):
  kind 0  converged by the shipping oracle, not without the cold-start retry (NMPC_ORACLE_NO_COLD_RETRY=1);
  kind 1  not converged with ONE retry only (NMPC_ORACLE_MAX_COLD=1): the elastic phase is what the shipping oracle reaches;
  kind 2  status 4 (stalled) with the shipping oracle.
Status 3 (infeasible x0) is the consequence of an earlier failure and is not captured.  Inputs only; the GPU test asserts the oracle's status
on every kernel.  Every solve runs without the retry first; only those that fail or reach the retry's watchdog there (the only solves where
the three settings can differ) are solved again with the other two."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, STEPS = 256, 40
SEEDS = (31, 7)      # seed 31 holds no solve that needs the elastic phase, seed 7 one


def composite_moving(N=25):
    from oracle import nlp_ref as R
    c = R.cfg_six(N); c.obstacles = [(0.0, 0.0, 0.1)] * 8; c.rob_dim = 0.2; c.margin = 0.1
    return c


def _solve(oc, P, F, W, env):
    from oracle import oracle_lib as O
    old = {k: os.environ.pop(k, None) for k in ("NMPC_ORACLE_NO_COLD_RETRY", "NMPC_ORACLE_MAX_COLD")}
    os.environ.update(env)
    try:
        return O.solve_batch_obs(oc, P, F, W)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


def soak(seed):
    from oracle import oracle_lib as O
    from tests import moving_obstacles_ref as MO
    c = composite_moving()
    oc = O.make_config(c, max_iter=2000)
    P, W, paths = MO.moving_batch(c, B, seed, L=STEPS + c.N)
    P = P.copy()
    cases = {"p": [], "w": [], "obs": [], "kind": [], "seed": [], "period": [], "swarm": []}
    counts = np.zeros(3, dtype=int)
    seen = set()
    for t in range(STEPS):
        F = np.ascontiguousarray(paths[:, t:t + c.N])
        r = _solve(oc, P, F, W, {"NMPC_ORACLE_NO_COLD_RETRY": "1"})
        sub = np.flatnonzero((r["status"] != 0) | (r["iters"] >= 500))
        sub = sub[r["status"][sub] != 3]
        if sub.size:
            d = _solve(oc, P[sub], F[sub], W[sub], {})
            one = _solve(oc, P[sub], F[sub], W[sub], {"NMPC_ORACLE_MAX_COLD": "1"})
            for j, b in enumerate(sub):
                kind = 2 if d["status"][j] == 4 else (1 if one["status"][j] != 0 else (0 if d["status"][j] == 0 and r["status"][b] != 0 else -1))
                if kind >= 0 and b not in seen:      # a swarm's first capture: its later failures follow from this one
                    seen.add(b)
                    for k, v in (("p", P[b]), ("w", W[b]), ("obs", F[b]), ("kind", kind), ("seed", seed), ("period", t), ("swarm", b)):
                        cases[k].append(np.copy(v))
                    counts[kind] += 1
                for k in ("x", "status", "iters"):
                    r[k][b] = d[k][j]
        W, x0n = O.shift_batch(oc, P, r["x"])
        P[:, : c.nx] = x0n
        print(f"seed {seed} period {t}: status {dict(zip(*np.unique(r['status'], return_counts=True)))}, captured so far {counts.tolist()}", flush=True)
    return cases, counts


if __name__ == "__main__":
    seeds = [int(a) for a in sys.argv[1:]] or SEEDS
    cases, counts = {}, np.zeros(3, dtype=int)
    for sd in seeds:
        c, n = soak(sd)
        for k, v in c.items():
            cases.setdefault(k, []).extend(v)
        counts += n
    out = os.path.join(ROOT, "tests", "golden", "moving_obstacle_cases.npz")
    np.savez_compressed(out, **{k: np.array(v) for k, v in cases.items()})
    print("captured (rescued by the cold retry, elastic phase, status 4):", counts.tolist(), "->", out, os.path.getsize(out), "bytes")
