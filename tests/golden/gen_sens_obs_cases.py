"""Generator of tests/golden/sens_obs_cases.npz: converged instances on which the obstacle map S_o of include/nmpc.h (nmpc_sens_adjoint_batch)
predicts the oracle's own re-solves under a moved obstacle field to first order.

Per configuration (tests/sens_adjoint_ref.obs_case_configs): starts and goals as in tests/golden/gen_sens_cases.py with an obstacle just beyond the
goal of each of the first K robots, so that the goal lies inside its clearance and the plan ends pressed against it; a unit direction d in the
field's own shape ([K, 3] static, [N, K, 3] moving: centres and radii move), and the CPU oracle's w*(obs), w*(obs + h d), w*(obs + h/2 d),
h = sens_adjoint_ref.H_OBS, the two re-solves warm-started at w*(obs).  The multipliers are the
least-squares multipliers of w*(obs) on its active set (tests/duals_ref.lsq_multipliers); the reference is tests/sens_adjoint_ref.  The screen and
the acceptance rule are those of gen_sens_cases.py.  A candidate is kept only if
  - the oracle converged at all three points and an obstacle row of stages 1..N-1 is active (S_o d is zero otherwise),
  - the reference's info is 0 and every F_uu has its smallest eigenvalue >= 1e-6,
  - the prediction-error ratio |w + h S_o d - w*(obs + h d)| / |w + h/2 S_o d - w*(obs + h/2 d)| lies in [3.8, 4.2] (elsewhere the re-solve
    changed its active set),
  - the reference's adjoint recursion agrees with its dense solve within 100 x its own spread + 1e-12 for the cotangent of the tests.
The first KEEP kept ones are stored; the generator fails on a configuration that keeps fewer.

    python tests/golden/gen_sens_obs_cases.py      -> tests/golden/sens_obs_cases.npz, one line per candidate on stdout
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CANDIDATES, KEEP = 40, 4
SEED = 20261020


def _sens_generator():
    spec = importlib.util.spec_from_file_location("gen_sens_cases", os.path.join(HERE, "gen_sens_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def candidate(rng, cfg, kind):
    """(p, obs): starts apart by more than dmin, goals within reach of the horizon, obstacle q up to 1.2 rad off the line of travel of robot q,
    its clearance circle 1 .. 8 cm over the goal and clear of every start"""
    from tests import helpers as Hh
    m, K, reach = cfg.m, cfg.K, min(cfg.v_max * cfg.T * cfg.N, 0.3)
    while True:
        s = Hh.sample_points(rng, m, cfg.dmin + 0.02, lim=0.6 * (cfg.dmin + 0.1) * m ** 0.5)
        th = rng.uniform(-np.pi, np.pi, m)
        ang = th + rng.uniform(-0.6, 0.6, m)
        dist = rng.uniform(0.4, 0.9, m) * reach
        g = s + dist[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        gth = th + rng.uniform(-0.5, 0.5, m)
        rad = rng.uniform(0.1, 0.15, K)
        off = ang[:K] + rng.uniform(-1.2, 1.2, K)
        c0 = g[:K] + np.stack([np.cos(off), np.sin(off)], axis=1) * (cfg.rob_dim + cfg.margin + rad - rng.uniform(0.01, 0.08, K))[:, None]
        if (np.linalg.norm(s[:, None] - c0[None], axis=2) >= cfg.rob_dim + cfg.margin + rad[None] + 0.03).all():
            break
    p = np.concatenate([np.concatenate([s, th[:, None]], axis=1).reshape(-1), np.concatenate([g, gth[:, None]], axis=1).reshape(-1)])
    if kind == "static":
        return p, np.concatenate([c0, rad[:, None]], axis=1)
    vel = rng.uniform(-0.3, 0.3, (K, 2)) * cfg.v_max
    k = np.arange(cfg.N)[:, None, None]
    return p, np.concatenate([c0[None] + k * cfg.T * vel[None], np.broadcast_to(rad[None, :, None] * (1.0 + 0.02 * k), (cfg.N, K, 1))], axis=2)


def main():
    from oracle import nlp_ref as R, oracle_lib as O
    from tests import duals_ref as D, sens_ref as S, sens_adjoint_ref as AR
    gen = _sens_generator()
    O.build()
    H = AR.H_OBS
    out, total = {"h": np.array(H), "names": np.array(list(AR.obs_case_configs()))}, 0
    for index, (name, (cfg, kind)) in enumerate(AR.obs_case_configs().items()):
        rng = np.random.default_rng(SEED + index)
        oc = O.make_config(cfg, max_iter=2000)
        kept = {k: [] for k in ("p", "obs", "d", "w", "w_h", "w_h2", "lam_g", "lam_x")}
        for c in range(CANDIDATES):
            p, obs = candidate(rng, cfg, kind)
            d = rng.normal(size=obs.shape); d /= np.linalg.norm(d)
            w, st0 = gen.solve(oc, p, R.cold_start(cfg, p[: cfg.nx]), obs)
            w1, st1 = gen.solve(oc, p, w, obs + H * d)
            w2, st2 = gen.solve(oc, p, w, obs + 0.5 * H * d)
            line = "%-12s %d: status %d %d %d" % (name, c, st0, st1, st2)
            ok = st0 == 0 and st1 == 0 and st2 == 0
            if ok:
                lam_g, lam_x, act = D.lsq_multipliers(cfg, w, p, tol_active=1e-6, obs=obs)
                rows = np.array([AR.MO.obstacle_row(cfg, k, i, q) for k in range(1, cfg.N) for i in range(cfg.m) for q in range(cfg.K)])
                nact = int((lam_g[rows] < 0).sum())
                r = S.stage_recursion(cfg, p, w, lam_g, lam_x, obs)
                line += ", info %d, min eig F_uu %.2e, active obstacle rows %d" % (r["info"], r["min_eig"], nact)
                ok = r["info"] == 0 and r["min_eig"] >= 1e-6 and nact >= 1
                if ok:
                    dw = AR.obs_prediction(cfg, p, w, lam_g, lam_x, obs, d)
                    e1, e2, ratio = S.prediction_errors(w, dw, w1, w2, H)
                    line += ", |w(obs+hd) - w| %.2e, errors %.2e %.2e ratio %.3f" % (float(np.abs(w - w1).max()), e1, e2, ratio)
                    ok = 3.8 <= ratio <= 4.2
                if ok:
                    wbar = AR.cotangent(cfg, SEED)
                    a = AR.stage_adjoint(cfg, p, w, lam_g, lam_x, obs, wbar)
                    pb, ob = AR.dense_reference(cfg, p, w, lam_g, lam_x, obs, wbar)
                    sp, so = AR.spread(cfg, p, w, lam_g, lam_x, obs, wbar)
                    ep, eo = AR.rel(a["pbar"], pb), AR.rel(a["obsbar"], ob)
                    line += ", recursion against dense %.1e (spread %.1e) %.1e (%.1e)" % (ep, sp, eo, so)
                    ok = ep <= 100.0 * sp + 1e-12 and eo <= 100.0 * so + 1e-12
            print(line + (" kept" if ok else " dropped"), flush=True)
            if ok:
                for k, v in (("p", p), ("obs", obs), ("d", d), ("w", w), ("w_h", w1), ("w_h2", w2), ("lam_g", lam_g), ("lam_x", lam_x)):
                    kept[k].append(v)
                if len(kept["p"]) == KEEP:
                    break
        if len(kept["p"]) < KEEP:
            raise SystemExit("%s: only %d of %d candidates pass the screen" % (name, len(kept["p"]), CANDIDATES))
        total += KEEP
        for k, v in kept.items():
            out[name + "/" + k] = np.array(v)
    path = os.path.join(ROOT, "tests", "golden", "sens_obs_cases.npz")
    np.savez_compressed(path, **out)
    print("kept %d instances -> %s, %d bytes" % (total, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
