"""Generator of tests/golden/sens_update_cases.npz: converged instances on which the forward plan update of include/nmpc.h (nmpc_sens_update_batch),
dw = S_p dp + S_o dobs, predicts the oracle's own re-solves under a SIMULTANEOUS move of the measured state and of the obstacle field to first
order, with nothing limiting the step.

Per configuration (tests/sens_adjoint_ref.obs_case_configs): the candidates of tests/golden/gen_sens_obs_cases.py (an obstacle just beyond the goal
of each of the first K robots, so that the plan ends pressed against it), a unit direction dx of the state and a unit direction d in the field's
own shape, and the CPU oracle's (oracle_lib.solve_batch_obs) w*(x0, obs), w*(x0 + h dx, obs + h d), the same at h / 2, h = sens_update_ref.H_UPD,
the two re-solves warm-started at the first.  The multipliers are the least-squares multipliers of the first point on its active set
(tests/duals_ref.lsq_multipliers); the reference is tests/sens_update_ref.  The screen is that of gen_sens_obs_cases.py plus the step's own
(sens_update_ref.screen).  A candidate is kept only if
  - the oracle converged at all three points and an obstacle row of stages 1..N-1 is active,
  - the reference's info is 0 and every F_uu has its smallest eigenvalue >= 1e-6,
  - the prediction-error ratio |w + h dw - w*(h)| / |w + h/2 dw - w*(h/2)| lies in [3.8, 4.2],
  - alpha of the step h (dw, d) is exactly 1 on the reference,
  - |U_0 + h dU_0 - U_0(h)| < |U_0 - U_0(h)|: the corrected first control is closer to the re-solve's than the prepared one,
  - the reference's recursion agrees with its dense solve within 100 x its own spread + 1e-12.
The first KEEP kept ones are stored; the generator fails on a configuration that keeps fewer.

    python tests/golden/gen_sens_update_cases.py      -> tests/golden/sens_update_cases.npz, one line per candidate on stdout
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CANDIDATES, KEEP = 40, 4
SEED = 20261021


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from oracle import nlp_ref as R, oracle_lib as O
    from tests import duals_ref as D, sens_adjoint_ref as AR, sens_update_ref as UR
    gen, gen_obs = _module("gen_sens_cases"), _module("gen_sens_obs_cases")
    O.build()
    H = UR.H_UPD
    out, total = {"h": np.array(H), "names": np.array(list(AR.obs_case_configs()))}, 0
    for index, (name, (cfg, kind)) in enumerate(AR.obs_case_configs().items()):
        rng = np.random.default_rng(SEED + index)
        oc = O.make_config(cfg, max_iter=2000)
        kept = {k: [] for k in ("p", "obs", "dx", "d", "w", "w_h", "w_h2", "lam_g", "lam_x")}
        for c in range(CANDIDATES):
            p, obs = gen_obs.candidate(rng, cfg, kind)
            d = rng.normal(size=obs.shape); d /= np.linalg.norm(d)
            dx = rng.normal(size=cfg.nx); dx /= np.linalg.norm(dx)
            moved = lambda s: np.concatenate([p[: cfg.nx] + s * dx, p[cfg.nx:]])
            w, st0 = gen.solve(oc, p, R.cold_start(cfg, p[: cfg.nx]), obs)
            w1, st1 = gen.solve(oc, moved(H), w, obs + H * d)
            w2, st2 = gen.solve(oc, moved(0.5 * H), w, obs + 0.5 * H * d)
            line = "%-12s %d: status %d %d %d" % (name, c, st0, st1, st2)
            ok = st0 == 0 and st1 == 0 and st2 == 0
            if ok:
                lam_g, lam_x, act = D.lsq_multipliers(cfg, w, p, tol_active=1e-6, obs=obs)
                rows = np.array([AR.MO.obstacle_row(cfg, k, i, q) for k in range(1, cfg.N) for i in range(cfg.m) for q in range(cfg.K)])
                nact = int((lam_g[rows] < 0).sum())
                s = UR.screen(cfg, p, w, lam_g, lam_x, obs, dx, d, w1, w2, H)
                line += ", info %d, min eig F_uu %.2e, active obstacle rows %d, errors %.2e %.2e ratio %.3f, alpha(h) %.6f, |U_0| error %.2e against %.2e" % (
                    s["info"], s["min_eig"], nact, s["e1"], s["e2"], s["ratio"], s["alpha_h"], s["e_u"], s["e_u0"])
                ok = s["ok"] and nact >= 1
                if ok:
                    dp = UR.case_dp(cfg, dx)
                    a = UR.stage_update(cfg, p, w, lam_g, lam_x, obs, dp=dp, dobs=d)
                    dd = UR.dense_update(cfg, p, w, lam_g, lam_x, obs, dp=dp, dobs=d)
                    sw, _ = UR.spread(cfg, p, w, lam_g, lam_x, obs, dp=dp, dobs=d)
                    e = UR.rel(a["dw"], dd)
                    line += ", recursion against dense %.1e (spread %.1e)" % (e, sw)
                    ok = e <= 100.0 * sw + 1e-12
            print(line + (" kept" if ok else " dropped"), flush=True)
            if ok:
                for k, v in (("p", p), ("obs", obs), ("dx", dx), ("d", d), ("w", w), ("w_h", w1), ("w_h2", w2), ("lam_g", lam_g), ("lam_x", lam_x)):
                    kept[k].append(v)
                if len(kept["p"]) == KEEP:
                    break
        if len(kept["p"]) < KEEP:
            raise SystemExit("%s: only %d of %d candidates pass the screen" % (name, len(kept["p"]), CANDIDATES))
        total += KEEP
        for k, v in kept.items():
            out[name + "/" + k] = np.array(v)
    path = os.path.join(ROOT, "tests", "golden", "sens_update_cases.npz")
    np.savez_compressed(path, **out)
    print("kept %d instances -> %s, %d bytes" % (total, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
