"""Generator of tests/golden/sens_cases.npz: converged instances on which the plan sensitivity of include/nmpc.h (nmpc_sens_batch) predicts the
oracle's own re-solves to first order.

Per configuration (tests/sens_ref.case_configs): candidates p = [x0; xs] with goals within a few horizons' reach (so that not every control sits on its
bound), a unit direction d in parameter space, and the CPU oracle's w*(p), w*(p + h d), w*(p + h/2 d), h = 1e-2, the two re-solves warm-started
at w*(p).  The multipliers are the least-squares multipliers of w*(p) on its active set (tests/duals_ref.lsq_multipliers); the reference is
tests/sens_ref.  A candidate is kept only if
  - the oracle converged at all three points,
  - the reference's info is 0 and every F_uu has its smallest eigenvalue >= 1e-6,
  - the reference's prediction-error ratio |w + h dw - w*(p + h d)| / |w + h/2 dw - w*(p + h/2 d)| lies in [3.8, 4.2],
  - the reference's stage recursion agrees with its dense solve within 100 x its own spread + 1e-12 (tests/sens_ref.recursion_against_dense):
    the bound of the tests; where the subtraction P = F_xx - F_xu F_uu^-1 F_ux cancels a Sigma of 1e7 against itself, rounding can exceed what
    the spread of the inputs shows, and the fixture is of no use as a yardstick
(elsewhere the re-solve changed its active set or its local minimum: the NLP has no derivative there, or the oracle left it).  The generator
fails if it keeps fewer than half of a configuration's candidates; the first KEEP kept ones are stored.

    python tests/golden/gen_sens_cases.py      -> tests/golden/sens_cases.npz, one line per candidate on stdout
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H = 1e-2
CANDIDATES, KEEP = 8, 4
SEED = 20261019


def configs():
    """name -> (oracle NLPConfig, obstacle field kind): the table the tests read the fixture by"""
    from tests import sens_ref as S
    return S.case_configs()


def candidate(rng, cfg, kind, name):
    """(p, d, obs): starts apart by more than dmin, goals within reach of the horizon, a unit direction, the instance's obstacle field"""
    from tests import helpers as Hh
    m, reach = cfg.m, min(cfg.v_max * cfg.T * cfg.N, 0.3)      # long horizons: goals well inside the reach, the plan slows down into them
    s = Hh.sample_points(rng, m, cfg.dmin + 0.02, lim=0.6 * (cfg.dmin + 0.1) * m ** 0.5)
    th = rng.uniform(-np.pi, np.pi, m)
    if m > 1 and rng.uniform() < 0.5:      # the team closes in on its centroid: pair rows become active
        to = s.mean(axis=0)[None] - s
        th = np.arctan2(to[:, 1], to[:, 0]) + rng.uniform(-0.3, 0.3, m)
    ang = th + rng.uniform(-0.6, 0.6, m)
    dist = rng.uniform(0.2, 0.9, m) * reach
    g = s + dist[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    gth = th + rng.uniform(-0.5, 0.5, m)
    if name == "heading1":      # the heading runs into its upper bound on the way to a goal heading beyond it
        th = np.array([cfg.th_max - rng.uniform(0.02, 0.1)]); gth = np.array([cfg.th_max + 0.4])
        g = s + dist[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
    p = np.concatenate([np.concatenate([s, th[:, None]], axis=1).reshape(-1), np.concatenate([g, gth[:, None]], axis=1).reshape(-1)])
    d = rng.normal(size=p.size); d /= np.linalg.norm(d)
    obs = None
    if kind is not None:      # obstacles beside the first robots' goals, close enough to bend the paths, clear of every start
        K = cfg.K
        nrm = np.stack([-np.sin(ang[:K]), np.cos(ang[:K])], axis=1)
        for tries in range(200):
            rad = rng.uniform(0.1, 0.15, K)
            c0 = g[:K] + nrm * (rng.choice([-1.0, 1.0], K) * (cfg.rob_dim + cfg.margin + rad + rng.uniform(-0.05, 0.08, K)))[:, None]
            if (np.linalg.norm(s[:, None] - c0[None], axis=2) >= cfg.rob_dim + cfg.margin + rad[None] + 0.03).all():
                break
        else:
            return candidate(rng, cfg, kind, name)      # no clear placement beside these goals: another draw
        if kind == "static":
            obs = np.concatenate([c0, rad[:, None]], axis=1)
        else:
            vel = rng.uniform(-0.3, 0.3, (K, 2)) * cfg.v_max
            k = np.arange(cfg.N)[:, None, None]
            obs = np.concatenate([c0[None] + k * cfg.T * vel[None], np.broadcast_to(rad[None, :, None] * (1.0 + 0.02 * k), (cfg.N, K, 1))], axis=2)
    return p, d, obs


def solve(oc, p, w0, obs):
    from oracle import oracle_lib as O
    r = O.solve_batch(oc, p[None], w0[None]) if obs is None else O.solve_batch_obs(oc, p[None], obs[None], w0[None])
    return r["x"][0], int(r["status"][0])


def main():
    from oracle import nlp_ref as R, oracle_lib as O
    from tests import duals_ref as D, sens_ref as S
    O.build()
    out, kept_all, cand_all = {"h": np.array(H), "names": np.array(list(configs()))}, 0, 0
    for index, (name, (cfg, kind)) in enumerate(configs().items()):
        rng = np.random.default_rng(SEED + index)      # a stream per configuration: one does not move the others
        oc = O.make_config(cfg, max_iter=2000)
        kept = {k: [] for k in ("p", "d", "obs", "w", "w_h", "w_h2", "lam_g", "lam_x")}
        passed = 0
        for c in range(CANDIDATES):
            p, d, obs = candidate(rng, cfg, kind, name)
            w, st0 = solve(oc, p, R.cold_start(cfg, p[: cfg.nx]), obs)
            w1, st1 = solve(oc, p + H * d, w, obs)
            w2, st2 = solve(oc, p + 0.5 * H * d, w, obs)
            line = "%-12s %d: status %d %d %d" % (name, c, st0, st1, st2)
            ok = st0 == 0 and st1 == 0 and st2 == 0
            if ok:
                lam_g, lam_x, act = D.lsq_multipliers(cfg, w, p, tol_active=1e-6, obs=obs)
                r = S.stage_recursion(cfg, p, w, lam_g, lam_x, obs, dp=d)
                e1, e2, ratio = S.prediction_errors(w, r["dw"], w1, w2, H)
                e0 = float(np.abs(w - w1).max())
                line += ", info %d, min eig F_uu %.2e, active rows %d bounds %d, |w(p+hd) - w| %.2e, errors %.2e %.2e ratio %.3f" % (
                    r["info"], r["min_eig"], act.size, int(np.count_nonzero(lam_x[cfg.nx:])), e0, e1, e2, ratio)
                ok = r["info"] == 0 and r["min_eig"] >= 1e-6 and 3.8 <= ratio <= 4.2
                if ok:
                    eg, sg, ew, sw = S.recursion_against_dense(cfg, p, w, lam_g, lam_x, obs, d)
                    line += ", recursion against dense %.1e (spread %.1e) %.1e (%.1e)" % (eg, sg, ew, sw)
                    ok = eg <= 100.0 * sg + 1e-12 and ew <= 100.0 * sw + 1e-12
            print(line + (" kept" if ok and passed < KEEP else " passed" if ok else " dropped"), flush=True)
            if ok:
                if passed < KEEP:
                    for k, v in (("p", p), ("d", d), ("obs", obs), ("w", w), ("w_h", w1), ("w_h2", w2), ("lam_g", lam_g), ("lam_x", lam_x)):
                        if v is not None:
                            kept[k].append(v)
                passed += 1
        kept_all += passed; cand_all += CANDIDATES
        if 2 * passed < CANDIDATES or passed < KEEP:
            raise SystemExit("%s: only %d of %d candidates pass the screen" % (name, passed, CANDIDATES))
        for k, v in kept.items():
            if v:
                out[name + "/" + k] = np.array(v)
    path = os.path.join(ROOT, "tests", "golden", "sens_cases.npz")
    np.savez_compressed(path, **out)
    print("kept %d of %d candidates -> %s, %d bytes" % (kept_all, cand_all, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
