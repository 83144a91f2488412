"""GPU: the per-instance obstacle field (nmpc_solve_batch_obs, nmpc_step_batch_obs, nmpc_eval_batch_obs, simulate_closed_loop(obstacle_paths=))
against the CPU oracle given the same field (oracle_lib.solve_batch_obs / eval_batch_obs), as the plain calls are checked against the plain
oracle: every team size 1..10, the throughput shape (kernel 3, with its small-team layouts), the latency shapes (kernel 4; 5 for five and six
robots) and the library's own choice, moving and growing fields (tests/moving_obstacles_ref.moving_batch), closed loops whose solves see a
moving window of per-swarm paths, and the rescue paths (cold retry, elastic phase, stall) captured with moving obstacles."""
import functools
import os

import numpy as np
import pytest

from oracle import nlp_ref as R, oracle_lib as O
from tests import helpers as Hh
from tests import moving_obstacles_ref as MO

pytestmark = pytest.mark.gpu

FIELDS = ("x", "f", "status", "iters", "kkt")


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items() if k in FIELDS}


def _solver(ocfg, B, kernel=None, max_iter=2000):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(ocfg, max_iter=max_iter), max_batch=B, kernel=kernel)


# name: (m, N, K, config keywords, B, seed).  m = 1 with the heading bound (third scenario, 2 pi); m = 2, 3: the small-team layouts of the
# throughput shape; m = 5, 6 with the composite's eight obstacles (the only team sizes with a four-wavefront shape); m = 8, 10: the largest
# workspace layouts, small batches (the oracle needs ~0.1 s per ten-robot solve)
CELLS = {
    "m1": (1, 100, 6, dict(th_max=2 * np.pi), 64, 1),
    "m2": (2, 20, 3, {}, 128, 2),
    "m3": (3, 10, 2, {}, 128, 3),
    "m4": (4, 20, 4, {}, 96, 4),
    "m5": (5, 25, 8, {}, 64, 5),
    "m6": (6, 25, 8, {}, 128, 6),
    "m8": (8, 20, 4, {}, 16, 8),
    "m10": (10, 20, 4, {}, 16, 10),
}
# identical iteration counts, measured on one MI355X: 1.000 in every cell and shape but m6 (127 of 128) and m1 (61 of 64 on every kernel, the
# same point on all 64; with the field's entry 0 held for every stage 62 of 64 — a long-horizon trait, not one of the moving field)
ITERS_FRAC = {"m1": 0.93}


@functools.lru_cache(maxsize=None)
def _cell(name):
    """(cfg, P, W0, F, oracle result) of a cell: cold starts among per-instance moving, growing fields [B, N, K, 3]"""
    m, N, K, kw, B, seed = CELLS[name]
    cfg = MO.team_cfg(m, N, K, **kw)
    P, W0, F = MO.moving_batch(cfg, B, 500 + seed)
    ref = O.solve_batch_obs(O.make_config(cfg, max_iter=2000), P, F, W0)
    return cfg, P, W0, F, ref


def check_parity(cfg, P, r, ref, what="", cell=None):
    """The oracle parity of test_full_size_bench_batches_match_oracle for a field solve: status equal on every instance, identical iteration
    counts on >= 97 %, the same point (1e-6) on >= 99 % (all but one below B = 100), the objective within 1e-6 relative where the point is
    the same, kkt <= 1e-8 on status 0, x0 pinned and the bounds held.  Returns (same-point fraction, identical-iteration fraction)."""
    B = P.shape[0]
    assert (r["status"] == ref["status"]).all(), (what, np.flatnonzero(r["status"] != ref["status"]), r["status"], ref["status"])
    ok = r["status"] == 0
    same = np.max(np.abs(r["x"] - ref["x"]), axis=1) <= 1e-6
    iters = r["iters"] == ref["iters"]
    print(f"{what}: B={B}, status 0 {ok.mean():.4f}, same point {same.mean():.4f}, identical iteration counts {iters.mean():.4f}, "
          f"mean iterations {r['iters'].mean():.2f} (oracle {ref['iters'].mean():.2f})")
    assert same.sum() >= (B - 1 if B < 100 else 0.99 * B), (what, np.flatnonzero(~same))
    assert iters.mean() >= ITERS_FRAC.get(cell, 0.97), (what, np.flatnonzero(~iters))
    rel = np.abs(r["f"] - ref["f"]) / np.maximum(1.0, np.abs(ref["f"]))
    assert (rel[same & ok] <= 1e-6).all(), what
    assert (r["kkt"][ok] <= 1e-8).all(), what
    assert np.array_equal(r["x"][:, : cfg.nx], P[:, : cfg.nx]), what
    lbx, ubx, _, _ = R.bounds(cfg)
    assert (r["x"] >= lbx - 1e-12).all() and (r["x"] <= ubx + 1e-12).all(), what
    return same.mean(), iters.mean()


PARITY = [(n, k) for n in CELLS for k in (None, 3, 4)] + [("m5", 5), ("m6", 5)]


@pytest.mark.parametrize("name,kernel", PARITY, ids=["%s-k%s" % (n, k) for n, k in PARITY])
def test_moving_field_solves_match_oracle(built, name, kernel):
    """Moving, growing fields, every team size, every column-kernel shape: the parity of check_parity against the oracle given the same
    fields.  The oracle solves each cell once for its kernels.  Measured on one MI355X: status 0 everywhere; the same point on every
    instance but one of m6 (127 of 128, every kernel); identical iteration counts on every instance of m2-m5, m8, m10, 127 of 128 of m6
    and 61 of 64 of m1 (100-stage solves, every kernel: ITERS_FRAC)."""
    import torch
    cfg, P, W0, F, ref = _cell(name)
    s = _solver(cfg, P.shape[0], kernel=kernel)
    r = _np(s.solve_batch(P, W0, obstacles=F)); torch.cuda.synchronize()
    assert (ref["status"] == 0).mean() >= 0.95, ref["status"]
    check_parity(cfg, P, r, ref, f"{name} kernel {kernel} (launches {s.kernel_for_batch(P.shape[0]) if kernel is None else kernel})", name)


def _field(seed, K=8):
    rng = np.random.default_rng(seed)
    return [(float(x), float(y), float(r)) for x, y, r in zip(rng.uniform(-1.5, 1.5, K), rng.uniform(-1.5, 1.5, K), rng.uniform(0.125, 0.2, K))]


def test_heterogeneous_static_fields_match_oracle(built):
    """256 composite instances, each with a static field of its own (S = 1, starts and goals clear of it), against solve_batch_obs with the
    same fields on kernels None, 3 and 4 (the per-field-handle comparison is test_gpu_obstacle_params.py's)."""
    import torch
    B = 256
    base = R.cfg_six(25); base.obstacles = _field(7); base.rob_dim = 0.2; base.margin = 0.1
    rng = np.random.default_rng(21)
    fld = np.stack([np.array(_field(3000 + b)) for b in range(B)])
    P = []
    for b in range(B):
        c = R.cfg_six(25); c.obstacles = list(map(tuple, fld[b])); c.rob_dim = 0.2; c.margin = 0.1
        P.append(Hh.instance(rng, c))
    P = np.stack(P)
    W0 = np.stack([R.cold_start(base, p[: base.nx]) for p in P])
    ref = O.solve_batch_obs(O.make_config(base, max_iter=2000), P, fld, W0)
    for kernel in (None, 3, 4):
        r = _np(_solver(base, B, kernel=kernel).solve_batch(P, W0, obstacles=fld)); torch.cuda.synchronize()
        check_parity(base, P, r, ref, f"static fields, kernel {kernel}")


EVAL_TEAMS = list(range(1, 11))


@pytest.mark.parametrize("m", EVAL_TEAMS)
def test_eval_batch_obs_matches_oracle_on_every_handle(built, m):
    """f and g of eval_batch_obs at random w against the oracle's eval_batch_obs (to 1e-12), S = 1 and S = N, on the default handle and on
    handles pinned to kernels 1 and 2 (the solve calls refuse those; eval works on every handle)."""
    import torch
    cfg = MO.team_cfg(m, 8, 3)
    B = 8
    P, W0, F = MO.moving_batch(cfg, B, 40 + m)
    W = W0 + np.random.default_rng(m).normal(0.0, 0.3, W0.shape)
    oc = O.make_config(cfg)
    for kernel in (None, 1, 2):
        s = _solver(cfg, B, kernel=kernel)
        for fld in (F, F[:, 3]):
            f, g = (t.cpu().numpy() for t in s.eval_batch(P, W, obstacles=fld)); torch.cuda.synchronize()
            fo, go = O.eval_batch_obs(oc, P, W, fld)
            assert np.all(np.abs(g - go) <= 1e-12 * np.maximum(1.0, np.abs(go))), (m, kernel, fld.ndim, np.abs(g - go).max())
            assert np.all(np.abs(f - fo) <= 1e-12 * np.maximum(1.0, np.abs(fo))), (m, kernel, fld.ndim)


def test_step_batch_obs_periods_match_oracle(built):
    """8 control periods of nmpc_step_batch_obs (solve, guess shift, plant step, in place) for 48 six-robot swarms with per-swarm moving
    paths, the period-t solve seeing rows t .. t+N-1.  The oracle's loop drives both sides (same p, guess and field each period): status
    equal, the same point on >= 97 %, and the device's shifted guess and next x0 equal to the oracle's shift of the device's solution to 1e-12."""
    import torch
    cfg = MO.team_cfg(6, 10, 4)
    B, T = 48, 8
    P, W, paths = MO.moving_batch(cfg, B, 12, L=T + cfg.N)
    P = P.copy()
    oc = O.make_config(cfg, max_iter=2000)
    s = _solver(cfg, B)
    nx = cfg.nx
    for t in range(T):
        F = np.ascontiguousarray(paths[:, t:t + cfg.N])
        ref = O.solve_batch_obs(oc, P, F, W)
        p = torch.as_tensor(P, device="cuda").clone(); w = torch.as_tensor(W, device="cuda").clone()
        r = _np(s.step_batch(p, w, None, obstacles=F)); torch.cuda.synchronize()
        assert (r["status"] == ref["status"]).all(), (t, r["status"], ref["status"])
        assert (ref["status"] == 0).all(), (t, ref["status"])
        same = np.max(np.abs(r["x"] - ref["x"]), axis=1) <= 1e-6
        print(f"period {t}: same point {same.mean():.4f}, identical iteration counts {(r['iters'] == ref['iters']).mean():.4f}")
        assert same.mean() >= 0.97, (t, np.flatnonzero(~same))
        Wd, x0d = O.shift_batch(oc, P, r["x"])
        assert np.abs(w.cpu().numpy() - Wd).max() <= 1e-12 and np.abs(p.cpu().numpy()[:, :nx] - x0d).max() <= 1e-12, t
        assert np.array_equal(p.cpu().numpy()[:, nx:], P[:, nx:])
        W, x0n = O.shift_batch(oc, P, ref["x"])
        P[:, :nx] = x0n


def test_closed_loop_episodes_with_moving_obstacles_match_oracle(built):
    """simulate_closed_loop(obstacle_paths=) against helpers.closed_loop_oracle with the same paths (the solve of period t sees rows
    t .. t+N-1): 12 two-robot swarms among two moving, growing obstacles each, 150 periods — arrival, arrival step and the state history,
    as test_closed_loop_episodes_match_oracle.  stop_tol 0.15: the swarms stall 0.08-0.17 short of their goals, so the batch holds both
    outcomes.  Seeded so that no solve of the oracle's loop fails: on a failed solve (an obstacle sweeping over a stalled robot, status 3)
    nmpc_step_batch leaves the swarm where it is while the oracle's loop applies the returned iterate, and the loops part by design."""
    import nmpc_amd
    cfg = MO.team_cfg(2, 20, 2)
    B, steps = 12, 150
    P, _, paths = MO.moving_batch(cfg, B, 78, L=steps + cfg.N)
    x0, goals = P[:, : cfg.nx], P[:, cfg.nx:]
    ep = nmpc_amd.simulate_closed_loop(_solver(cfg, B), x0, goals, max_steps=steps, stop_tol=0.15, keep_states=True, obstacle_paths=paths)
    ref = Hh.closed_loop_oracle(cfg, x0, goals, max_steps=steps, stop_tol=0.15, obstacle_paths=paths)
    print(f"episodes: arrived {ep.arrived.sum()} (oracle {ref['arrived'].sum()}), arrival steps {ep.arrival_step} (oracle {ref['arrival_step']})")
    assert ep.failed_solves == 0 and ref["failed_solves"] == 0 and ep.total_solves == ep.steps * B
    assert ref["arrived"].sum() >= 6 and (~ref["arrived"]).sum() >= 1          # the batch holds both outcomes (oracle: 11 arrive)
    assert ep.collision_free.all() and (ep.min_pair_distance >= cfg.dmin - 1e-6).all()
    same = (ep.arrival_step == ref["arrival_step"]) & (ep.arrived == ref["arrived"])
    assert ep.states.shape == ref["states"].shape
    dx = np.abs(ep.states - ref["states"]).max(axis=(0, 2))
    print(f"same arrival step {same.mean():.3f}, largest state difference per swarm {dx}")
    # measured on one MI355X: arrival and arrival step equal on all 12, states within 3e-7 over the 150 periods
    assert same.all(), (ep.arrival_step, ref["arrival_step"])
    assert (dx <= 1e-5).all(), dx


# same-point counts of the moving-obstacle rescue fixtures (long solves through restarts and retries may part at late forks), as measured on
# the GPU box, less one instance of slack
SAME_MOVING_RESCUE = {"None": 9, "3": 9, "4": 9}      # measured: 10 of 11 on every kernel


@pytest.mark.parametrize("kernel", [None, 3, 4])
def test_moving_obstacle_rescue_paths_match_oracle(built, kernel):
    """Measured on one MI355X, every kernel: status equal on all 11, the oracle's point on 10, identical iteration counts on 8.
    tests/golden/moving_obstacle_cases.npz (gen_moving_obstacle_cases.py: the first captured solve of each swarm of composite closed-loop
    soaks among moving obstacles that the cold retry rescues, that needs the elastic phase, or that stalls): status equal to the oracle's on
    every case; where both converge kkt <= 1e-8 and the restated NLP's KKT check (stationarity <= 1e-6, equality and inequality <= 1e-8;
    the oracle's own points: stationarity 3e-8 - 2e-7) with every obstacle row clear at its stage position."""
    import torch
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "moving_obstacle_cases.npz"))
    cfg = MO.team_cfg(6, 25, 8)
    P, W, F = z["p"], z["w"], z["obs"]
    ref = O.solve_batch_obs(O.make_config(cfg, max_iter=2000), P, F, W)
    assert (ref["status"][z["kind"] < 2] == 0).all() and (ref["status"][z["kind"] == 2] == 4).all(), (z["kind"], ref["status"])
    r = _np(_solver(cfg, len(P), kernel=kernel).solve_batch(P, W, obstacles=F)); torch.cuda.synchronize()
    same = np.max(np.abs(r["x"] - ref["x"]), axis=1) <= 1e-6
    print(f"moving rescue fixtures, kernel {kernel}: kinds {z['kind'].tolist()}, status {r['status'].tolist()} (oracle {ref['status'].tolist()}), "
          f"same point {same.sum()} of {len(P)}, iterations {r['iters'].tolist()} (oracle {ref['iters'].tolist()})")
    assert (r["status"] == ref["status"]).all(), (kernel, r["status"], ref["status"])
    assert same.sum() >= SAME_MOVING_RESCUE[str(kernel)], (kernel, same)
    for b in np.flatnonzero(r["status"] == 0):
        assert r["kkt"][b] <= 1e-8, (b, r["kkt"][b])
        k = MO.kkt_report(cfg, r["x"][b], P[b], F[b], tol_active=1e-2)
        assert k["stat"] <= 1e-6 and k["eq"] <= 1e-8 and k["ineq"] <= 1e-8 and k["bnd"] <= 1e-12, (b, k)
        assert MO.obstacle_values(cfg, r["x"][b], F[b]).min() >= cfg.margin - 1e-8, b
