"""GPU: obstacles as per-instance solve parameters (nmpc_solve_batch_obs, nmpc_step_batch_obs, nmpc_eval_batch_obs; NmpcSolver(...)(obstacles=),
simulate_closed_loop(obstacle_paths=)).  Checked against the config path (bit-identical by construction), the unchanged CPU oracle (one oracle
config per field) and, for moving obstacles, an independent restatement of the NLP (tests/moving_obstacles_ref.py)."""
import numpy as np
import pytest

from oracle import nlp_ref as R, oracle_lib as O
from tests import helpers as Hh
from tests import moving_obstacles_ref as MO

pytestmark = pytest.mark.gpu

FIELDS = ("x", "f", "status", "iters", "kkt")


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items() if k in FIELDS}


def _field(seed, K=8):
    """a composite-like field: K circles in [-1.5, 1.5]^2, radii U[0.125, 0.2] (bench.py composite_obstacles with another seed)"""
    rng = np.random.default_rng(seed)
    return [(float(x), float(y), float(r)) for x, y, r in zip(rng.uniform(-1.5, 1.5, K), rng.uniform(-1.5, 1.5, K), rng.uniform(0.125, 0.2, K))]


def _composite(N=25, obstacles=None):
    c = R.cfg_six(N); c.obstacles = list(obstacles if obstacles is not None else _field(7)); c.rob_dim = 0.2; c.margin = 0.1
    return c


def _third(N=100):
    import nmpc_amd
    return Hh.to_oracle_cfg(nmpc_amd.third_scenario_obstacles(N))


def _solver(ocfg, B, kernel=None, max_iter=600):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(ocfg, max_iter=max_iter), max_batch=B, kernel=kernel)


def _same(a, b, what=""):
    """bit-identical per-instance outputs (a NaN objective — status 3 — equals itself)"""
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), \
            (what, k, np.flatnonzero([not np.array_equal(u, v, equal_nan=True) for u, v in zip(x, y)])[:20])


CONFIGS = {"composite": (lambda: _composite(25), 256, 4), "third": (lambda: _third(100), 64, 5), "mix3": (lambda: Hh.cfg_mix3(10), 64, 6)}


@pytest.mark.parametrize("kernel", [3, 4, 5])
@pytest.mark.parametrize("name", ["composite", "third", "mix3"])
def test_config_field_as_parameter_is_bit_identical(built, name, kernel):
    """Every instance given the handle's own field, static (S = 1) and per stage (S = N, the entry repeated): x, f, status, iters and kkt equal
    to the plain solve bit for bit, at each pinned column shape; eval_batch equal on g, f to 1e-12 (the eval kernel sums f with atomics)."""
    import torch
    mk, B, idx = CONFIGS[name]
    ocfg = mk()
    P, W0 = Hh.batch(ocfg, B, idx)
    s = _solver(ocfg, B, kernel=kernel)
    K, N = ocfg.K, ocfg.N
    f1 = np.broadcast_to(np.array(ocfg.obstacles), (B, K, 3)).copy()
    fN = np.broadcast_to(np.array(ocfg.obstacles), (B, N, K, 3)).copy()
    ref = _np(s.solve_batch(P, W0))
    r1 = _np(s.solve_batch(P, W0, obstacles=f1))
    rN = _np(s.solve_batch(P, W0, obstacles=torch.as_tensor(fN, device="cuda")))
    torch.cuda.synchronize()
    print(f"{name} kernel {kernel}: status-0 {np.mean(ref['status'] == 0):.3f}, mean iterations {ref['iters'].mean():.2f}")
    _same(r1, ref, "S=1")
    _same(rN, ref, "S=N")
    fe, ge = (t.cpu().numpy() for t in s.eval_batch(P, ref["x"]))
    for fld in (f1, fN):
        fo, go = (t.cpu().numpy() for t in s.eval_batch(P, ref["x"], obstacles=fld))
        assert np.array_equal(go, ge)
        assert np.all(np.abs(fo - fe) <= 1e-12 * np.maximum(1.0, np.abs(fe)))


@pytest.mark.parametrize("kernel", [3, 4])
def test_heterogeneous_batch_matches_per_field_handles_and_oracle(built, kernel):
    """1,024 composite instances over 16 seeded fields (starts and goals clear of their own field): each group bit-identical to a handle whose
    config holds that field (same pinned shape), and against the CPU oracle with that field: status equal in every group; over the batch, as in
    test_full_size_bench_batches_match_oracle, identical iteration counts >= 0.97 and same basin at 1e-6 >= 0.99 (in a group of 64 one
    instance is 1.6 %)."""
    import torch
    G, per = 16, 64
    B = G * per
    cfgs = [_composite(25, _field(1000 + j)) for j in range(G)]
    PW = [Hh.batch(c, per, 40 + j) for j, c in enumerate(cfgs)]
    P = np.concatenate([pw[0] for pw in PW]); W0 = np.concatenate([pw[1] for pw in PW])
    fld = np.repeat(np.stack([np.array(c.obstacles) for c in cfgs]), per, axis=0)
    s = _solver(cfgs[0], B, kernel=kernel, max_iter=2000)
    r = _np(s.solve_batch(P, W0, obstacles=fld)); torch.cuda.synchronize()
    same, iters = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for j, c in enumerate(cfgs):
        sl = slice(j * per, (j + 1) * per)
        rj = _np(_solver(c, per, kernel=kernel, max_iter=2000).solve_batch(P[sl], W0[sl])); torch.cuda.synchronize()
        _same({k: v[sl] for k, v in r.items()}, rj, "group %d" % j)
        ref = O.solve_batch(O.make_config(c, max_iter=2000), P[sl], W0[sl])
        assert (r["status"][sl] == ref["status"]).all(), (j, r["status"][sl], ref["status"])
        same[sl] = np.max(np.abs(r["x"][sl] - ref["x"]), axis=1) <= 1e-6
        iters[sl] = r["iters"][sl] == ref["iters"]
    print(f"16 fields: same basin {same.mean():.4f} (per field {[round(same[j * per:(j + 1) * per].mean(), 3) for j in range(G)]}), "
          f"identical iteration counts {iters.mean():.4f}, status 0 {np.mean(r['status'] == 0):.4f}")
    assert same.mean() >= 0.99 and iters.mean() >= 0.97
    assert (r["kkt"][r["status"] == 0] <= 1e-8).all()


def test_dispatch_order_reads_the_instance_field(built):
    """order = a random permutation: results identical to the unordered call, with every instance holding a different field (a field read at
    the workgroup index would solve another instance's problem)."""
    import torch
    B = 256
    ocfg = _composite(25)
    rng = np.random.default_rng(11)
    fld = np.stack([np.array(_field(2000 + b)) for b in range(B)])
    P = np.stack([Hh.instance(rng, _composite(25, list(map(tuple, fld[b])))) for b in range(B)])
    W0 = np.stack([R.cold_start(ocfg, p[: ocfg.nx]) for p in P])
    for kernel in (None, 3):
        s = _solver(ocfg, B, kernel=kernel)
        a = _np(s.solve_batch(P, W0, obstacles=fld))
        b = _np(s.solve_batch(P, W0, obstacles=fld, order=rng.permutation(B)))
        torch.cuda.synchronize()
        _same(a, b, "order, kernel %s" % kernel)
        assert (a["status"] == 0).mean() >= 0.99


def _moving_cfg(N=10):
    c = R.cfg_six(N); c.obstacles = [(0.0, 0.0, 0.1)] * 4; c.rob_dim = 0.2; c.margin = 0.1
    return c


def test_moving_obstacles_eval_matches_restatement(built):
    """g of eval_batch(obstacles=[B, N, K, 3]) at random w equals the numpy restatement (oracle rows, obstacle rows with stage-indexed
    centres) to 1e-12."""
    import torch
    cfg = _moving_cfg(10)
    B = 64
    P, W0, F = MO.moving_batch(cfg, B, 5)
    rng = np.random.default_rng(6)
    W = W0 + rng.normal(0.0, 0.3, W0.shape)
    s = _solver(cfg, B)
    f, g = (t.cpu().numpy() for t in s.eval_batch(P, W, obstacles=F)); torch.cuda.synchronize()
    for b in range(B):
        gr = MO.constraints(cfg, W[b], P[b], F[b])
        assert np.all(np.abs(g[b] - gr) <= 1e-12 * np.maximum(1.0, np.abs(gr))), (b, np.abs(g[b] - gr).max())
        assert abs(f[b] - R.objective(cfg, W[b], P[b])) <= 1e-12 * max(1.0, abs(f[b]))


def test_moving_obstacles_solve_kkt(built):
    """512 six-robot swarms among four moving, growing obstacles: >= 99 % status 0, each with kkt <= 1e-8; on every status-0 instance the
    independent KKT check (stationarity <= 1e-6, equality and inequality <= 1e-8) and every obstacle row clear at that obstacle's stage
    position (g_obs >= margin - 1e-8).  The check's active set: rows within 1e-2 of their bound (the barrier multiplier mu / s of a row
    further away is below 1e-6 at the final barrier parameter)."""
    import torch
    cfg = _moving_cfg(10)
    B = 512
    P, W0, F = MO.moving_batch(cfg, B, 7)
    r = _np(_solver(cfg, B, max_iter=2000).solve_batch(P, W0, obstacles=F)); torch.cuda.synchronize()
    ok = r["status"] == 0
    print(f"moving obstacles: status 0 on {ok.mean():.4f} of {B}, statuses {np.unique(r['status'], return_counts=True)}, mean iterations {r['iters'].mean():.2f}")
    assert ok.mean() >= 0.99
    assert (r["kkt"][ok] <= 1e-8).all()
    worst = dict(stat=0.0, eq=0.0, ineq=0.0)
    for b in np.flatnonzero(ok):
        k = MO.kkt_report(cfg, r["x"][b], P[b], F[b], tol_active=1e-2)
        for key in worst:
            worst[key] = max(worst[key], k[key])
        assert k["stat"] <= 1e-6 and k["eq"] <= 1e-8 and k["ineq"] <= 1e-8, (b, k)
        assert MO.obstacle_values(cfg, r["x"][b], F[b]).min() >= cfg.margin - 1e-8, b
    print("worst KKT residuals over the status-0 instances:", worst)
    # the field matters: the same instances against the placeholder field of the config are other problems
    s2 = _np(_solver(cfg, B, max_iter=2000).solve_batch(P, W0)); torch.cuda.synchronize()
    assert not np.array_equal(s2["x"], r["x"])


def test_stage0_precheck_uses_the_instance_field(built):
    """An instance whose entry 0 covers its x0 returns status 3 (the rest of its field clear); the rest of the batch is identical to a run
    without it."""
    import torch
    ocfg = _composite(25)
    B = 64
    P, W0 = Hh.batch(ocfg, B, 4)
    K, N = ocfg.K, ocfg.N
    fld = np.broadcast_to(np.array(ocfg.obstacles), (B, N, K, 3)).copy()
    bad = fld.copy()
    bad[5, 0, 3] = (P[5, 0], P[5, 1], 0.3)           # entry 0 of obstacle 3 sits on robot 0 of instance 5
    s = _solver(ocfg, B, kernel=3)
    a = _np(s.solve_batch(P, W0, obstacles=fld))
    b = _np(s.solve_batch(P, W0, obstacles=bad))
    torch.cuda.synchronize()
    assert b["status"][5] == 3 and a["status"][5] != 3
    keep = np.arange(B) != 5
    _same({k: v[keep] for k, v in a.items()}, {k: v[keep] for k, v in b.items()}, "rest of the batch")


def _episode_equal(a, b):
    for k in ("steps", "failed_solves", "total_solves"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("arrived", "arrival_step", "collision_free", "min_pair_distance", "deadlocked", "final_error", "mean_iters_by_step", "states"):
        va, vb = getattr(a, k), getattr(b, k)
        assert (va is None and vb is None) or np.array_equal(va, vb), k


def test_closed_loop_with_obstacle_paths(built):
    """(a) a time-invariant obstacle_paths reproduces the config-field run exactly (fused step and previous_plan); (b) one robot whose straight
    path to its goal is crossed by an obstacle moving at constant velocity arrives, collision-free against the moving obstacle at every period;
    (c) simulate_closed_loop_fleets with obstacle_paths gives the single-fleet run's per-swarm results."""
    import nmpc_amd
    ocfg = Hh.cfg_mix3(10)
    pcfg = Hh.to_product_cfg(ocfg, max_iter=600)
    B, steps = 32, 40
    P, _ = Hh.batch(ocfg, B, 8)
    x0, goals = P[:, : ocfg.nx], P[:, ocfg.nx:]
    L = steps + ocfg.N
    paths = np.broadcast_to(np.array(ocfg.obstacles), (B, L, ocfg.K, 3)).copy()
    for mode in ("apply", "previous_plan"):
        a = nmpc_amd.simulate_closed_loop(nmpc_amd.NmpcSolver(pcfg, max_batch=B), x0, goals, steps, on_failure=mode, keep_states=True)
        b = nmpc_amd.simulate_closed_loop(nmpc_amd.NmpcSolver(pcfg, max_batch=B), x0, goals, steps, on_failure=mode, keep_states=True, obstacle_paths=paths)
        _episode_equal(a, b)
    # (b) the robot drives from (-1.2, 0) to (1.2, 0); the obstacle crosses the x axis at x = 0 when a straight drive would be there
    one = R.cfg_one(20); one.T = 0.1; one.obstacles = [(0.0, 0.0, 0.15)]; one.rob_dim = 0.1; one.margin = 0.05
    free = R.cfg_one(20); free.T = 0.1
    steps1 = 400
    t_meet = 1.2 / one.v_max
    vo = 0.5 * one.v_max
    t = np.arange(steps1 + one.N) * one.T
    path = np.stack([np.zeros_like(t), vo * (t - t_meet), np.full_like(t, 0.15)], axis=1)[None, :, None, :]
    x0_1, g1 = np.array([[-1.2, 0.0, 0.0]]), np.array([[1.2, 0.0, 0.0]])
    e = nmpc_amd.simulate_closed_loop(_solver(one, 1, max_iter=2000), x0_1, g1, steps1, obstacle_paths=path, keep_states=True)
    X = e.states[:, 0]
    clear = np.hypot(X[:, 0] - path[0, : len(X), 0, 0], X[:, 1] - path[0, : len(X), 0, 1]) - one.rob_dim - 0.15
    print(f"crossing obstacle: arrived {e.arrived[0]} at period {e.arrival_step[0]}, smallest clearance {clear.min():.4f} (margin {one.margin})")
    assert e.arrived[0] and e.collision_free[0] and clear.min() >= one.margin - 1e-6
    # without the obstacle rows the straight drive would have hit it
    e0 = nmpc_amd.simulate_closed_loop(_solver(free, 1, max_iter=2000), x0_1, g1, steps1, keep_states=True)
    X0 = e0.states[:, 0]
    assert (np.hypot(X0[:, 0] - path[0, : len(X0), 0, 0], X0[:, 1] - path[0, : len(X0), 0, 1]) - one.rob_dim - 0.15).min() < one.margin
    # (c) fleets: moving paths, different per swarm
    rng = np.random.default_rng(9)
    mv = paths.copy()
    vel = rng.uniform(-0.02, 0.02, (B, 1, ocfg.K, 2)) * ocfg.T
    mv[:, :, :, :2] += np.arange(L)[None, :, None, None] * vel
    single = nmpc_amd.simulate_closed_loop(nmpc_amd.NmpcSolver(pcfg, max_batch=B), x0, goals, steps, obstacle_paths=mv)
    fleets = nmpc_amd.simulate_closed_loop_fleets(pcfg, x0, goals, steps, fleets=4, obstacle_paths=mv)
    for k in ("arrived", "arrival_step", "collision_free", "min_pair_distance", "deadlocked", "final_error"):
        assert np.array_equal(getattr(fleets, k), getattr(single, k)), k


def test_errors(built):
    """Host: a wrong K or S, or a handle without obstacle rows -> ValueError.  ABI: obs_stages not 1 or N, obs == NULL, n_obs == 0 ->
    NMPC_E_ARG; handles pinned to kernel 1 / 2 -> NMPC_E_UNSUPPORTED on the obstacle solve calls and still solve plain calls.
    PipelinedSolver with obstacles= equals the serial solves."""
    import torch
    import nmpc_amd
    from nmpc_amd import _lib
    ocfg = Hh.cfg_mix3(10)
    B, N, K = 8, ocfg.N, ocfg.K
    P, W0 = Hh.batch(ocfg, B, 6)
    s = _solver(ocfg, B)
    good = np.broadcast_to(np.array(ocfg.obstacles), (B, K, 3)).copy()
    for bad in (np.zeros((B, K + 1, 3)), np.zeros((B, N - 1, K, 3)), np.zeros((B, N + 1, K, 3)), np.zeros((B - 1, K, 3)), np.zeros((B, K, 2))):
        with pytest.raises(ValueError):
            s.solve_batch(P, W0, obstacles=bad)
        with pytest.raises(ValueError):
            s.eval_batch(P, W0, obstacles=bad)
    s0 = _solver(R.cfg_six(10), B)
    P6, W6 = Hh.batch(R.cfg_six(10), B, 2)
    with pytest.raises(ValueError):
        s0.solve_batch(P6, W6, obstacles=np.zeros((B, 0, 3)))
    # raw ABI
    L = _lib.load()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    p, w0, ob = dev(P), dev(W0), dev(good)
    out = torch.empty_like(w0)
    g = torch.empty((B, s.n_g), dtype=torch.float64, device="cuda")
    pc, wc, ws = p.clone(), w0.clone(), torch.empty_like(w0)
    p6, w6, o6 = dev(P6), dev(W6), torch.empty((B, s0.n_var), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def solve(h, obs_ptr, S):
        return L.nmpc_solve_batch_obs(h, B, p.data_ptr(), obs_ptr, S, w0.data_ptr(), out.data_ptr(), None, None, None, None, None, st)
    assert solve(s._h, ob.data_ptr(), 1) == 0
    assert solve(s._h, ob.data_ptr(), 2) == -1 and solve(s._h, ob.data_ptr(), 0) == -1 and solve(s._h, ob.data_ptr(), N + 1) == -1
    assert solve(s._h, None, 1) == -1
    assert L.nmpc_eval_batch_obs(s._h, B, p.data_ptr(), w0.data_ptr(), None, 1, None, g.data_ptr(), st) == -1
    assert L.nmpc_eval_batch_obs(s._h, B, p.data_ptr(), w0.data_ptr(), ob.data_ptr(), 3, None, g.data_ptr(), st) == -1
    assert L.nmpc_step_batch_obs(s._h, B, pc.data_ptr(), wc.data_ptr(), ws.data_ptr(), None, 1, None, None, None, None, None, st) == -1
    assert L.nmpc_solve_batch_obs(s0._h, B, p6.data_ptr(), ob.data_ptr(), 1, w6.data_ptr(), o6.data_ptr(), None, None, None, None, None, st) == -1
    for kernel in (1, 2):
        sk = _solver(ocfg, B, kernel=kernel)
        assert solve(sk._h, ob.data_ptr(), 1) == -2
        assert L.nmpc_step_batch_obs(sk._h, B, pc.data_ptr(), wc.data_ptr(), ws.data_ptr(), ob.data_ptr(), 1, None, None, None, None, None, st) == -2
        with pytest.raises(RuntimeError, match="NMPC_E_UNSUPPORTED"):
            sk.solve_batch(P, W0, obstacles=good)
        r = _np(sk.solve_batch(P, W0)); torch.cuda.synchronize()
        assert (r["status"] == 0).sum() >= B - 1, (kernel, r["status"])
    torch.cuda.synchronize()
    # PipelinedSolver: the field travels with the batch
    rng = np.random.default_rng(3)
    pipe = nmpc_amd.PipelinedSolver(Hh.to_product_cfg(ocfg, max_iter=600), max_batch=B, depth=2)
    fields = [good + rng.uniform(-0.05, 0.05, good.shape) * np.array([1.0, 1.0, 0.0]) for _ in range(4)]
    res = [pipe.solve_batch(P, W0, obstacles=f) for f in fields]
    pipe.synchronize()
    for f, r in zip(fields, res):
        _same(_np(r), _np(s.solve_batch(P, W0, obstacles=f)), "pipelined")
    torch.cuda.synchronize()
