"""-m gpu: the LIDAR-ray distance-state NMPC (V4 = AllScripts/obs_avoid_static_first_scenario_v4.py) —
the HIP path through the C ABI of include/nmpc_lidar.h against the CPU oracle on the same inputs.

Tolerances: f, g element-wise 1e-12; solve: status equal, max |w_hip - w_oracle| <= 1e-6, |f| relative 1e-6, reported KKT <= 1e-8;
independent least-squares KKT report on the HIP output."""
import numpy as np
import pytest

from oracle import lidar_ref as LR, oracle_lib as O
from tests import helpers as Hh
from tests.lidar_variants import batch as _batch, world as _world      # noqa: F401  (the generator lives with the recipes that share it)

pytestmark = pytest.mark.gpu

W_TOL = 1e-6


def _product(cfg, **kw):
    import nmpc_amd
    return nmpc_amd.LidarProblemConfig(N=cfg.N, Nc=cfg.Nc, R=cfg.R, T=cfg.T, q=tuple(cfg.q), r=tuple(cfg.r), lw=cfg.lw, v_max=cfg.v_max, w_max=cfg.w_max,
                                       xy_max=cfg.xy_max, th_max=cfg.th_max, d_min=cfg.d_min, d_max=cfg.d_max, **kw)


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_lidar_eval_and_shift_kernels(built):
    import torch
    import nmpc_amd
    rng = np.random.default_rng(3)
    for cfg in (LR.lidar_v4(), LR.lidar_v3(20), LR.LidarConfig(N=7, Nc=3, R=4)):
        pc = _product(cfg)
        for a, b in zip(pc.bounds(), LR.bounds(cfg)):
            np.testing.assert_array_equal(a, b)                      # two independent statements of V4:158-176
        s = nmpc_amd.LidarSolver(pc, max_batch=9)
        B = 9
        P = rng.normal(size=(B, cfg.n_p)); W = rng.normal(size=(B, cfg.n_var)); W[:, 3: 3 + cfg.R] = np.abs(W[:, 3: 3 + cfg.R]) + 0.3
        W[:, : cfg.ns * (cfg.N + 1)].reshape(B, cfg.N + 1, cfg.ns)[:, :, 3:] = rng.uniform(0.3, 3.0, (B, cfg.N + 1, cfg.R))
        f, g = s.eval_batch(P, W); torch.cuda.synchronize()
        fo, go = O.lidar_eval_batch(cfg, P, W)
        gn = np.stack([LR.constraints(cfg, W[b], P[b]) for b in range(2)])
        assert np.abs(go[:2] - gn).max() < 1e-12
        assert np.abs(g.cpu().numpy() - go).max() <= 1e-12 * max(1.0, np.abs(go).max())
        assert np.max(np.abs(f.cpu().numpy() - fo) / np.maximum(1.0, np.abs(fo))) < 1e-12
        wn = s.shift_batch(W).cpu().numpy()
        assert np.array_equal(wn, np.stack([LR.shift_guess(cfg, w) for w in W]))      # pure data movement: bit-exact


@pytest.mark.parametrize("name,cfg,B", [("v4", LR.lidar_v4(), 96), ("v3", LR.lidar_v3(), 24), ("v4_aligned", LR.LidarConfig(aligned_bounds=True), 64),
                                        ("short", LR.LidarConfig(N=12, Nc=6, R=4, aligned_bounds=True), 130)])
def test_lidar_solve_matches_oracle(built, name, cfg, B):
    import torch
    import nmpc_amd
    P, W0 = _batch(cfg, B, 11)
    lbx, ubx, _, _ = LR.bounds(cfg)
    s = nmpc_amd.LidarSolver(_product(cfg, max_iter=1500), lbx=lbx, ubx=ubx, max_batch=B)
    r = _np(s.solve_batch(P, W0)); torch.cuda.synchronize()
    ref = O.lidar_solve_batch(cfg, P, W0, max_iter=1500)
    print(f"{name}: status hip {np.bincount(r['status'], minlength=5)} oracle {np.bincount(ref['status'], minlength=5)}, iters hip mean {r['iters'].mean():.1f} max {r['iters'].max()} "
          f"oracle mean {ref['iters'].mean():.1f}")
    assert (r["status"] == ref["status"]).all(), (r["status"], ref["status"])
    conv = r["status"] == 0
    assert conv.mean() >= 0.9, r["status"]
    assert (r["kkt"][conv] <= 1e-8).all()
    dw = np.max(np.abs(r["x"] - ref["x"]), axis=1)
    assert (dw[conv] <= W_TOL).mean() >= 0.97, dw
    same = conv & (dw <= W_TOL)
    assert (np.abs(r["f"] - ref["f"])[same] <= 1e-6 * np.maximum(1.0, np.abs(ref["f"][same]))).all()
    assert (r["iters"] == ref["iters"])[conv].mean() >= 0.9
    for b in np.where(conv)[0][:6]:
        k = LR.kkt_report(cfg, r["x"][b], P[b], tol_active=1e-4)
        assert k["stat"] < 1e-5 and k["eq"] < 1e-9 and k["bnd"] == 0.0, (b, k)
    # X_0 pinned; the caller's bounds hold entry by entry
    assert np.array_equal(r["x"][:, :3], P[:, :3]) and np.array_equal(r["x"][:, 3: 3 + cfg.R], P[:, 6: 6 + cfg.R])
    assert (r["x"][conv] >= lbx - 1e-12).all() and (r["x"][conv] <= ubx + 1e-12).all()


def test_lidar_reference_call_surface_and_closed_loop(built):
    """the loop of V4:209-300 with a synthetic scan: p = [x0; xs; scan; B0], the keyword call with the script's own bounds arrays,
    u = first control, shift of the guess; 6 control periods with the plant x0 + T f(x0, u0) standing in for the robot."""
    import nmpc_amd
    cfg = nmpc_amd.lidar_v4()
    ocfg = LR.lidar_v4()
    opts = {'print_time': 0, 'ipopt': {'max_iter': 2000, 'print_level': 0, 'acceptable_tol': 1e-8, 'acceptable_obj_change_tol': 1e-6}}
    lbx, ubx, lbg, ubg = cfg.bounds()
    solver = nmpc_amd.lidar_nlpsol('solver', 'ipopt', cfg, opts, lbx=lbx, ubx=ubx)
    obst = [(1.2, 0.9, 0.25), (2.0, 2.2, 0.3)]
    pose = np.array([0.0, 0.0, 0.0]); xs = np.array([3.0, 2.5, 0.0])
    scan = LR.scan_of_world(pose, obst, cfg.R)
    x0 = np.concatenate([pose, scan])
    w = nmpc_amd.lidar_cold_start(cfg, x0)
    ns, N, Nc = cfg.ns, cfg.N, cfg.Nc
    d0 = np.linalg.norm(pose[:2] - xs[:2])
    for it in range(6):
        p = nmpc_amd.lidar_params(cfg, pose, xs, scan)
        sol = solver(x0=w.reshape(-1, 1), p=p.reshape(-1, 1), lbx=lbx.reshape(-1, 1), ubx=ubx.reshape(-1, 1), lbg=lbg.reshape(1, -1), ubg=ubg.reshape(1, -1))
        assert solver.stats()['success'], solver.stats()
        assert sol['x'].shape == (cfg.n_var, 1) and sol['g'].shape == (cfg.n_g, 1) and np.abs(sol['g']).max() < 1e-8
        assert abs(sol['f'] - LR.objective(ocfg, sol['x'], p)) < 1e-9 * max(1.0, abs(sol['f']))
        u = sol['x'][ns * (N + 1):].reshape(Nc, 2)
        assert (np.abs(u[:, 0]) <= cfg.v_max + 1e-12).all() and (np.abs(u[:, 1]) <= cfg.w_max + 1e-12).all()
        pose = pose + cfg.T * np.array([u[0, 0] * np.cos(pose[2]), u[0, 0] * np.sin(pose[2]), u[0, 1]])
        scan = LR.scan_of_world(pose, obst, cfg.R)
        w = solver.shift_batch(sol['x'].reshape(1, -1)).cpu().numpy()[0]
        assert np.array_equal(w, LR.shift_guess(ocfg, sol['x']))
    assert np.linalg.norm(pose[:2] - xs[:2]) < d0
    with pytest.raises(ValueError):
        solver(x0=w, p=p, lbx=lbx * 2)


def test_lidar_closed_loop_episodes_match_oracle(built):
    """nmpc_amd.simulate_lidar_closed_loop — the main loop of V4:209-300 for a batch of simulated robots (scan refresh from a synthetic world
    on the device, x0[3:] = Scan, goal sequencing ne < 0.2 over ng = 2 goals, the V4:258-270 shift) — against the same loop driven by the
    oracle (tests/helpers.lidar_closed_loop_oracle): arrival step equal on >= 0.97 of the robots, every solve converged on both sides, the
    device scan equal to lidar_ref.scan_of_world, minimum obstacle clearance reported and equal where the arrival steps are."""
    import torch
    import nmpc_amd
    # V4's NLP at a horizon the oracle walks through in seconds: R = 10 rays as V4, N = 25 stages of 0.3 s (the 7.5 s look-ahead of V4's
    # N = 100 x 0.075 s; with a shorter look-ahead the quadratic cost stalls short of the 0.2 m arrival radius), bounds aligned with the
    # packing (with the script's misaligned bounds the later stages of every plan are confined to x, y, theta >= 0.15: its own second goal
    # (0, 2.5, -0.785) cannot be approached; the solve with those bounds is tested above)
    cfg = LR.LidarConfig(N=25, Nc=12, R=10, T=0.3, aligned_bounds=True)
    lbx, ubx, _, _ = LR.bounds(cfg)
    B = 64
    pose0, goals, world = Hh.lidar_episode_batch(20210141 + 66, B)
    s = nmpc_amd.LidarSolver(_product(cfg, max_iter=600), lbx=lbx, ubx=ubx, max_batch=B)
    # the device scan is the oracle's scan
    sc = s.scan_batch(pose0, world).cpu().numpy()
    ref_sc = np.stack([LR.scan_of_world(pose0[b], [tuple(o) for o in world[b]], cfg.R) for b in range(B)])
    assert np.abs(sc - ref_sc).max() <= 1e-13 and (sc < 3.5).any()
    steps = 140
    res = nmpc_amd.simulate_lidar_closed_loop(s, pose0, goals, world, max_steps=steps, keep_poses=True)
    ref = Hh.lidar_closed_loop_oracle(cfg, pose0, goals, world, steps, lbx=lbx, ubx=ubx, max_iter=600)
    same = res.arrival_step == ref["arrival_step"]
    print(f"lidar closed loop: {res.steps} periods, arrived {res.arrived.mean():.3f} (oracle {ref['arrived'].mean():.3f}), arrival step equal {same.mean():.3f}, "
          f"failed solves {res.failed_solves} of {res.total_solves} (oracle {ref['failed_solves']}), min clearance {res.min_clearance.min():.3f} m, "
          f"mean iterations first / later periods {res.mean_iters_by_step[0]:.1f} / {res.mean_iters_by_step[1:].mean():.1f}")
    assert res.failed_solves == 0 and ref["failed_solves"] == 0
    # (measured on the oracle: 0.77 of these 64 robots reach both goals within 140 periods, the others stall short of the 0.2 m radius —
    # quadratic cost against the 1/d^2 repulsion; 0 failed solves, minimum clearance 0.164 m)
    assert res.arrived.mean() >= 0.7 and (res.arrived == ref["arrived"]).mean() >= 0.97
    assert same.mean() >= 0.97, (res.arrival_step, ref["arrival_step"])
    assert np.abs(res.min_clearance - ref["min_clearance"])[same].max() <= 1e-5
    assert (res.min_clearance > 0.0).all()                       # no robot centre ever inside an obstacle
    n = min(res.poses.shape[0], ref["poses"].shape[0])
    dp = np.abs(res.poses[:n] - ref["poses"][:n]).max(axis=(0, 2))
    assert (dp[same] <= 1e-5).mean() >= 0.95, dp


def test_lidar_edge_cases(built):
    import ctypes as C
    import torch
    import nmpc_amd
    cfg = LR.LidarConfig(N=12, Nc=6, R=4, aligned_bounds=True)
    lbx, ubx, _, _ = LR.bounds(cfg)
    s = nmpc_amd.LidarSolver(_product(cfg), lbx=lbx, ubx=ubx, max_batch=4)
    r = s.solve_batch(np.zeros((0, cfg.n_p)), np.zeros((0, cfg.n_var)))
    assert r["x"].shape == (0, cfg.n_var)
    P, W0 = _batch(cfg, 8, 5)
    with pytest.raises(ValueError):
        s.solve_batch(P, W0)
    # a scan below the lower bound of the (pinned) stage-0 distance states: status 3, guess returned (with X_0 pinned)
    P2 = P[:2].copy(); P2[0, 6] = 0.05
    W2 = W0[:2].copy()
    r2 = _np(s.solve_batch(P2, W2)); ref2 = O.lidar_solve_batch(cfg, P2, W2)
    assert r2["status"][0] == 3 and ref2["status"][0] == 3 and r2["status"][1] == ref2["status"][1] == 0
    # iteration limit 0
    s0 = nmpc_amd.LidarSolver(_product(cfg, max_iter=0), lbx=lbx, ubx=ubx, max_batch=4)
    r0 = _np(s0.solve_batch(P[:4], W0[:4])); ref0 = O.lidar_solve_batch(cfg, P[:4], W0[:4], max_iter=0)
    assert (r0["status"] == 1).all() and (r0["iters"] == 0).all() and np.abs(r0["x"] - ref0["x"]).max() <= 1e-15
    # bad bounds / configs are rejected by the C ABI
    L = nmpc_amd._lib.load(); h = C.c_void_p(); dp = C.POINTER(C.c_double)
    cc = _product(cfg).to_c()
    bad = lbx.copy(); bad[20] = ubx[20] + 1.0
    assert L.nmpc_lidar_create(C.byref(cc), bad.ctypes.data_as(dp), ubx.ctypes.data_as(dp), 4, C.byref(h)) == -1
    c2 = _product(cfg); c2.Nc = cfg.N + 1
    assert L.nmpc_lidar_create(C.byref(c2.to_c()), lbx.ctypes.data_as(dp), ubx.ctypes.data_as(dp), 4, C.byref(h)) == -1
    assert L.nmpc_lidar_n_var(None) == -1
    # scan / plant helpers of the closed loop: no obstacle -> scan_max on every ray; plant step in place of the pose part of p; bad arguments
    pose = np.array([[0.0, 0.0, 0.3], [1.0, -0.5, 2.0]])
    sc = s.scan_batch(pose, np.zeros((2, 0, 3))).cpu().numpy()
    assert sc.shape == (2, cfg.R) and (sc == 3.5).all()
    ob = (float(np.cos(0.3)), float(np.sin(0.3)), 0.25)          # on ray 0 of the first robot, one metre out
    one = s.scan_batch(pose[:1], np.array([[ob]]), scan_max=3.5).cpu().numpy()[0]
    ref1 = LR.scan_of_world(pose[0], [ob], cfg.R)
    assert np.abs(one - ref1).max() <= 1e-13 and abs(one[0] - 0.75) <= 1e-12 and (one[1:] == 3.5).all()
    # a pose inside an obstacle's circle reads range 0 on every ray (never a negative range); a pose touching it reads ~0
    # on the ray through the contact point; the device scan equals the checker's
    inside = np.array([[float(ob[0]) - 0.1, float(ob[1]), 0.3]])
    sin_ = s.scan_batch(inside, np.array([[ob]])).cpu().numpy()[0]
    assert (sin_ == 0.0).all() and np.array_equal(sin_, LR.scan_of_world(inside[0], [ob], cfg.R))
    tang = np.array([[float(ob[0]) - (0.25 + 1e-9) * np.cos(0.3), float(ob[1]) - (0.25 + 1e-9) * np.sin(0.3), 0.3]])      # a nanometre off the surface
    st_ = s.scan_batch(tang, np.array([[ob]])).cpu().numpy()[0]
    assert (st_ >= 0.0).all() and st_[0] <= 1e-7 and np.abs(st_ - LR.scan_of_world(tang[0], [ob], cfg.R)).max() <= 1e-7
    assert L.nmpc_lidar_scan_batch(1, cfg.R, 1, None, None, C.c_double(3.5), None, None) == -1
    assert L.nmpc_lidar_scan_batch(0, cfg.R, 0, None, None, C.c_double(3.5), None, None) == 0
    assert L.nmpc_lidar_scan_batch(1, 99, 0, None, None, C.c_double(3.5), None, None) == -1
    Pd = torch.as_tensor(P[:4], device="cuda").clone(); r4 = s.solve_batch(Pd, W0[:4])
    want = s.plant_batch(Pd, r4["x"]).cpu().numpy()
    u0 = r4["x"][:, cfg.ns * (cfg.N + 1): cfg.ns * (cfg.N + 1) + 2].cpu().numpy(); p0 = P[:4, :3]
    assert np.abs(want - (p0 + cfg.T * np.stack([u0[:, 0] * np.cos(p0[:, 2]), u0[:, 0] * np.sin(p0[:, 2]), u0[:, 1]], axis=1))).max() <= 1e-15
    assert L.nmpc_lidar_plant_batch(s._h, 4, Pd.data_ptr(), r4["x"].data_ptr(), Pd.data_ptr(), cfg.n_p, None) == 0      # in place: pose part of p
    torch.cuda.synchronize()
    assert np.array_equal(Pd.cpu().numpy()[:, :3], want) and np.array_equal(Pd.cpu().numpy()[:, 3:], P[:4, 3:])
    assert L.nmpc_lidar_plant_batch(s._h, 4, Pd.data_ptr(), r4["x"].data_ptr(), Pd.data_ptr(), 2, None) == -1


def test_hip_lidar_matches_slsqp_golden(built):
    """the HIP LIDAR solve DIRECTLY against tests/golden/slsqp_lidar.npz (scipy-SLSQP on the restated NLP — an independent solver, "not
    CasADi/IPOPT"), tolerances of tests/test_oracle_lidar.py: objective 1e-6 relative, iterate 2e-4 (SLSQP's own accuracy); four triples with
    aligned bounds — one of them with R = 10 rays, the count the kernel is specialised for — and one with the bounds exactly as the script
    builds them (V4:161-176)."""
    import torch
    import nmpc_amd
    from tests.test_oracle_lidar import _lidar_golden
    n = 0
    for name, cfg, p, w0, ws, fs in _lidar_golden():
        lbx, ubx, _, _ = LR.bounds(cfg)
        s = nmpc_amd.LidarSolver(_product(cfg, max_iter=500), lbx=lbx, ubx=ubx, max_batch=1)
        r = _np(s.solve_batch(p[None], w0[None])); torch.cuda.synchronize()
        assert r["status"][0] == 0 and r["kkt"][0] <= 1e-8, (name, r["status"], r["iters"], r["kkt"])
        assert abs(r["f"][0] - fs) <= 1e-6 * max(1.0, abs(fs)), (name, r["f"][0], fs)
        assert np.abs(r["x"][0] - ws).max() < 2e-4, (name, np.abs(r["x"][0] - ws).max())
        k = LR.kkt_report(cfg, r["x"][0], p, tol_active=1e-4)
        assert k["stat"] < 1e-5 and k["eq"] < 1e-9 and k["bnd"] == 0.0, (name, k)
        print(f"lidar golden {name}: |f - f_slsqp| = {abs(r['f'][0] - fs):.2e}, max|w - w_slsqp| = {np.abs(r['x'][0] - ws).max():.2e}, iters {r['iters'][0]}")
        n += 1
    assert n == 5


def test_lidar_two_long_horizon_handles_and_reproducible_objective(built):
    """(a) The dynamic-LDS limit is an attribute of the kernel function, not of a handle: a handle that needs 86 KB (N = 450) must keep
    solving after a second one with a smaller need (N = 300: 58 KB, below HIP's 64 KB default) has been created and used — solved in
    creation order, then the first one again.  (b) sol['f'] of nmpc_lidar_eval_batch is summed in a fixed order: bit-identical between runs."""
    import torch
    import nmpc_amd
    solvers = []
    for N in (450, 300):
        cfg = LR.LidarConfig(N=N, Nc=N // 2, R=3, aligned_bounds=True)
        lbx, ubx, _, _ = LR.bounds(cfg)
        P, W0 = _batch(cfg, 3, 40 + N)
        solvers.append((cfg, nmpc_amd.LidarSolver(_product(cfg, max_iter=12), lbx=lbx, ubx=ubx, max_batch=3), P, W0))
    for cfg, s, P, W0 in solvers + solvers[:1]:
        r = _np(s.solve_batch(P, W0)); torch.cuda.synchronize()
        ref = O.lidar_solve_batch(cfg, P, W0, max_iter=12)
        assert (r["status"] == ref["status"]).all() and (r["iters"] == ref["iters"]).all(), (cfg.N, r["status"], ref["status"])
        assert np.abs(r["x"] - ref["x"]).max() <= W_TOL
    cfg, s, P, W0 = solvers[0]
    f1, _ = s.eval_batch(P, W0); f2, _ = s.eval_batch(P, W0)
    assert torch.equal(f1, f2)
    cfg4 = LR.lidar_v4()
    lbx, ubx, _, _ = LR.bounds(cfg4)
    P4, W4 = _batch(cfg4, 64, 41)
    s4 = nmpc_amd.LidarSolver(_product(cfg4), lbx=lbx, ubx=ubx, max_batch=64)
    fs = [s4.eval_batch(P4, W4)[0] for _ in range(4)]
    assert all(torch.equal(fs[0], f) for f in fs[1:])
    fo = np.array([LR.objective(cfg4, w, p) for w, p in zip(W4, P4)])
    assert np.abs(fs[0].cpu().numpy() - fo).max() <= 1e-12 * np.abs(fo).max()


def test_lidar_full_size_batch_matches_oracle(built):
    """2048 V4 instances (N=100, Nc=50, the script's bounds as built) — the size class of the bench entry — against the oracle on every one."""
    import torch
    import nmpc_amd
    cfg = LR.lidar_v4()
    B = 2048
    P, W0 = _batch(cfg, B, 23)
    lbx, ubx, _, _ = LR.bounds(cfg)
    r = _np(nmpc_amd.LidarSolver(_product(cfg), lbx=lbx, ubx=ubx, max_batch=B).solve_batch(P, W0)); torch.cuda.synchronize()
    ref = O.lidar_solve_batch(cfg, P, W0)
    conv = ref["status"] == 0
    dw = np.max(np.abs(r["x"] - ref["x"]), axis=1)
    print(f"lidar V4 B={B}: status equal {(r['status'] == ref['status']).mean():.4f}, converged {conv.mean():.4f}, same point {(dw[conv] <= W_TOL).mean():.4f}, "
          f"identical iteration counts {(r['iters'] == ref['iters']).mean():.4f}, max iterations {r['iters'].max()}")
    assert (r["status"] == ref["status"]).mean() >= 0.999 and conv.mean() >= 0.99
    assert (dw[conv] <= W_TOL).mean() >= 0.99 and (r["iters"] == ref["iters"])[conv].mean() >= 0.97


def test_lidar_cold_start_retry(built):
    """the crawling instance of tests/golden/lidar_cold_retry_case.npz (2074 iterations at mu_init = 0.5 without the retry; the oracle takes
    1024 with two retries): the kernel converges it to the oracle's point in no more iterations.  The crawl is a knife edge: the kernel's
    evaluation order (symmetric Riccati form, product form of the barrier sum) differs from the oracle's in the last bits, and since round 3
    the kernel leaves the crawl by itself after 456 iterations — when it does need the retry, its count must be the oracle's."""
    import os
    import torch
    import nmpc_amd
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_cold_retry_case.npz"))
    cfg = LR.lidar_v4()
    lbx, ubx, _, _ = LR.bounds(cfg)
    s = nmpc_amd.LidarSolver(_product(cfg, max_iter=2000), lbx=lbx, ubx=ubx, max_batch=1)
    r = _np(s.solve_batch(g["p"], g["w0"])); torch.cuda.synchronize()
    ref = O.lidar_solve_batch(cfg, g["p"], g["w0"], max_iter=2000, lbx=lbx, ubx=ubx)
    print("hip", r["status"], r["iters"], "oracle", ref["status"], ref["iters"])
    assert r["status"][0] == 0 and ref["status"][0] == 0
    it, it_ref = int(r["iters"][0]), int(ref["iters"][0])
    assert it <= it_ref + 3 and 1000 <= it_ref <= 1100
    assert it < 500 or abs(it - it_ref) <= 3      # 500 = NMPC_COLD_RETRY_ITERS: past it the retry ran, and must have run like the oracle's
    assert np.max(np.abs(r["x"] - ref["x"])) <= W_TOL


def test_lidar_line_search_watchdog(built):
    """tests/golden/lidar_watchdog_cases.npz: the bench batch's three long solves (175 / 154 / 145 iterations without the watchdog of the
    line search, include/nmpc_constants.h) and the five longest that remain: the kernel converges all of them to the oracle's point, in the
    oracle's iteration count (at most 61) give or take the late forks of a chaotic solve."""
    import os
    import torch
    import nmpc_amd
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_watchdog_cases.npz"))
    cfg = LR.lidar_v4()
    lbx, ubx, _, _ = LR.bounds(cfg)
    s = nmpc_amd.LidarSolver(_product(cfg, max_iter=2000), lbx=lbx, ubx=ubx, max_batch=len(g["p"]))
    r = _np(s.solve_batch(g["p"], g["w0"])); torch.cuda.synchronize()
    ref = O.lidar_solve_batch(cfg, g["p"], g["w0"], max_iter=2000, lbx=lbx, ubx=ubx)
    print("hip", r["iters"], "oracle", ref["iters"], "without the watchdog", g["iters_without"])
    assert (r["status"] == 0).all() and (ref["status"] == 0).all()
    assert r["iters"].max() <= 70 and (r["iters"] == ref["iters"]).mean() >= 0.75, (r["iters"], ref["iters"])
    assert np.max(np.abs(r["f"] - ref["f"]) / np.abs(ref["f"])) < 1e-8
    same = r["iters"] == ref["iters"]
    assert np.max(np.abs(r["x"][same] - ref["x"][same])) <= W_TOL
