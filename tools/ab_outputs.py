"""Development aid (GPU box): bit-identity of two library builds.  One process per library:
    NMPC_SO=<a.so> python tools/ab_outputs.py a.npz          every output array of the fixed case list below, solved on that library
    NMPC_SO=<a.so> python tools/ab_outputs.py a.npz sens     only the named groups of the list: solve, lidar, sens
    NMPC_SO=<b.so> python tools/ab_outputs.py b.npz
    python tools/ab_outputs.py --compare a.npz b.npz         lists the arrays whose bit patterns differ (exit status 1 if any)
    python tools/ab_outputs.py --compare-dumps dirA dirB     the same for two `bench.py --dump-outputs` directories
Cases: the ten shapes of tests/test_gpu_phase_passes.py (plain call and with multipliers), the elastic / cold-retry fixtures of the composite
on every pin (1 .. 5: they walk the barrier restarts, both cold retries and the elastic phase of all three swarm kernels), the moving-obstacle
rescue fixtures (per-instance field) on pins 3, 4, 5, nmpc_solve_batch_duals on the six-robot bench batch, every kernel-1 and kernel-2 row of
tests/kernel_variants.TABLE by its own recipe, and the LIDAR kernel: one recipe of tests/lidar_variants.TABLE per instantiation and
LIDAR_BENCH_PICK of its bench batch; and the sensitivity calls on the constructed points of every row of tests/sens_points.SENS_TABLE (N = 2 .. 12,
four to six points a row): nmpc_sens_batch (the gains of every stage and dw), nmpc_sens_adjoint_batch (pbar, and obsbar on the rows with a
per-instance field), nmpc_sens_update_batch (dw, alpha) and nmpc_sens_update_batch_duals, with the seeded cotangent, dobs and rhs of the GPU
tests and the verdicts of each.  After each swarm solve the handle's workspace is recorded too, as one sha256 per instance (`<case>/ws`):
a changed scratch value shows even where no output moved.  NaN payloads count: arrays are compared as raw bytes."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(a, b):
    """names of the arrays of two {name: array} mappings that are missing on one side or differ in dtype, shape or bytes"""
    bad = sorted(set(a) ^ set(b))
    for k in sorted(set(a) & set(b)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    return bad


def load_dumps(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def workspace_hashes(s, B):
    """sha256 of the workspace of each of the first B instances of a solver's handle, [B, 32] uint8"""
    n = s.lib.nmpc_debug_workspace(s._h, 0, None, 0, None)
    buf = np.zeros(n)
    out = np.zeros((B, 32), dtype=np.uint8)
    for b in range(B):
        s.lib.nmpc_debug_workspace(s._h, b, buf.ctypes.data_as(C.c_void_p), n, None)
        out[b] = np.frombuffer(hashlib.sha256(buf.tobytes()).digest(), dtype=np.uint8)
    return out


def record(out, name, s, P, W, ws=True, **kw):
    import torch
    r = s.solve_batch(P, W, **kw)
    torch.cuda.synchronize()
    for k, v in r.items():
        out["%s/%s" % (name, k)] = v.cpu().numpy()
    if ws:
        out[name + "/ws"] = workspace_hashes(s, len(P))
    print("%-52s status %s iterations %d..%d" % (name, sorted(set(out[name + "/status"].tolist())), out[name + "/iters"].min(), out[name + "/iters"].max()), flush=True)


# Instances of the LIDAR bench batch (lidar_bench_batch below, 4096 instances), chosen on the CPU from the oracle's per-iteration trace
# (NMPC_LIDAR_ORACLE_TRACE): the watchdog of the line search fires, once or twice, in the first LIDAR_WATCHDOG of them (ten successive
# shortened steps, then a step of fraction-to-the-boundary length >= 0.5 taken as it is; they are among the 55 longest solves of the batch,
# 45 .. 60 iterations); the rest are the first sixteen instances of the batch.
# Traced were the 64 longest solves of the batch, not all 4096: none of those takes a barrier restart on the oracle (no five successive steps
# below 1e-10), so none is picked for one; whether a shorter solve of the batch does is not known.  The restart ladder of the LIDAR kernel is
# walked by its parity tests.
LIDAR_BENCH_PICK = [1985, 88, 1345, 222, 899, 3625, 2352, 141, 2303, 2883, 3786, 3853, 3584, 3316, 1905, 3005, 976, 4011, 3643, 2600, 1793, 2498, 64, 2518, 1998, 1524, 232, 3899, 1437, 3670, 1898, 1922, 3949, 3716, 737, 2270, 980, 996, 1314, 3287, 2060, 2050, 367, 1283, 238, 806, 2609, 733, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
LIDAR_WATCHDOG = 48


def lidar_bench_batch(B=4096):
    """the LIDAR batch of bench.py --full and tools/bench_lidar.py (same generator and seed), with the scan made on the CPU"""
    from oracle import lidar_ref as LR
    lc = LR.lidar_v4()
    rng = np.random.Generator(np.random.PCG64(20210146))
    P, W = [], []
    for _ in range(B):
        pose = np.array([rng.uniform(0.0, 0.15), rng.uniform(0.0, 0.15), rng.uniform(0.4, 1.1)])
        world = [(float(rng.uniform(0.8, 2.6)), float(rng.uniform(0.3, 2.4)), float(rng.uniform(0.15, 0.3))) for _ in range(3)]
        scan = LR.scan_of_world(pose, world, lc.R)
        P.append(LR.make_p(lc, pose, np.array([3.0, 2.5, 0.0]) + rng.uniform(-0.3, 0.3, 3), scan)); W.append(LR.cold_start(lc, np.concatenate([pose, scan])))
    return lc, np.stack(P), np.stack(W)


def run_lidar(out):
    import nmpc_amd
    from oracle import lidar_ref as LR
    from tests import lidar_variants as LV
    from tests.test_gpu_lidar import _product
    from tests.test_gpu_lidar_variants import _two_wave_threshold

    def solver(cfg, max_iter, B):
        lbx, ubx, _, _ = LR.bounds(cfg)
        return nmpc_amd.LidarSolver(_product(cfg, max_iter=max_iter), lbx=lbx, ubx=ubx, max_batch=B)
    for inst in ((-1, 1), (10, 1), (10, 2)):      # the first recipe of each instantiation with a horizon of nine stages or more
        r = next(r for r in LV.TABLE if r.inst == inst and r.N >= 8 and r.R > 0)
        B = _two_wave_threshold() + 1 if r.B is None else r.B
        cfg, P, W = LV.inputs(r, B)
        record(out, "lidar_" + LV.row_id(r), solver(cfg, r.max_iter, B), P, W, ws=False)
    lc, P, W = lidar_bench_batch()
    P, W = P[LIDAR_BENCH_PICK], W[LIDAR_BENCH_PICK]
    record(out, "lidar_bench_pick", solver(lc, 2000, len(P)), P, W, ws=False)


def run_sens(out):
    import nmpc_amd
    from tests import helpers as Hh
    from tests import sens_adjoint_ref as AR
    from tests import sens_points as SP
    from tests import sens_update_ref as UR
    stack = lambda xs: None if xs[0] is None else np.stack(xs)
    for r in SP.SENS_TABLE:
        pts = SP.points(r); n = len(pts)
        s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(r.cfg, max_iter=10, pair_rows=r.cfg.pair_rows), max_batch=2 * n + 2)      # the handle of the GPU tests
        a = [np.stack([getattr(pt, k) for pt in pts]) for k in ("p", "w", "lam_g", "lam_x")]
        obs = np.stack([pt.obs for pt in pts]) if r.field else None      # an "own" row calls with the handle's field
        dp = np.stack([pt.dp for pt in pts])
        dobs, rhs = stack([UR.row_dobs(r, k) for k in range(n)]), np.stack([UR.row_rhs(r, k) for k in range(n)])
        calls = dict(sens=s.sens_batch(*a, dp=dp, gains="N", obstacles=obs),
                     adjoint=s.sens_adjoint_batch(*a, np.stack([AR.row_cotangent(r, k) for k in range(n)]), obstacles=obs),
                     update=s.sens_update_batch(*a, dp=dp, dobs=dobs, rhs=rhs, obstacles=obs),
                     update_duals=s.sens_update_batch(*a, dp=dp, dobs=dobs, rhs=rhs, obstacles=obs, want_duals=True))
        for call, res in calls.items():
            for k, v in res.items():
                if v is not None:
                    out["sens_%s/%s/%s" % (SP.row_id(r), call, k)] = v.cpu().numpy()
        print("%-52s info %s" % ("sens_" + SP.row_id(r), sorted({int(i) for c in calls for i in out["sens_%s/%s/info" % (SP.row_id(r), c)]})), flush=True)


def run(path, groups=("solve", "lidar", "sens")):
    out = {}
    if "solve" in groups:
        run_solve(out)
    if "lidar" in groups:
        run_lidar(out)
    if "sens" in groups:
        run_sens(out)
    import nmpc_amd
    np.savez_compressed(path, **out)
    print("%d arrays of %s -> %s" % (len(out), nmpc_amd._lib.SO_PATH, path))


def run_solve(out):
    import nmpc_amd
    from tests import helpers as Hh
    from tests import moving_obstacles_ref as MO
    from tests import test_gpu_phase_passes as PP
    for name in PP.CASES:
        cfg, P, W0, F = PP.case_inputs(name)
        for duals in (False, True):
            s = nmpc_amd.NmpcSolver(PP._product_cfg(cfg), max_batch=PP.B + 3, kernel=PP.CASES[name][5])
            record(out, name + ("_duals" if duals else ""), s, P, W0, obstacles=F, want_duals=duals)
    oc = Hh.bench_batch("composite", 1)[0]
    gold = os.path.join(ROOT, "tests", "golden")
    for f in ("elastic_cases", "cold_retry_cases", "cold_retry_cases2"):
        z = np.load(os.path.join(gold, f + ".npz"))
        for pin in (1, 2, 3, 4, 5):
            s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(oc, max_iter=2000), max_batch=len(z["p"]), kernel=pin)
            record(out, "%s_pin%d" % (f, pin), s, z["p"], z["w"])
    z = np.load(os.path.join(gold, "moving_obstacle_cases.npz"))
    for pin in (3, 4, 5):
        s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(MO.team_cfg(6, 25, 8), max_iter=2000), max_batch=len(z["p"]), kernel=pin)
        record(out, "moving_obstacle_cases_pin%d" % pin, s, z["p"], z["w"], obstacles=z["obs"])
    oc, B, P, W0 = Hh.bench_batch("six", 64)
    record(out, "bench_six_64_duals", nmpc_amd.NmpcSolver(Hh.to_product_cfg(oc, max_iter=2000), max_batch=B), P, W0, want_duals=True)
    from tests import kernel_variants as KV
    for r in KV.TABLE:
        if r.row[0] in (1, 2):      # the HBM-resident and the element-per-lane kernel: short cold solves at the recipes' batch sizes
            cfg, P, W0, F = KV.inputs(r)
            s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=r.max_iter), max_batch=r.B, kernel=r.pin)
            assert int(s.kernel_for_batch(r.B)) == r.row[0], (r.row, s.kernel_for_batch(r.B))
            record(out, KV.row_id(r), s, P, W0)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"] or sys.argv[1:2] == ["--compare-dumps"]:
        a, b = (load_dumps(p) for p in sys.argv[2:4]) if sys.argv[1] == "--compare-dumps" else (dict(np.load(p)) for p in sys.argv[2:4])
        bad = compare(a, b)
        print("%d arrays compared, %d differ%s" % (len(set(a) | set(b)), len(bad), (": " + ", ".join(bad)) if bad else ""))
        sys.exit(1 if bad else 0)
    run(sys.argv[1], *([tuple(sys.argv[2:])] if sys.argv[2:] else []))
