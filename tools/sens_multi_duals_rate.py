"""Development aid (GPU box): one call of nmpc_sens_update_batch_multi_duals at D directions against D calls of nmpc_sens_update_batch_duals, on
solved points of the benchmark's configurations.   python tools/sens_multi_duals_rate.py [--out profiles/current/sens_multi_duals_rate.json]

The method of tools/sens_multi_rate.py, the same shapes and D values.  One process.  Per shape: the batch is solved with multipliers, both
sides are warmed, then the two sides alternate for --repeats windows of at least --window seconds of work each, a synchronise at the end of
every window; a side's time is the median of its windows, its spread (max - min) / median.  The directions are the first D unit vectors of p
(D = n_p: the Jacobians of the plan and of its multipliers).  Both sides go through the C ABI with outputs allocated once and write every output
they have.  A third side, nmpc_sens_update_batch_multi alone, alternates with them: the difference to the first is what the multipliers cost."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import nmpc_amd
import bench

SHAPES = [("six", 4096, (1, 12, 36)), ("ten", 512, (60,)), ("two", 4096, (12,))]      # (bench workload, B, the D values); n_p = 36, 60, 12

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "current", "sens_multi_duals_rate.json"))
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

rows = []
for name, B, Ds in SHAPES:
    cfg, _, P, W0 = bench.make_batch(name, 0, B)
    s = nmpc_amd.NmpcSolver(cfg, max_batch=B)
    sol = s.solve_batch(P, W0, want_duals=True)
    p = s._dev(P, (B, s.n_p)); w, lg, lx = sol["x"], sol["lam_g"], sol["lam_x"]
    info = torch.empty(B, dtype=torch.int32, device=s.device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=s.device)
    for D in Ds:
        dp = torch.eye(s.n_p, dtype=torch.float64, device=s.device)[:D].expand(B, D, s.n_p).contiguous()
        cols = [dp[:, d].contiguous() for d in range(D)]
        dwm, alm, dgm, dxm, dpm, adm = new(B, D, s.n_var), new(B, D), new(B, D, s.n_g), new(B, D, s.n_var), new(B, D, s.n_p), new(B, D)
        dws, als, dgs, dxs, ads = new(B, s.n_var), new(B), new(B, s.n_g), new(B, s.n_var), new(B)
        st = s._stream()

        def multi():
            rc = s.lib.nmpc_sens_update_batch_multi_duals(s._h, B, D, p.data_ptr(), None, 0, w.data_ptr(), lg.data_ptr(), lx.data_ptr(), dp.data_ptr(), None, None,
                                                          dwm.data_ptr(), alm.data_ptr(), dgm.data_ptr(), dxm.data_ptr(), dpm.data_ptr(), adm.data_ptr(), info.data_ptr(), st)
            assert rc == 0, rc

        def single():
            for c in cols:
                rc = s.lib.nmpc_sens_update_batch_duals(s._h, B, p.data_ptr(), None, 0, w.data_ptr(), lg.data_ptr(), lx.data_ptr(), c.data_ptr(), None, None,
                                                        dws.data_ptr(), als.data_ptr(), dgs.data_ptr(), dxs.data_ptr(), ads.data_ptr(), info.data_ptr(), st)
                assert rc == 0, rc

        def primal():
            rc = s.lib.nmpc_sens_update_batch_multi(s._h, B, D, p.data_ptr(), None, 0, w.data_ptr(), lg.data_ptr(), lx.data_ptr(), dp.data_ptr(), None, None,
                                                    dwm.data_ptr(), alm.data_ptr(), info.data_ptr(), st)
            assert rc == 0, rc

        def window(f, n):
            torch.cuda.synchronize(); t = time.perf_counter()
            for _ in range(n):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n

        sides = (("multi", multi), ("single", single), ("primal", primal))
        reps = {}
        for key, f in sides:      # warm, then the number of calls that fills a window
            window(f, 2)
            reps[key] = max(1, int(np.ceil(args.window / window(f, 3))))
        ok = int((info == 0).sum())
        t = {key: [] for key, _ in sides}
        for _ in range(args.repeats):
            for key, f in sides:
                t[key].append(window(f, reps[key]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
        row = dict(workload=name, m=cfg.m, N=cfg.N, B=B, D=D, n_p=s.n_p, verdict_0=ok, status_0=int((sol["status"] == 0).sum()),
                   multi_ms=1e3 * med["multi"], single_ms=1e3 * med["single"], primal_ms=1e3 * med["primal"], ratio=med["single"] / med["multi"],
                   duals_ms=1e3 * (med["multi"] - med["primal"]), multi_spread=spread["multi"], single_spread=spread["single"], primal_spread=spread["primal"],
                   calls_per_window=reps, **{k + "_windows_ms": [1e3 * v for v in t[k]] for k in t})
        rows.append(row)
        print("%-4s m = %2d N = %2d B = %4d D = %2d: one call %8.3f ms (spread %.1f %%; without multipliers %8.3f ms), %2d calls %8.3f ms (spread %.1f %%), ratio %.2f, verdict 0 on %d" % (
            name, cfg.m, cfg.N, B, D, row["multi_ms"], 100 * spread["multi"], row["primal_ms"], D, row["single_ms"], 100 * spread["single"], row["ratio"], ok), flush=True)
    del s
rec = dict(device=torch.cuda.get_device_name(0), library=nmpc_amd._lib.load().nmpc_version().decode(), window_s=args.window, repeats=args.repeats, rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
