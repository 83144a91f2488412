"""Development aid (GPU box): solves/s of the tracking solve (nmpc_solve_batch_ref, track_col_kernel) with constant reference rows against
the plain solve of the same inputs, on the benchmark's configurations.   python tools/track_rate.py [--out profiles/current/track_rate.json]

With every reference row equal to the goal the two calls are bit-identical (include/nmpc.h), so they make the same iterations and the ratio
of their rates is the cost of reading the reference's rows from device memory instead of the goal from LDS.  The sibling call is
nmpc_solve_batch_obs with the config's own obstacles as a static per-instance field where the configuration has obstacle rows (the same field
instantiation the tracking kernel is built from), nmpc_solve_batch where it has none.  The reference is passed per stage (S = N).

One process.  Per shape both sides are warmed, then they alternate for --repeats windows of at least --window seconds of work each, a
synchronise at the end of every window; a side's time is the median of its windows, its spread (max - min) / median.  Both sides go through
the C ABI with outputs allocated once; their outputs are compared bit for bit after the timing."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import nmpc_amd
import bench

SHAPES = [("two", 4096), ("six", 4096), ("composite", 1024)]      # (bench workload, B): two and six robots N = 20, six robots among eight obstacles

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "current", "track_rate.json"))
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

rows = []
for name, B in SHAPES:
    cfg, _, P, W0 = bench.make_batch(name, 0, B)
    s = nmpc_amd.NmpcSolver(cfg, max_batch=B)
    K = len(cfg.obstacles)
    p = s._dev(P, (B, s.n_p)); w0 = s._dev(W0, (B, s.n_var))
    ref = p[:, cfg.nx:].reshape(B, 1, cfg.nx).expand(B, cfg.N, cfg.nx).contiguous()
    fld = torch.tensor(cfg.obstacles, dtype=torch.float64, device=s.device).reshape(1, 1, K, 3).expand(B, 1, K, 3).contiguous() if K else None
    out = {k: dict(x=torch.empty((B, s.n_var), dtype=torch.float64, device=s.device), f=torch.empty(B, dtype=torch.float64, device=s.device),
                   kkt=torch.empty(B, dtype=torch.float64, device=s.device), status=torch.empty(B, dtype=torch.int32, device=s.device),
                   iters=torch.empty(B, dtype=torch.int32, device=s.device)) for k in ("track", "plain")}
    st = s._stream()

    def track():
        o = out["track"]
        rc = s.lib.nmpc_solve_batch_ref(s._h, B, p.data_ptr(), ref.data_ptr(), cfg.N, fld.data_ptr() if K else None, 1 if K else 0, w0.data_ptr(), o["x"].data_ptr(),
                                        o["f"].data_ptr(), o["status"].data_ptr(), o["iters"].data_ptr(), o["kkt"].data_ptr(), None, None, st)
        assert rc == 0, rc

    def plain():
        o = out["plain"]
        if K:
            rc = s.lib.nmpc_solve_batch_obs(s._h, B, p.data_ptr(), fld.data_ptr(), 1, w0.data_ptr(), o["x"].data_ptr(), o["f"].data_ptr(), o["status"].data_ptr(),
                                            o["iters"].data_ptr(), o["kkt"].data_ptr(), None, st)
        else:
            rc = s.lib.nmpc_solve_batch(s._h, B, p.data_ptr(), w0.data_ptr(), o["x"].data_ptr(), o["f"].data_ptr(), o["status"].data_ptr(), o["iters"].data_ptr(),
                                        o["kkt"].data_ptr(), st)
        assert rc == 0, rc

    def window(f, n):
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(n):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n

    reps = {}
    for key, f in (("track", track), ("plain", plain)):      # warm, then the number of calls that fills a window
        window(f, 2)
        reps[key] = max(1, int(np.ceil(args.window / window(f, 3))))
    t = {"track": [], "plain": []}
    for _ in range(args.repeats):
        for key, f in (("track", track), ("plain", plain)):
            t[key].append(window(f, reps[key]))
    same = all(torch.equal(out["track"][k].view(torch.int64 if out["track"][k].dtype == torch.float64 else torch.int32),
                           out["plain"][k].view(torch.int64 if out["plain"][k].dtype == torch.float64 else torch.int32)) for k in out["track"])
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    v, code = nmpc_amd._lib.CDebugVariant(), C.c_int32(0)
    rc = s.lib.nmpc_debug_track_variant_of_config(C.byref(s._ccfg), None, torch.cuda.get_device_properties(s.device).multi_processor_count, B, 0, int(K > 0),
                                                  C.byref(v), C.byref(code))
    assert rc == 0, rc
    row = dict(workload=name, m=cfg.m, N=cfg.N, K=K, B=B, bit_identical=bool(same), status_0=int((out["plain"]["status"] == 0).sum()),
               mean_iters=float(out["plain"]["iters"].double().mean()), track_solves_per_s=B / med["track"], plain_solves_per_s=B / med["plain"],
               ratio=med["plain"] / med["track"], track_spread=spread["track"], plain_spread=spread["plain"], calls_per_window=reps,
               track_variant=[v.kernel, v.m, v.thb, v.flags, v.threads], lds_bytes_per_instance=int(v.lds_bytes),
               track_windows_ms=[1e3 * x for x in t["track"]], plain_windows_ms=[1e3 * x for x in t["plain"]])
    rows.append(row)
    print("%-9s m = %2d N = %2d K = %d B = %4d: tracking %9.0f solves/s (spread %.1f %%), plain %9.0f solves/s (spread %.1f %%), ratio %.3f, LDS %d B per instance, "
          "bit-identical %s" % (name, cfg.m, cfg.N, K, B, row["track_solves_per_s"], 100 * spread["track"], row["plain_solves_per_s"], 100 * spread["plain"],
                                row["ratio"], row["lds_bytes_per_instance"], same), flush=True)
    del s
rec = dict(device=torch.cuda.get_device_name(0), library=nmpc_amd._lib.load().nmpc_version().decode(), window_s=args.window, repeats=args.repeats, rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
