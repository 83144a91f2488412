"""Development aid (GPU box): cost of the per-instance obstacle field (nmpc_solve_batch_obs) on the composite (six robots, eight obstacles, N=25).

At B = 1024 (the library's latency shape) and B = 4096 (throughput), three variants of the same batch: config obstacles (nmpc_solve_batch),
per-instance S = 1 with every instance holding the config field, S = N with that entry repeated.  All three do identical iterations (checked:
identical iterates and iteration counts), so a difference is the cost of the data path alone.  The variants alternate inside every repetition;
each launch is timed with HIP events on the launch stream.  One heterogeneous batch (16 fields, instances clear of their own field) is timed
for context (other problems: not comparable launch for launch).

    python tools/bench_obstacles.py [reps]      -> one line per shape on stderr, one JSON line on stdout
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import nmpc_amd  # noqa: E402


def timed(solver, dP, dW, obstacles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = solver.solve_batch(dP, dW, obstacles=obstacles)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"library": nmpc_amd._lib.load().nmpc_version().decode(), "reps": reps, "shapes": {}}
    for B in (1024, 4096):
        cfg, _, P, W0 = bench.make_batch("composite", 0, B)
        K, N = len(cfg.obstacles), cfg.N
        s = nmpc_amd.NmpcSolver(cfg, max_batch=B)
        dP, dW = torch.as_tensor(P, device="cuda"), torch.as_tensor(W0, device="cuda")
        field = np.array(cfg.obstacles)
        variants = {"config": None,
                    "S=1": torch.as_tensor(np.broadcast_to(field, (B, K, 3)).copy(), device="cuda"),
                    "S=N": torch.as_tensor(np.broadcast_to(field, (B, N, K, 3)).copy(), device="cuda")}
        ms = {v: [] for v in variants}
        res = {}
        for v, o in variants.items():      # warm-up (code objects, allocator)
            _, res[v] = timed(s, dP, dW, o)
        ref = res["config"]
        for v in ("S=1", "S=N"):
            assert torch.equal(res[v]["x"], ref["x"]) and torch.equal(res[v]["iters"], ref["iters"]), v
        for _ in range(reps):
            for v, o in variants.items():
                ms[v].append(timed(s, dP, dW, o)[0])
        # heterogeneous batch: 16 fields, each instance drawn clear of its own field (bench.instance)
        rng = np.random.Generator(np.random.PCG64(20210141 + 40))
        fields = [[(float(x), float(y), float(r)) for x, y, r in zip(rng.uniform(-1.5, 1.5, K), rng.uniform(-1.5, 1.5, K), rng.uniform(0.125, 0.2, K))]
                  for _ in range(16)]
        Ph, Fh = [], []
        for b in range(B):
            c = nmpc_amd.six_robots_eight_obstacles(N=N, obstacles=fields[b % 16])
            Ph.append(bench.instance(rng, c)); Fh.append(fields[b % 16])
        dPh = torch.as_tensor(np.stack(Ph), device="cuda")
        dWh = torch.as_tensor(np.stack([nmpc_amd.cold_start(cfg, p[: cfg.nx]) for p in Ph]), device="cuda")
        dFh = torch.as_tensor(np.array(Fh), device="cuda")
        timed(s, dPh, dWh, dFh)
        hms = []
        for _ in range(reps):
            t, rh = timed(s, dPh, dWh, dFh)
            hms.append(t)
        row = {"kernel": s.kernel_for_batch(B), "mean_iters": float(ref["iters"].double().mean()), "max_iters": int(ref["iters"].max())}
        base = float(np.median(ms["config"]))
        for v, t in ms.items():
            med = float(np.median(t))
            row[v] = {"ms_median": med, "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "solves_per_s": B / med * 1e3, "vs_config": med / base}
        row["heterogeneous_16_fields"] = {"ms_median": float(np.median(hms)), "ms_min": float(np.min(hms)), "ms_max": float(np.max(hms)),
                                          "solves_per_s": B / float(np.median(hms)) * 1e3, "mean_iters": float(rh["iters"].double().mean()),
                                          "max_iters": int(rh["iters"].max()), "converged_frac": float((rh["status"] == 0).double().mean())}
        out["shapes"]["B=%d" % B] = row
        print("B=%d kernel %d: " % (B, row["kernel"]) + ", ".join("%s %.2f ms [%.2f, %.2f] (x%.3f)" % (v, row[v]["ms_median"], row[v]["ms_min"], row[v]["ms_max"],
                                                                                                     row[v]["vs_config"]) for v in ms)
              + "; heterogeneous %.2f ms, mean iterations %.2f vs %.2f" % (row["heterogeneous_16_fields"]["ms_median"], row["heterogeneous_16_fields"]["mean_iters"],
                                                                       row["mean_iters"]), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
