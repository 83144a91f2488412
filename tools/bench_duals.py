"""Development aid (GPU box): cost of returning the multipliers (nmpc_solve_batch_duals) and of the device-side KKT certificate (nmpc_kkt_batch)
on the headline batch (six robots, N = 20, B = 4096).

The same batch with and without want_duals — identical iterates, checked — alternating inside every repetition, each launch timed with HIP
events on the launch stream; then nmpc_kkt_batch on the solve's own output.

    python tools/bench_duals.py [reps]      -> one line on stderr, one JSON line on stdout
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    B = 4096
    cfg, _, P, W0 = bench.make_batch("six", 0, B)
    s = nmpc_amd.NmpcSolver(cfg, max_batch=B)
    dP, dW = torch.as_tensor(P, device="cuda"), torch.as_tensor(W0, device="cuda")
    variants = {"plain": lambda: s.solve_batch(dP, dW), "want_duals": lambda: s.solve_batch(dP, dW, want_duals=True)}
    res = {v: timed(f)[1] for v, f in variants.items()}      # warm-up (code objects, allocator)
    assert all(torch.equal(res["plain"][k], res["want_duals"][k]) for k in ("x", "f", "status", "iters", "kkt"))
    ms = {v: [] for v in variants}
    for _ in range(reps):
        for v, f in variants.items():
            ms[v].append(timed(f)[0])
    r = res["want_duals"]
    kkt = lambda: s.kkt_batch(dP, r["x"], r["lam_g"], r["lam_x"])      # noqa: E731
    cert = timed(kkt)[1]
    kms = [timed(kkt)[0] for _ in range(reps)]
    ok = (r["status"] == 0)
    out = {"library": nmpc_amd._lib.load().nmpc_version().decode(), "reps": reps, "B": B, "kernel": s.kernel_for_batch(B),
           "converged_frac": float(ok.double().mean()), "worst_stat_converged": float(cert[ok][:, 0].max()), "worst_compl_converged": float(cert[ok][:, 4].max())}
    base = float(np.median(ms["plain"]))
    for v, t in list(ms.items()) + [("kkt_batch", kms)]:
        out[v] = {"ms_median": float(np.median(t)), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "vs_plain": float(np.median(t)) / base}
    print("six robots B=%d: " % B + ", ".join("%s %.3f ms [%.3f, %.3f]" % (v, out[v]["ms_median"], out[v]["ms_min"], out[v]["ms_max"]) for v in ("plain", "want_duals", "kkt_batch"))
          + "; worst stat %.2e compl %.2e over the converged %.4f of the batch" % (out["worst_stat_converged"], out["worst_compl_converged"], out["converged_frac"]),
          file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
