"""Development aid (GPU box): cost of the plan sensitivities (nmpc_sens_batch) next to the solve that feeds them, on the headline batch
(six robots, N = 20, B = 4096).

The batch is solved once with want_duals=True; then, inside every repetition, the plain solve launch and the sensitivity call on that solve's
own output in its four shapes (gains of stage 0 / of every stage, with and without dw) alternate, each launch timed with HIP events on the
launch stream.

    python tools/bench_sens.py [reps]      -> one line on stderr, one JSON line on stdout
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
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 5
    B = 4096
    cfg, _, P, W0 = bench.make_batch("six", 0, B)
    s = nmpc_amd.NmpcSolver(cfg, max_batch=B)
    dP, dW = torch.as_tensor(P, device="cuda"), torch.as_tensor(W0, device="cuda")
    r = s.solve_batch(dP, dW, want_duals=True)
    dp = torch.zeros_like(dP)
    dp[:, : cfg.nx] = 1e-2      # the advanced-step shape: a measured state off the predicted one, the goal as it was
    sens = lambda gains, with_dw: (lambda: s.sens_batch(dP, r["x"], r["lam_g"], r["lam_x"], dp=dp if with_dw else None, gains=gains))      # noqa: E731
    variants = {"plain_solve": lambda: s.solve_batch(dP, dW), "gains1": sens(1, False), "gains1_dw": sens(1, True), "gainsN": sens("N", False),
                "gainsN_dw": sens("N", True)}
    res = {v: timed(f)[1] for v, f in variants.items()}      # warm-up (code objects, allocator)
    assert all(torch.equal(res["plain_solve"][k], r[k]) for k in ("x", "f", "status", "iters", "kkt"))      # the calls in between leave the solve as it was
    assert torch.equal(res["gains1"]["gains"][:, 0], res["gainsN_dw"]["gains"][:, 0]) and torch.equal(res["gains1_dw"]["dw"], res["gainsN_dw"]["dw"])
    ms = {v: [] for v in variants}
    for _ in range(reps):
        for v, f in variants.items():
            ms[v].append(timed(f)[0])
    info, ok = res["gainsN_dw"]["info"], (r["status"] == 0)
    out = {"library": nmpc_amd._lib.load().nmpc_version().decode(), "reps": reps, "B": B, "kernel": s.kernel_for_batch(B),
           "converged_frac": float(ok.double().mean()), "info_counts": torch.bincount(info.long(), minlength=3).tolist(),
           "info_ok_of_converged": float((info[ok] == 0).double().mean()), "gains_bytes": int(res["gainsN_dw"]["gains"].numel() * 8)}
    base = float(np.median(ms["plain_solve"]))
    for v, t in ms.items():
        out[v] = {"ms_median": float(np.median(t)), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "vs_plain_solve": float(np.median(t)) / base}
    print("six robots B=%d: " % B + ", ".join("%s %.3f ms [%.3f, %.3f]" % (v, out[v]["ms_median"], out[v]["ms_min"], out[v]["ms_max"]) for v in variants)
          + "; gains S=N + dw at %.1f %% of the plain solve launch; info %s" % (100.0 * out["gainsN_dw"]["vs_plain_solve"], out["info_counts"]),
          file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
