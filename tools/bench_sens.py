"""Development aid (GPU box): cost of the plan sensitivities (nmpc_sens_batch) next to the solve that feeds them, on the headline batch
(six robots, N = 20, B = 4096).

The batch is solved once with want_duals=True; then, inside every repetition, the plain solve launch, the sensitivity call on that solve's
own output in its four shapes (gains of stage 0 / of every stage, with and without dw) and the adjoint call (nmpc_sens_adjoint_batch, pbar)
alternate, each launch timed with HIP events on the launch stream; so do the forward plan update (nmpc_sens_update_batch: dp alone with and
without alpha, and with the multiplier updates of nmpc_sens_update_batch_duals behind it) and its yardstick, nmpc_sens_batch(dp, gains=None).  The adjoint's obstacle cotangent needs a per-instance field: a second
handle (six robots, eight obstacles, N = 20, the config's field given per instance) is solved the same way and its plain solve, the
forward call, the adjoint and the update (dp and dobs) with a static ([B, K, 3]) and a per-stage ([B, N, K, 3]) field alternate in the same
repetitions.

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
    wbar = torch.as_tensor(np.random.default_rng(0).normal(size=(B, cfg.n_var)), device="cuda")
    variants["adjoint"] = lambda: s.sens_adjoint_batch(dP, r["x"], r["lam_g"], r["lam_x"], wbar)
    variants["dw_only"] = sens(None, True)      # the yardstick of the update: the same dw from nmpc_sens_batch
    variants["update"] = lambda: s.sens_update_batch(dP, r["x"], r["lam_g"], r["lam_x"], dp=dp)
    variants["update_no_alpha"] = lambda: s.sens_update_batch(dP, r["x"], r["lam_g"], r["lam_x"], dp=dp, want_alpha=False)
    variants["update_duals"] = lambda: s.sens_update_batch(dP, r["x"], r["lam_g"], r["lam_x"], dp=dp, want_duals=True)
    # the obstacle cotangent: six robots among eight obstacles, every instance holding the config's field, static and per stage
    ocfg = nmpc_amd.six_robots_eight_obstacles(N=cfg.N, obstacles=bench.make_batch("composite", 0, 1)[0].obstacles)
    ocfg.max_iter = cfg.max_iter
    rng = np.random.Generator(np.random.PCG64(20210141))
    Po = np.stack([bench.instance(rng, ocfg) for _ in range(B)])
    so = nmpc_amd.NmpcSolver(ocfg, max_batch=B)
    dPo = torch.as_tensor(Po, device="cuda")
    dWo = torch.as_tensor(np.stack([nmpc_amd.cold_start(ocfg, q[: ocfg.nx]) for q in Po]), device="cuda")
    K = len(ocfg.obstacles)
    f1 = torch.as_tensor(np.broadcast_to(np.array(ocfg.obstacles), (B, K, 3)).copy(), device="cuda")
    fN = torch.as_tensor(np.broadcast_to(np.array(ocfg.obstacles), (B, ocfg.N, K, 3)).copy(), device="cuda")
    ro = so.solve_batch(dPo, dWo, obstacles=f1, want_duals=True)
    wbo = torch.as_tensor(np.random.default_rng(1).normal(size=(B, ocfg.n_var)), device="cuda")
    dpo = torch.zeros_like(dPo)
    dpo[:, : ocfg.nx] = 1e-2
    variants["obs_plain_solve"] = lambda: so.solve_batch(dPo, dWo, obstacles=f1)
    variants["obs_gainsN_dw"] = lambda: so.sens_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], dp=dpo, gains="N", obstacles=f1)
    variants["obs_adjoint_static"] = lambda: so.sens_adjoint_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], wbo, obstacles=f1)
    variants["obs_adjoint_moving"] = lambda: so.sens_adjoint_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], wbo, obstacles=fN)
    dob1, dobN = torch.full_like(f1, 1e-3), torch.full_like(fN, 1e-3)      # every obstacle a millimetre off where the solve saw it
    variants["obs_dw_only"] = lambda: so.sens_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], dp=dpo, obstacles=f1)
    variants["obs_update_static"] = lambda: so.sens_update_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], dp=dpo, dobs=dob1, obstacles=f1)
    variants["obs_update_moving"] = lambda: so.sens_update_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], dp=dpo, dobs=dobN, obstacles=fN)
    variants["obs_update_moving_duals"] = lambda: so.sens_update_batch(dPo, ro["x"], ro["lam_g"], ro["lam_x"], dp=dpo, dobs=dobN, obstacles=fN, want_duals=True)
    res = {v: timed(f)[1] for v, f in variants.items()}      # warm-up (code objects, allocator)
    assert all(torch.equal(res["plain_solve"][k], r[k]) for k in ("x", "f", "status", "iters", "kkt"))      # the calls in between leave the solve as it was
    assert torch.equal(res["gains1"]["gains"][:, 0], res["gainsN_dw"]["gains"][:, 0]) and torch.equal(res["gains1_dw"]["dw"], res["gainsN_dw"]["dw"])
    assert torch.equal(res["adjoint"]["info"], res["gainsN_dw"]["info"]) and torch.equal(res["obs_adjoint_static"]["pbar"], res["obs_adjoint_moving"]["pbar"])
    assert torch.equal(res["update"]["info"], res["dw_only"]["info"]) and torch.equal(res["update"]["dw"], res["update_no_alpha"]["dw"])
    assert torch.equal(res["update_duals"]["dw"], res["update"]["dw"]) and torch.equal(res["update_duals"]["alpha"], res["update"]["alpha"])
    assert torch.equal(res["obs_update_moving_duals"]["dw"], res["obs_update_moving"]["dw"])
    assert torch.allclose(res["update"]["dw"], res["dw_only"]["dw"], rtol=0.0, atol=1e-9 * float(res["dw_only"]["dw"].abs().max()))
    ms = {v: [] for v in variants}
    for _ in range(reps):
        for v, f in variants.items():
            ms[v].append(timed(f)[0])
    info, ok = res["gainsN_dw"]["info"], (r["status"] == 0)
    out = {"library": nmpc_amd._lib.load().nmpc_version().decode(), "reps": reps, "B": B, "kernel": s.kernel_for_batch(B),
           "converged_frac": float(ok.double().mean()), "info_counts": torch.bincount(info.long(), minlength=3).tolist(),
           "info_ok_of_converged": float((info[ok] == 0).double().mean()), "gains_bytes": int(res["gainsN_dw"]["gains"].numel() * 8)}
    out["obs_info_counts"] = torch.bincount(res["obs_adjoint_moving"]["info"].long(), minlength=3).tolist()
    out["obs_converged_frac"] = float((ro["status"] == 0).double().mean())
    for v, t in ms.items():
        base = float(np.median(ms["obs_plain_solve" if v.startswith("obs_") else "plain_solve"]))      # each call against the solve that feeds it
        out[v] = {"ms_median": float(np.median(t)), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "vs_plain_solve": float(np.median(t)) / base}
    print("six robots B=%d: " % B + ", ".join("%s %.3f ms [%.3f, %.3f]" % (v, out[v]["ms_median"], out[v]["ms_min"], out[v]["ms_max"]) for v in variants)
          + "; gains S=N + dw at %.1f %%, adjoint at %.1f %% of the plain solve launch, adjoint with obsbar (per stage) at %.1f %% of its own; update (dp) at %.2f x nmpc_sens_batch(dp, gains=None), update (dp, dobs per stage) at %.2f x; update with multipliers at %.2f x the plain update, among obstacles %.2f x; info %s" % (
              100.0 * out["gainsN_dw"]["vs_plain_solve"], 100.0 * out["adjoint"]["vs_plain_solve"], 100.0 * out["obs_adjoint_moving"]["vs_plain_solve"],
              out["update"]["ms_median"] / out["dw_only"]["ms_median"], out["obs_update_moving"]["ms_median"] / out["obs_dw_only"]["ms_median"], out["update_duals"]["ms_median"] / out["update"]["ms_median"],
              out["obs_update_moving_duals"]["ms_median"] / out["obs_update_moving"]["ms_median"], out["info_counts"]),
          file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
