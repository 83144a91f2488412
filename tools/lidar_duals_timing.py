"""Development aid (GPU box): what the LIDAR multipliers and the KKT certificate cost next to the solve they follow.

V4 (N = 100, Nc = 50, R = 10, the script's bounds, cold start, the generator of bench.py's LIDAR entry) at B = 1024 and B = 4096, three calls
on one handle: nmpc_lidar_solve_batch, nmpc_lidar_solve_batch_duals (the same solve, then the launch that reads the multipliers) and
nmpc_lidar_kkt_batch alone at the solve's primal-dual point.  Device events around each call, one warm-up of every call and shape, then
ROUNDS rounds in which the calls alternate in one process; per call the median and the spread (min .. max) over the rounds.

--other-so PATH: another build of libnmpc_hip.so (the parent commit's) whose nmpc_lidar_solve_batch joins the alternation on a handle of its
own: the solve kernel is the same code, so the difference to this build's plain call is the run-to-run spread of the measurement.

Prints one JSON line.  Needs a GPU: there is nothing to fall back to."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import nmpc_amd  # noqa: E402

SEED = 20210141 + 5


def make_batch(lc, solver, B):
    rng = np.random.Generator(np.random.PCG64(SEED))
    poses, worlds, goals = [], [], []
    for _ in range(B):
        poses.append([rng.uniform(0.0, 0.15), rng.uniform(0.0, 0.15), rng.uniform(0.4, 1.1)])
        worlds.append([(float(rng.uniform(0.8, 2.6)), float(rng.uniform(0.3, 2.4)), float(rng.uniform(0.15, 0.3))) for _ in range(3)])
        goals.append(np.array([3.0, 2.5, 0.0]) + rng.uniform(-0.3, 0.3, 3))
    poses = np.array(poses)
    scans = solver.scan_batch(poses, np.array(worlds)).cpu().numpy()
    P = np.stack([nmpc_amd.lidar_params(lc, poses[b], goals[b], scans[b]) for b in range(B)])
    W = np.stack([nmpc_amd.lidar_cold_start(lc, np.concatenate([poses[b], scans[b]])) for b in range(B)])
    return torch.as_tensor(P, device="cuda"), torch.as_tensor(W, device="cuda")


def other_plain_call(path, lc, lbx, ubx, B):
    """nmpc_lidar_solve_batch of another build of the library, on its own handle"""
    L = C.CDLL(path)
    vp, i32, dp = C.c_void_p, C.c_int32, C.POINTER(C.c_double)
    L.nmpc_lidar_create.argtypes = [C.POINTER(nmpc_amd._lib.CLidarConfig), dp, dp, i32, C.POINTER(vp)]; L.nmpc_lidar_create.restype = i32
    L.nmpc_lidar_solve_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]; L.nmpc_lidar_solve_batch.restype = i32
    L.nmpc_version.restype = C.c_char_p
    h = vp()
    cc = lc.to_c()
    nmpc_amd._lib.check(L.nmpc_lidar_create(C.byref(cc), lbx.ctypes.data_as(dp), ubx.ctypes.data_as(dp), B, C.byref(h)), "nmpc_lidar_create (other build)")
    return L, h, L.nmpc_version().decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--other-so", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lidar_duals_timing.py needs a GPU")
    lc = nmpc_amd.lidar_v4()
    lbx, ubx = (np.ascontiguousarray(a, dtype=np.float64) for a in lc.bounds()[:2])
    out = {"workload": "lidar_v4: N=100, Nc=50, R=10, cold start", "rounds": args.rounds, "library": nmpc_amd._lib.load().nmpc_version().decode(), "batches": []}
    for B in (int(b) for b in args.batches.split(",")):
        s = nmpc_amd.LidarSolver(lc, lbx=lbx, ubx=ubx, max_batch=B)
        L, h, st = s.lib, s._h, s._stream()
        p, w0 = make_batch(lc, s, B)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
        w, obj, kkt, status, iters = f64(B, lc.n_var), f64(B), f64(B), i32(B), i32(B)
        lam_g, lam_x, lam_p, res = f64(B, lc.n_g), f64(B, lc.n_var), f64(B, lc.n_p), f64(B, 6)
        cd = nmpc_amd._lib.CDuals(lam_g.data_ptr(), lam_x.data_ptr(), lam_p.data_ptr())
        solve_args = (B, p.data_ptr(), w0.data_ptr(), w.data_ptr(), obj.data_ptr(), status.data_ptr(), iters.data_ptr(), kkt.data_ptr())
        calls = {"solve": lambda: L.nmpc_lidar_solve_batch(h, *solve_args, st),
                 "solve_duals": lambda: L.nmpc_lidar_solve_batch_duals(h, *solve_args, C.byref(cd), st),
                 "kkt": lambda: L.nmpc_lidar_kkt_batch(h, B, p.data_ptr(), w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), res.data_ptr(), None, st)}
        other = None
        if args.other_so:
            Lo, ho, ver = other_plain_call(args.other_so, lc, lbx, ubx, B)
            other = ver
            calls["solve_other_build"] = lambda: Lo.nmpc_lidar_solve_batch(ho, *solve_args, st)
        order = ["solve_duals"] + [k for k in calls if k != "solve_duals"]      # the duals call first: kkt reads its multipliers
        ms = {k: [] for k in calls}
        for rnd in range(args.rounds + 1):      # round 0: the warm-up of every call at this shape
            for k in (order if rnd % 2 == 0 else order[:1] + order[1:][::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = calls[k]()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0, (k, rc)
                if rnd:
                    ms[k].append(a.elapsed_time(b))
        stc = status.cpu().numpy()
        rec = {"B": B, "converged_frac": float((stc == 0).mean()), "mean_iters": float(iters.double().mean()),
               "worst_stat_eq_compl": [float(v) for v in res[torch.as_tensor(stc == 0, device="cuda")][:, [0, 1, 4]].max(dim=0).values],
               "ms": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}}
        base = rec["ms"]["solve"]["median"]
        rec["duals_launch_ms"] = rec["ms"]["solve_duals"]["median"] - base
        rec["duals_launch_share_of_solve"] = rec["duals_launch_ms"] / base
        rec["kkt_share_of_solve"] = rec["ms"]["kkt"]["median"] / base
        if other:
            rec["other_build"] = other
            Lo.nmpc_lidar_destroy.argtypes = [C.c_void_p]; Lo.nmpc_lidar_destroy(ho)
        out["batches"].append(rec)
        del s
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
