"""Development aid (GPU box): bit-identity of two library builds.  One process per library:
    NMPC_SO=<a.so> python tools/ab_outputs.py a.npz          every output array of the fixed case list below, solved on that library
    NMPC_SO=<b.so> python tools/ab_outputs.py b.npz
    python tools/ab_outputs.py --compare a.npz b.npz         lists the arrays whose bit patterns differ (exit status 1 if any)
    python tools/ab_outputs.py --compare-dumps dirA dirB     the same for two `bench.py --dump-outputs` directories
Cases: the ten shapes of tests/test_gpu_phase_passes.py (plain call and with multipliers), the elastic / cold-retry fixtures of the composite
and the moving-obstacle rescue fixtures (per-instance field) on pins 3, 4, 5, and nmpc_solve_batch_duals on the six-robot bench batch.  After
each solve the handle's workspace is recorded too, as one sha256 per instance (`<case>/ws`): a changed scratch value shows even where no
output moved.  NaN payloads count: arrays are compared as raw bytes."""
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


def record(out, name, s, P, W, **kw):
    import torch
    r = s.solve_batch(P, W, **kw)
    torch.cuda.synchronize()
    for k, v in r.items():
        out["%s/%s" % (name, k)] = v.cpu().numpy()
    out[name + "/ws"] = workspace_hashes(s, len(P))
    print("%-52s status %s iterations %d..%d" % (name, sorted(set(out[name + "/status"].tolist())), out[name + "/iters"].min(), out[name + "/iters"].max()), flush=True)


def run(path):
    import nmpc_amd
    from tests import helpers as Hh
    from tests import moving_obstacles_ref as MO
    from tests import test_gpu_phase_passes as PP
    out = {}
    for name in PP.CASES:
        cfg, P, W0, F = PP.case_inputs(name)
        for duals in (False, True):
            s = nmpc_amd.NmpcSolver(PP._product_cfg(cfg), max_batch=PP.B + 3, kernel=PP.CASES[name][5])
            record(out, name + ("_duals" if duals else ""), s, P, W0, obstacles=F, want_duals=duals)
    oc = Hh.bench_batch("composite", 1)[0]
    gold = os.path.join(ROOT, "tests", "golden")
    for f in ("elastic_cases", "cold_retry_cases", "cold_retry_cases2"):
        z = np.load(os.path.join(gold, f + ".npz"))
        for pin in (3, 4, 5):
            s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(oc, max_iter=2000), max_batch=len(z["p"]), kernel=pin)
            record(out, "%s_pin%d" % (f, pin), s, z["p"], z["w"])
    z = np.load(os.path.join(gold, "moving_obstacle_cases.npz"))
    for pin in (3, 4, 5):
        s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(MO.team_cfg(6, 25, 8), max_iter=2000), max_batch=len(z["p"]), kernel=pin)
        record(out, "moving_obstacle_cases_pin%d" % pin, s, z["p"], z["w"], obstacles=z["obs"])
    oc, B, P, W0 = Hh.bench_batch("six", 64)
    record(out, "bench_six_64_duals", nmpc_amd.NmpcSolver(Hh.to_product_cfg(oc, max_iter=2000), max_batch=B), P, W0, want_duals=True)
    np.savez_compressed(path, **out)
    print("%d arrays of %s -> %s" % (len(out), nmpc_amd._lib.SO_PATH, path))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"] or sys.argv[1:2] == ["--compare-dumps"]:
        a, b = (load_dumps(p) for p in sys.argv[2:4]) if sys.argv[1] == "--compare-dumps" else (dict(np.load(p)) for p in sys.argv[2:4])
        bad = compare(a, b)
        print("%d arrays compared, %d differ%s" % (len(set(a) | set(b)), len(bad), (": " + ", ".join(bad)) if bad else ""))
        sys.exit(1 if bad else 0)
    run(sys.argv[1])
