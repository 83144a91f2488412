"""Generates tests/golden/workspace_bytes.json: nmpc_workspace_bytes of a handle for every configuration of GRID.  Needs the GPU (a handle
allocates its workspace); runs no solve.

    python tests/golden/gen_workspace_bytes.py

The file pins the per-instance workspace strides of the swarm solve kernels: regenerate it only from a build whose workspace layout is
the intended one (it was recorded from the build before the layouts moved into structs).  tests/test_gpu_workspace_bytes.py checks a
build against it with measure() below.
Grid: every team size, heading bounded or free, no / two obstacles, horizons 2, 5, 6, 11, 20 (5, 6 and 11 sit on the steps of the
checkpoint slot count (N - 1) / 5 + 1), pin 0 (an LDS-resident kernel: stride2) and pin 1 (the HBM-resident kernel: stride), one and
three instances.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes.json")
GRID = [(m, thb, K, N, pin, mb) for m in range(1, 11) for thb in (0, 1) for K in (0, 2) for N in (2, 5, 6, 11, 20) for pin in (0, 1) for mb in (1, 3)]


def key(row):
    return "m%d thb%d K%d N%d pin%d B%d" % row


def measure():
    """{key(row): nmpc_workspace_bytes of the handle of that row} over GRID"""
    import nmpc_amd
    lib = nmpc_amd._lib
    L = lib.load()
    out = {}
    for row in GRID:
        m, thb, K, N, pin, mb = row
        cc = lib.CConfig()
        L.nmpc_config_default(C.byref(cc), m, N)
        cc.n_obs = K
        for o in range(K):
            cc.obs[3 * o], cc.obs[3 * o + 1], cc.obs[3 * o + 2] = 1.0 + o, 1.0, 0.2
        if thb:
            cc.th_max = 3.5
        h = C.c_void_p()
        lib.check(L.nmpc_create_opts(C.byref(cc), mb, C.byref(lib.COptions(kernel=pin, trace_instance=-1)), C.byref(h)), "nmpc_create_opts " + key(row))
        out[key(row)] = int(L.nmpc_workspace_bytes(h))
        lib.check(L.nmpc_destroy(h), "nmpc_destroy")
    return out


if __name__ == "__main__":
    got = measure()
    with open(PATH, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d handles -> %s" % (len(got), PATH))
