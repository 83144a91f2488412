"""-m gpu: the pivot row of the column kernel's row-paired backward stage, replicated by lane gathers (docs/PIVOT_GATHER.md).

(i) One wavefront, one launch (tests/probes/pivot_gather_probe.hip): `own` and `ur` formed from registers of distinct lane tags by the lane
    swaps and by the two gathers, for a pivot row of the lower and of the upper half, compared with one another and with the lane
    emulation of tools/rp_emu.py.  The gathers leave the register as it was; the swaps leave the other row in both of its halves.

(ii) Solves.  What the gathers can break is whatever reads a register the swaps used to rearrange: the other row of a pivot's register at
    its own turn, the diagonal's lane of a later pivot, the resumed sweep after a rejected pivot.  Cases (tests/pivot_gather_cases.py):
    clusters standing at dmin (their sweeps reject pivots), teams of 2 .. 6 robots (3 and 5: the upper half's last robot slot is empty),
    with and without the heading bound, N = 6 and N = 11 (one and two saved cost-to-gos), 16 instances, on the throughput shape (pin 3)
    and on pin 4.  On EVERY instance the status and the iteration count are the C oracle's, the point is the oracle's within 1e-6 and the
    reported KKT error of a converged instance is at most 1e-8; the instances are screened on the oracle alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as Hh
from tests import pivot_gather_cases as GC
from tests import pivot_step_cases as PC
from tests import test_gpu_duals as TD
from tests import wave_probe_ref as WR

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
KKT_TOL = 1e-8
PINS = {3: 64, 4: 128}      # nmpc_options_t.kernel: threads per instance of the launch
PATTERNS = 2


def test_gathered_replicas_on_one_wavefront(tmp_path):
    if WR.hipcc() is None:
        pytest.skip("no hipcc on this box")
    sys.path.insert(0, os.path.join(WR.ROOT, "tools"))
    import rp_emu as E
    exe, dump = tmp_path / "pivot_gather_probe", tmp_path / "dump.bin"
    r = subprocess.run([WR.hipcc()] + WR.build_module().codegen_flags() + [os.path.join(WR.PROBE_DIR, "pivot_gather_probe.hip"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    try:
        r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the probe did not finish in 120 s", pytrace=False)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    w = np.frombuffer(dump.read_bytes(), dtype=np.float64).reshape(PATTERNS, 2, 6, 64)
    lanes = np.arange(64)
    for p in range(PATTERNS):
        tags = 1000.0 * (p + 1) + lanes + (lanes + 1) * 2.0 ** -40
        for hj in (0, 1):
            reg, own_s, ur_s, left_s, own_g, ur_g = w[p, hj]
            assert np.array_equal(reg, tags), (p, hj)
            assert np.array_equal(own_g, own_s) and np.array_equal(ur_g, ur_s), (p, hj, own_g, own_s, ur_g, ur_s)
            e_own, e_ur, e_left = E.replicate_swap(tags, hj)
            assert np.array_equal(own_s, e_own) and np.array_equal(ur_s, e_ur) and np.array_equal(left_s, e_left), (p, hj)
            g_own, g_ur, _ = E.replicate_gather(tags, hj)
            assert np.array_equal(own_g, g_own) and np.array_equal(ur_g, g_ur), (p, hj)


@pytest.mark.parametrize("pin", list(PINS))
@pytest.mark.parametrize("N", GC.HORIZONS)
@pytest.mark.parametrize("thb", (0, 1))
@pytest.mark.parametrize("m", GC.TEAMS)
def test_clusters_solve_like_the_oracle(built, capsys, m, thb, N, pin):
    import nmpc_amd
    cfg, P, W0, ref, _, whole = GC.select(m, N, thb)
    assert (ref["status"] == 0).all() and (whole > 0).any()      # the premises: the oracle converges, and sweeps of the case reject pivots
    pcfg = Hh.to_product_cfg(cfg, max_iter=PC.MAX_ITER, pair_rows=cfg.pair_rows)
    L = nmpc_amd._lib.load()
    h = C.c_void_p()
    cc, opts = pcfg.to_c(), nmpc_amd._lib.COptions(kernel=pin, trace_instance=-1)
    nmpc_amd._lib.check(L.nmpc_create_opts(C.byref(cc), GC.B, C.byref(opts), C.byref(h)), "nmpc_create_opts")
    try:
        rc, got = TD._variant(L, h, GC.B, 0, False)
        assert rc == 0 and got[:3] == (3, m, thb) and got[4] == PINS[pin], ("the case launches another kernel", rc, got)
        out = TD._solve(L, h, pcfg, np.array(P), np.array(W0), duals=None)      # (writable copies: the shared inputs stay unchanged)
    finally:
        L.nmpc_destroy(h)
    x = out["x"].view(np.float64).reshape(GC.B, pcfg.n_var)
    kkt = out["kkt"].view(np.float64).reshape(GC.B)
    dw = np.max(np.abs(x - ref["x"]), axis=1)
    conv = out["status"] == 0
    with capsys.disabled():
        print("\n  m %d thb %d N %d variant %s: max |dw| %.2e, max kkt %.2e, iterations %d..%d, iteration counts that differ %d, statuses that differ %d"
              % (m, thb, N, got, dw.max(), kkt[conv].max() if conv.any() else np.nan, out["iters"].min(), out["iters"].max(),
                 (out["iters"] != ref["iters"]).sum(), (out["status"] != ref["status"]).sum()), end="")
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    assert (out["iters"] == ref["iters"]).all(), (out["iters"], ref["iters"])
    assert (dw <= W_TOL).all(), dw
    assert (kkt[conv] <= KKT_TOL).all(), kkt
