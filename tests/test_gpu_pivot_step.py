"""-m gpu: the pivot step of the column kernel's row-paired backward stage, on starts whose sweeps reject pivots.

The pivot step takes its verdict from the diagonal lane's bit of the compare mask, leaves the reciprocal of a rejected pivot as it comes,
forms the right-hand side of a pivot row on the diagonal's lane and stores it from there (docs/PIVOT_STEP.md).  What that can break is the
retry after a rejected pivot — a stage that goes on with an arbitrary reciprocal, the rows, right-hand sides and saved cost-to-go it leaves
behind, the resumed sweep — and the lane that stores the right-hand side, whose robot slot is empty in the upper half of an odd team.

Cases (tests/pivot_step_cases.py): clusters of m = 2 (the smallest row-paired team), 3 and 5 (odd teams) and 6 robots standing at dmin from
one another, cold start, 64 instances each, on the column kernel's throughput shape (pin 3) and latency shape (pin 4); N = 3 (no cost-to-go
is ever saved: every retry starts again at stage N - 1 from the terminal block) and N = 6 (exactly one is saved, on entry to stage 0).
The oracle's counters show that every case rejects pivots during its solves, that at N = 6 most instances reject in their FIRST sweep and
some of those reject at stage 0 only (at N = 3 two or three instances of the five- and six-robot cases do); no start can reject at stage
N - 1, whose control block is positive definite by construction (tests/pivot_step_cases.py says why, and the test holds that the oracle
never does; tests/test_pivot_step_host.py holds all of this without a GPU).

On EVERY instance the status and the iteration count are the C oracle's and the point is the oracle's within 1e-6 — the bounds of
tests/test_gpu_phase_passes.py; the instances are screened on the oracle alone, as there (pivot_step_cases.holds)."""
import numpy as np
import pytest

from tests import helpers as Hh
from tests import pivot_step_cases as PC
from tests import test_gpu_duals as TD
from tests import test_gpu_phase_passes as PP

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
TEAMS = (2, 3, 5, 6)
HORIZONS = (3, 6)
PINS = {3: 64, 4: 128}      # nmpc_options_t.kernel: threads per instance of the launch


@pytest.mark.parametrize("pin", list(PINS))
@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("m", TEAMS)
def test_rejecting_starts_solve_like_the_oracle(built, capsys, m, N, pin):
    cfg, P, W0, ref, _, _ = PC.select(m, N)
    pcfg = Hh.to_product_cfg(cfg, max_iter=PC.MAX_ITER, pair_rows=cfg.pair_rows)
    L, h = PP._handle(cfg, PC.B, pin)
    try:
        rc, got = TD._variant(L, h, PC.B, 0, False)
        assert rc == 0 and got[:3] == (3, m, 0) and got[4] == PINS[pin], ("the case launches another kernel", rc, got)
        out = TD._solve(L, h, pcfg, np.array(P), np.array(W0), duals=None)      # (writable copies: the shared inputs stay unchanged)
    finally:
        L.nmpc_destroy(h)
    x = out["x"].view(np.float64).reshape(PC.B, pcfg.n_var)
    dw = np.max(np.abs(x - ref["x"]), axis=1)
    with capsys.disabled():
        print("\n  m %d N %d variant %s: max |dw| %.2e, iterations %d..%d, iteration counts that differ %d, statuses that differ %d"
              % (m, N, got, dw.max(), out["iters"].min(), out["iters"].max(), (out["iters"] != ref["iters"]).sum(), (out["status"] != ref["status"]).sum()), end="")
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    assert (out["iters"] == ref["iters"]).all(), (out["iters"], ref["iters"])
    assert (dw <= W_TOL).all(), dw
