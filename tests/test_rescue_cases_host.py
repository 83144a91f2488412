"""CPU: the constructed rescue-ladder cases (tests/rescue_cases.py) on the oracle alone.  Every case has its eight distinct instances, every
instance passes the screen (the oracle holds its result under rounding-level perturbations of the inputs), the families go through the rungs
they claim — read from the oracle's ladder counters (nmpc_oracle_ladder_stats) and from a solve without the cold retry — every row of the table
appears in every family that applies to it, and the launch of every case names its row."""
import os

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO
from tests import rescue_cases as RC

CUS = 256      # compute units of an MI355X

CASES = RC.cases()
DISTINCT = {}
for _r, _lr, _fam in CASES:
    DISTINCT.setdefault(RC.case_key(_lr, _fam), (_lr, _fam))


def test_every_row_appears_in_its_families():
    got = {(r.row, fam) for r, _, fam in CASES}
    for r in KV.TABLE:
        assert (r.row, "garbage_guess") in got
        assert ((r.row, "overrun") in got) == (r.obs_field == "N")
        assert ((r.row, "outside_box") in got) == (not r.obs_field)
    plain = [r for r in KV.TABLE if not r.obs_field]
    assert {r.row[0] for r in plain} == {1, 2, 3}      # outside_box reaches all three kernels
    for m in range(1, 11):                              # and overrun every team size, with and without the duals in LDS
        assert {r.row[3] & 3 for r in KV.TABLE if r.obs_field == "N" and r.row[1] == m} >= ({0, 1} if m <= 6 else {0}), m


def test_every_launch_names_its_row(built):
    """the two changes to a row's recipe (pin 3 with the small batch instead of TP_BATCH instances, pin 1 at N = 20 instead of the long
    horizons of the HBM-resident rows) still launch the row: the device-free descriptor says so"""
    changed = 0
    for r in KV.TABLE:
        lr = RC.launch(r)
        rc, got, lds, _ = KV.variant_of_config(KV.c_config(R.NLPConfig(**lr.cfg), lr.max_iter), lr.pin, CUS, lr.B, lr.ordered, lr.obs_field)
        assert rc == 0 and got == r.row and 0 <= lds <= 160 * 1024, (r.row, lr.pin, lr.B, rc, got, lds)
        assert lr.max_iter == RC.MAX_ITER and lr.B <= 513
        if r.row[0] == 1:
            assert (lr.pin, lr.cfg["N"], lr.B) == (1, 20, RC.INSTANCES)
        elif r.B == KV.TP_BATCH.get(r.row[1]) and r.row[0] == 3:
            assert (lr.pin, lr.B) == (3, RC.INSTANCES) and lr.cfg == r.cfg
        else:
            assert lr.pin == r.pin and lr.cfg == r.cfg
        changed += (lr.pin, lr.cfg) != (r.pin, r.cfg)
    assert changed == 10 + sum(1 for r in KV.TABLE if r.row[0] == 3 and r.B > 16)


def _solve_env(cfg, P, W0, F, env):
    """the oracle with the fixture-generation switches of tests/golden/gen_moving_obstacle_cases.py"""
    old = {k: os.environ.pop(k, None) for k in ("NMPC_ORACLE_NO_COLD_RETRY", "NMPC_ORACLE_MAX_COLD")}
    os.environ.update(env)
    try:
        return KV.oracle_solve(cfg, P, W0, F, RC.MAX_ITER)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


@pytest.mark.parametrize("key", list(DISTINCT), ids=list(DISTINCT))
def test_case_is_screened_and_means_what_it_claims(built, key):
    lr, fam = DISTINCT[key]
    cfg, P, W0, F, picks = RC.inputs(lr, fam)
    assert len(picks) == len(set(picks)) == RC.INSTANCES == P.shape[0]
    assert len({p.tobytes() + w.tobytes() for p, w in zip(P, W0)}) == RC.INSTANCES      # distinct instances
    assert np.isfinite(P).all() and np.isfinite(W0).all()
    ok, status, iters = RC.screen(lr, fam)
    assert ok.all(), (key, np.flatnonzero(~ok), status, iters)
    ref = RC.oracle(lr, fam)
    lad = ref["ladder"]
    if fam == "garbage_guess":
        assert (status == 0).all() and (ref["kkt"] <= 1e-8).all(), status
        assert (lad[:, 0] == 1).all() and (lad[:, 2] == 0).all(), lad      # exactly one cold retry, no elastic phase
        none = _solve_env(cfg, P, W0, F, {"NMPC_ORACLE_NO_COLD_RETRY": "1"})
        # and without it the solve fails or is still iterating where the retry's watchdog stands (the criterion of gen_moving_obstacle_cases.py)
        assert ((none["status"] != 0) | (none["iters"] >= 500)).all(), (none["status"], none["iters"])
        cold = KV.oracle_solve(cfg, P, RC.cold_inputs(cfg, P), F, RC.MAX_ITER)
        assert (cold["status"] == 0).all()
        for k in ("x", "f", "kkt"):                                        # the retry keeps nothing of the failed attempt
            assert np.array_equal(ref[k], cold[k]), k
        attempt = iters - cold["iters"]
        assert (attempt > 0).all() and (attempt <= 500).all(), attempt      # a stall, a failed factorisation, or the watchdog at 500
    else:
        assert (status == 4).all(), status
        assert (lad[:, 0] == 2).all() and (lad[:, 2] > 0).all(), lad
        if fam == "overrun":
            assert (iters > 1000).all() and (iters < 1100).all(), iters
            assert all(MO.obstacle_values(cfg, ref["x"][b], F[b]).min() < cfg.margin - 1e-3 for b in range(RC.INSTANCES))
        else:
            assert not lr.obs_field and (P[:, 0] > cfg.xy_max).all()
            assert (iters > 1000).all() and (iters < RC.MAX_ITER - 500).all(), iters      # two attempts, and no status that depends on the cap
