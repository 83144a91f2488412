"""-m gpu: the column kernel's stage-parallel passes at the smallest shapes where their (stage, robot) item loops can go wrong.

Where an instance has no obstacle rows the optimality-error pass writes the stage packs as it goes (one pass over the (stage, robot) items
and one over the (stage, pair) rows instead of two each), and writes their mu-dependent part again when the barrier parameter moves.  An item
is the state rows of stage k + 1 and the control rows of stage k, so it writes into two packs; a wavefront takes 64 items per trip, the last
stage has states and no controls, the multipliers start at stage 1 and the pair rows live on stages 1 .. N - 1: the cases sit on those edges,
and two carry obstacle rows (the separate passes).  Each case is solved once through nmpc_solve_batch (nmpc_solve_batch_obs for the field
case) and once through nmpc_solve_batch_duals, 16 instances, and on EVERY instance of both calls the status and the iteration count are the
C oracle's and the point is the oracle's within 1e-6 (the bounds of tests/test_gpu_kernel_variants.py, without its one-instance allowance).

Seeds.  tests/helpers.batch(cfg, 16, seed) (moving_obstacles_ref.moving_batch(cfg, 16, 900 + seed) for the field case), the first seed
from 5 upwards at which the oracle converges (status 0) on all 16 instances in under 60 iterations and holds its point to 1e-8 and its
iteration counts under the rounding-level perturbation of tests/kernel_variants.screen (so that no instance sits on a rounding fork of the
oracle's own): seed 5 for every case.  The build BEFORE the passes were fused met every assertion of this file at these seeds on an MI355X
(21 passed), so a failure here is the fusion's and not a fork that was always there.

Horizon 1 (no pair stage, a one-step recursion) is outside the C ABI (nmpc_config_t.N is 2..4096: nmpc_create returns NMPC_E_ARG), which the
last test holds; what that shape would exercise is covered from inside the ABI by two robots at N = 2 without pair rows (no pair stage at
all, the pair slots never touched) and with them (one pair stage; the recursion takes its first step without and its second with the
stage-coupling branch)."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO
from tests import test_gpu_duals as TD

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
B = 16
MAX_ITER = 400
ITER_LIMIT = 60

# name: (team, horizon, heading bound, obstacles, pair rows, pin, field, seed, (kernel, m, thb, flags, threads) the launch must be)
CASES = {
    "four_N16_one_trip": (4, 16, 0, 0, 1, 0, 0, 5, (3, 4, 0, 1, 128)),               # 64 items: exactly one trip of a wavefront (two wavefronts: half a trip each)
    "four_N16_one_trip_one_wave": (4, 16, 0, 0, 1, 3, 0, 5, (3, 4, 0, 1, 64)),       # the same on the throughput shape, one wavefront
    "six_N11_over_one_trip": (6, 11, 0, 0, 1, 3, 0, 5, (3, 6, 0, 0, 64)),            # 66 items: a second trip of two lanes
    "six_N22_two_waves": (6, 22, 0, 0, 1, 4, 0, 5, (3, 6, 0, 1, 128)),               # 132 items on 128 lanes: a second trip of four lanes
    "one_N3_no_pairs": (1, 3, 0, 0, 1, 0, 0, 5, (3, 1, 0, 1, 64)),                   # no pair rows, three items
    "two_N2_one_pair_stage": (2, 2, 0, 0, 1, 0, 0, 5, (3, 2, 0, 2, 64)),             # one pair stage; a two-step recursion
    "two_N2_no_pair_stage": (2, 2, 0, 0, 0, 0, 0, 5, (3, 2, 0, 2, 64)),              # no pair stage at all
    "six_N11_heading_bound": (6, 11, 1, 0, 1, 3, 0, 5, (3, 6, 1, 0, 64)),            # three bounded states per item
    "six_N5_two_obstacles": (6, 5, 0, 2, 1, 3, 0, 5, (3, 6, 0, 0, 64)),
    "six_N5_two_obstacles_field": (6, 5, 0, 2, 1, 3, "N", 5, (3, 6, 0, 4, 64)),      # the same rows from the per-instance field
}


def case_cfg(name):
    m, N, thb, K, pairs, _, _, _, _ = CASES[name]
    d = KV._cfg(m, N, thb, K, True)
    if not pairs:
        d["pair_rows"] = False
        d["pad_rows"] = False
    return R.NLPConfig(**d)


def case_inputs(name):
    """(oracle config, P, W0, field or None) of a case"""
    cfg = case_cfg(name)
    fld, seed = CASES[name][6], CASES[name][7]
    if fld:
        P, W0, F = MO.moving_batch(cfg, B, 900 + seed)
        return cfg, np.ascontiguousarray(P), np.ascontiguousarray(W0), np.ascontiguousarray(F)
    P, W0 = Hh.batch(cfg, B, seed)
    return cfg, np.ascontiguousarray(P), np.ascontiguousarray(W0), None


def _product_cfg(cfg):
    return Hh.to_product_cfg(cfg, max_iter=MAX_ITER, pair_rows=cfg.pair_rows)


def _handle(cfg, max_batch, pin):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    cc = _product_cfg(cfg).to_c()
    h = C.c_void_p()
    o = nmpc_amd._lib.COptions(kernel=pin, trace_instance=-1)
    nmpc_amd._lib.check(L.nmpc_create_opts(C.byref(cc), max_batch, C.byref(o), C.byref(h)), "nmpc_create_opts")
    return L, h


_REF = {}


def _reference(name):
    """the oracle's solve of a case, computed once and shared by the two calls"""
    if name not in _REF:
        cfg, P, W0, F = case_inputs(name)
        ref = KV.oracle_solve(cfg, P, W0, F, MAX_ITER)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


@pytest.mark.parametrize("duals", [None, "gxp"], ids=["solve_batch", "solve_batch_duals"])
@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_fused_passes_solve_like_the_oracle(built, capsys, name, duals):
    cfg, P, W0, F = case_inputs(name)
    pin, row = CASES[name][5], CASES[name][8]
    ref = _reference(name)
    assert (ref["status"] == 0).all() and ref["iters"].max() < ITER_LIMIT, (ref["status"], ref["iters"])      # the seed's screening, held here too
    L, h = _handle(cfg, B + 3, pin)
    try:
        rc, got = TD._variant(L, h, B, 0, F is not None)
        assert rc == 0 and got == row, ("the case launches another instantiation", row, rc, got)
        pcfg = _product_cfg(cfg)
        out = TD._solve(L, h, pcfg, P, W0, F=F, duals=duals)
    finally:
        L.nmpc_destroy(h)
    x = out["x"].view(np.float64).reshape(B, pcfg.n_var)
    dw = np.max(np.abs(x - ref["x"]), axis=1)
    with capsys.disabled():
        print("\n  %s %s variant %s: max |dw| %.2e, iterations hip %s oracle %s" % (name, duals or "plain", got, dw.max(), out["iters"].tolist(), ref["iters"].tolist()), end="")
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    assert (out["iters"] == ref["iters"]).all(), (out["iters"], ref["iters"])
    assert (dw <= W_TOL).all(), dw
    if duals:
        for k, n in (("lam_g", pcfg.n_g), ("lam_x", pcfg.n_var), ("lam_p", 2 * pcfg.nx)):
            assert np.isfinite(out[k].view(np.float64)).all() and out[k].size == B * n, k


def test_horizon_one_is_outside_the_abi(built):
    """N = 1 — no pair stage, a one-step recursion — cannot be asked of the library: nmpc_config_t.N is 2..4096 (include/nmpc.h)"""
    import nmpc_amd
    cc = Hh.to_product_cfg(R.NLPConfig(**KV._cfg(2, 2, 0, 0, True)), max_iter=10).to_c()
    cc.N = 1
    h = C.c_void_p()
    o = nmpc_amd._lib.COptions(kernel=0, trace_instance=-1)
    assert nmpc_amd._lib.load().nmpc_create_opts(C.byref(cc), 4, C.byref(o), C.byref(h)) == -1      # NMPC_E_ARG
