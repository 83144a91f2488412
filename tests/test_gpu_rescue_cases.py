"""-m gpu: every solve-kernel instantiation goes through the rescue ladder like the CPU oracle, on the constructed cases of
tests/rescue_cases.py (barrier restarts, cold retry, elastic phase, statuses 0 and 4).

Per row and family: the descriptor must name the row for the case's launch, then the solve through the raw C ABI (helpers.guarded_call:
sentinel bands around every output, inputs unchanged, a second call bit-identical) is compared with the oracle on the same inputs.  The oracle
is the reference throughout; the one comparison of the library with itself is the identity the oracle shows too: a solve rescued by the cold
retry returns the bits of a solve started from the cold start."""
import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO
from tests import rescue_cases as RC
from tests.test_gpu_kernel_variants import _abi_solve, _compute_units, _handle, _order, _variant

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
CASES = RC.cases()


@pytest.mark.parametrize("r,lr,fam", CASES, ids=["%s-%s" % (KV.row_id(r), fam) for r, _, fam in CASES])
def test_rescue_case_solves_like_the_oracle(built, capsys, r, lr, fam):
    """All families: status equal on every instance, iterate finite, x0 pinned bit-exactly, bounds of stages 1..N and of the controls held to
    1e-12 (the x0 of outside_box is outside the box by construction; it is pinned), guard bands untouched and a second call bit-identical
    (guarded_call).
    garbage_guess: status 0, kkt <= 1e-8, w_out / obj / kkt bit-identical to the same handle's solve from nlp_ref.cold_start, more iterations
    than that solve, the oracle's point within 1e-6.
    overrun, outside_box: status 4; the oracle's point within 1e-6 and its iteration count on all but at most one instance; overrun also
    1000 < iters < 1100 and an obstacle row left open."""
    cfg, P8, W8, F8, _ = RC.inputs(lr, fam)
    P, W0, F = RC.tiled(lr, P8, W8, F8)
    B, nb = lr.B, RC.INSTANCES
    order = _order(B, 3) if lr.ordered else None
    L, h = _handle(cfg, RC.MAX_ITER, B + 3, lr.pin)
    try:
        rc, got, lds = _variant(L, h, B, lr.ordered, lr.obs_field)
        assert rc == 0 and got == r.row, ("the case launches another instantiation", r.row, rc, got)
        assert (rc, got, lds) == KV.variant_of_config(KV.c_config(cfg, RC.MAX_ITER), lr.pin, _compute_units(), B, lr.ordered, lr.obs_field)[:3]
        out = _abi_solve(L, h, cfg, P, W0, F, order)
        cold = _abi_solve(L, h, cfg, P, RC.cold_inputs(cfg, P), F, order) if fam == "garbage_guess" else None
    finally:
        L.nmpc_destroy(h)
    ref8 = RC.oracle(lr, fam)
    ref = {k: v[np.arange(B) % nb] for k, v in ref8.items()}      # a tiled batch repeats its instances: so does the reference
    dw = np.max(np.abs(out["x"] - ref["x"]), axis=1)
    same = dw[:nb] <= W_TOL
    it_eq = out["iters"][:nb] == ref["iters"][:nb]
    with capsys.disabled():
        print("\n  rescue %s %s B %d: same point %d/%d (max |dw| %.1e), iterations equal %d/%d, hip %d..%d oracle %d..%d"
              % (fam, got, B, same.sum(), nb, dw.max(), it_eq.sum(), nb, out["iters"].min(), out["iters"].max(), ref["iters"].min(), ref["iters"].max()), end="")
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    assert np.isfinite(out["x"]).all()
    assert np.array_equal(out["x"][:, : cfg.nx], P[:, : cfg.nx])
    lbx, ubx, _, _ = R.bounds(cfg)
    assert (out["x"][:, cfg.nx:] >= lbx[cfg.nx:] - 1e-12).all() and (out["x"][:, cfg.nx:] <= ubx[cfg.nx:] + 1e-12).all()
    for k in ("x", "status", "iters"):      # the copies of a tiled instance are solved alike
        assert np.array_equal(out[k], out[k][np.arange(B) % nb]), k
    if fam == "garbage_guess":
        assert (out["status"] == 0).all() and (out["kkt"] <= 1e-8).all(), (out["status"], out["kkt"].max())
        for k in ("x", "f", "kkt"):
            assert np.array_equal(out[k], cold[k]), ("the cold retry kept state of the failed attempt", k, np.flatnonzero((out[k] != cold[k]).reshape(B, -1).any(axis=1)))
        assert (cold["status"] == 0).all() and (out["iters"] > cold["iters"]).all(), (out["iters"], cold["iters"])
        assert (dw <= W_TOL).all(), dw
    else:
        assert (out["status"] == 4).all(), out["status"]
        assert (~same).sum() <= 1, (np.flatnonzero(~same), dw[:nb])
        assert (~it_eq).sum() <= 1, (out["iters"][:nb], ref["iters"][:nb])
        if fam == "overrun":
            assert (out["iters"] > 1000).all() and (out["iters"] < 1100).all(), out["iters"]
            assert all(MO.obstacle_values(cfg, out["x"][b], F[b]).min() < cfg.margin - 1e-3 for b in range(nb))
