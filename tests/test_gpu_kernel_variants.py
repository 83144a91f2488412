"""-m gpu: every solve-kernel instantiation of the library (the table of tests/kernel_variants.py) solves like the CPU oracle.

Per row: nmpc_debug_variant() must name exactly that row for the row's recipe (so the launch below runs that instantiation and no other),
then the solve through the raw C ABI is compared with oracle_lib.solve_batch / solve_batch_obs on the same seeded inputs, by the
conventions of tests/test_gpu_parity.py.  The long horizons of the HBM-resident kernel are compared along the path (bounded iterations).
Every call is made with its outputs carved out of the middle of larger sentinel-filled arrays on a handle with max_batch > B: the bands around
every output stay untouched, the inputs come back bit-identical, and a second call returns bit-identical outputs."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
F_RTOL = 1e-6


def _handle(cfg, max_iter, max_batch, pin):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    cc = Hh.to_product_cfg(cfg, max_iter=max_iter).to_c()
    h = C.c_void_p()
    o = nmpc_amd._lib.COptions(kernel=pin, trace_instance=-1)
    nmpc_amd._lib.check(L.nmpc_create_opts(C.byref(cc), max_batch, C.byref(o), C.byref(h)), "nmpc_create_opts")
    return L, h


def _variant(L, h, B, ordered, obs_field):
    import nmpc_amd
    v = nmpc_amd._lib.CDebugVariant()
    rc = L.nmpc_debug_variant(h, B, int(ordered), int(bool(obs_field)), C.byref(v))
    return rc, (v.kernel, v.m, v.thb, v.flags, v.threads), int(v.lds_bytes)


def _abi_solve(L, h, cfg, P, W0, F, order):
    """One nmpc_solve_batch / _ordered / _obs call with guarded outputs, twice (helpers.guarded_call).  Returns the outputs of the first call
    as numpy arrays."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    B, nvar = P.shape[0], W0.shape[1]
    p = torch.as_tensor(P, device=dev).contiguous(); w0 = torch.as_tensor(W0, device=dev).contiguous()
    od = torch.as_tensor(order, device=dev).to(torch.int32).contiguous() if order is not None else None
    ob = torch.as_tensor(F, device=dev).contiguous() if F is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(ptr):
        if ob is not None:
            return L.nmpc_solve_batch_obs(h, B, p.data_ptr(), ob.data_ptr(), int(ob.shape[1]), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"],
                                          ptr["kkt"], od.data_ptr() if od is not None else None, stream)
        if od is not None:
            return L.nmpc_solve_batch_ordered(h, B, p.data_ptr(), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"], ptr["kkt"], od.data_ptr(), stream)
        return L.nmpc_solve_batch(h, B, p.data_ptr(), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"], ptr["kkt"], stream)
    out = Hh.guarded_call(dict(x=(B * nvar, "f8"), f=(B, "f8"), kkt=(B, "f8"), status=(B, "i4"), iters=(B, "i4")),
                          [t for t in (p, w0, od, ob) if t is not None], call)
    out["x"] = out["x"].reshape(B, nvar)
    return out


def _compute_units():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _order(B, seed):
    return np.random.default_rng(seed).permutation(B).astype(np.int32)


@pytest.mark.parametrize("r", KV.TABLE, ids=[KV.row_id(r) for r in KV.TABLE])
def test_variant_solves_like_the_oracle(built, capsys, r):
    """Step 1: the descriptor returns exactly this row for the recipe.  Step 2: status equal on every instance and all converged, reported
    kkt <= 1e-8, the oracle's point (1e-6) and objective (1e-6 relative) on every instance but at most one, which must then pass
    nlp_ref.kkt_report with the thresholds of test_gpu_parity.py, iteration counts equal on at least 0.9 of the batch, x0 pinned bit-exactly,
    bounds held to 1e-12.  The inputs are screened (test_kernel_variants_host.py) so that the oracle alone never needs the allowance."""
    import nmpc_amd
    cfg, P, W0, F = KV.inputs(r)
    B = r.B
    L, h = _handle(cfg, r.max_iter, B + 3, r.pin)
    try:
        rc, got, lds = _variant(L, h, B, r.ordered, r.obs_field)
        assert rc == 0 and got == r.row, ("the recipe launches another instantiation", r.row, rc, got)
        assert (rc, got, lds) == KV.variant_of_config(KV.c_config(cfg, r.max_iter), r.pin, _compute_units(), B, r.ordered, r.obs_field)[:3]
        out = _abi_solve(L, h, cfg, P, W0, F, _order(B, 3) if r.ordered else None)
    finally:
        L.nmpc_destroy(h)
    nb = min(B, 16)
    ref16 = KV.oracle_solve(cfg, P[:nb], W0[:nb], F[:nb] if F is not None else None, r.max_iter)
    ref = {k: v[np.arange(B) % nb] for k, v in ref16.items()}      # a tiled batch repeats its instances: so does the reference
    dw = np.max(np.abs(out["x"] - ref["x"]), axis=1)
    rel = np.abs(out["f"] - ref["f"]) / np.maximum(1.0, np.abs(ref["f"]))
    same = (dw <= W_TOL) & (rel <= F_RTOL)
    it_eq = out["iters"] == ref["iters"]
    with capsys.disabled():
        print("\n  variant %s lds %d B %d: same point %d/%d (max |dw| %.1e), iterations equal %d/%d, hip %d..%d oracle %d..%d"
              % (got, lds, B, same.sum(), B, dw.max(), it_eq.sum(), B, out["iters"].min(), out["iters"].max(), ref["iters"].min(), ref["iters"].max()), end="")
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    assert (out["status"] == 0).all(), out["status"]
    assert (out["kkt"] <= 1e-8).all(), out["kkt"].max()
    off = np.flatnonzero(~same)
    assert off.size <= 1, (off, dw[off], rel[off])
    for b in off:
        k = R.kkt_report(cfg, out["x"][b], P[b], tol_active=1e-3) if F is None else \
            MO.kkt_report(cfg, out["x"][b], P[b], F[b, 0] if F.shape[1] == 1 else F[b], tol_active=1e-3)
        assert k["stat"] < 1e-5 and k["eq"] < 1e-7 and k["ineq"] < 1e-7 and k["bnd"] < 1e-9, (b, k)
    assert it_eq.mean() >= 0.9, (out["iters"], ref["iters"])
    assert np.array_equal(out["x"][:, : cfg.nx], P[:, : cfg.nx])
    lbx, ubx, _, _ = R.bounds(cfg)
    assert (out["x"] >= lbx - 1e-12).all() and (out["x"] <= ubx + 1e-12).all()


def test_own_choice_never_launches_the_element_kernel(built):
    """Why every element-per-lane row is pinned: for five to ten robots, both heading flags, 0 / 1 / 2 / 8 obstacles and every horizon up to
    the first one of the HBM-resident kernel, the unpinned library launches the column kernel (B = 1 satisfies every batch condition of
    kernel_for_batch), then kernel 1: the element-per-lane kernel outgrows the LDS before the column kernel's latency shape does."""
    import nmpc_amd
    seen = set()
    for m in range(5, 11):
        for thb in (0, 1):
            for K in (0, 1, 2, 8):
                d = KV._cfg(m, 2, thb, 2 if K else 0, True)
                if K:
                    d["obstacles"] = [(0.0, 0.0, 0.1)] * K
                for N in range(2, KV.KERNEL1[m] + 1):
                    d["N"] = N
                    L, h = _handle(R.NLPConfig(**d), 10, 1, 0)
                    rc, got, _ = _variant(L, h, 1, 0, 0)
                    L.nmpc_destroy(h)
                    assert rc == 0 and got[0] in (1, 3), (m, thb, K, N, rc, got)
                    assert (got[0] == 1) == (N >= KV.KERNEL1[m]), (m, thb, K, N, got)
                    seen.add(got)
    assert {v[0] for v in seen} == {1, 3}


def test_descriptor_argument_errors(built):
    """NMPC_E_ARG / NMPC_E_UNSUPPORTED where the call itself would return them"""
    L, h = _handle(R.NLPConfig(**KV._cfg(2, 20, 0, 0, True)), 10, 4, 0)
    L2, h2 = _handle(R.NLPConfig(**KV._cfg(2, 20, 0, 2, True)), 10, 4, 2)
    try:
        assert _variant(L, h, 5, 0, 0)[0] == -1 and _variant(L, h, -1, 0, 0)[0] == -1      # beyond max_batch, negative
        assert _variant(L, h, 4, 0, 1)[0] == -1                                               # a field call on a handle without obstacle rows
        assert L.nmpc_debug_variant(h, 1, 0, 0, None) == -1
        assert _variant(L2, h2, 4, 0, 1)[0] == -2                                             # a field call on a handle pinned off the column kernel
        assert _variant(L2, h2, 4, 0, 0)[:2] == (0, (2, 2, 0, 0, 64))
    finally:
        L.nmpc_destroy(h); L2.nmpc_destroy(h2)


@pytest.mark.parametrize("name", list(KV.PATHS), ids=list(KV.PATHS))
def test_long_horizon_path_matches_the_oracle(built, capsys, name):
    """The HBM-resident kernel far beyond the LDS limit (the library's own choice), max_iter = K on both sides: status and iteration count
    equal, iterate and reported kkt within the case's tolerance (100 x the oracle's own spread under a rounding-level perturbation, see
    tests/kernel_variants.PATHS)."""
    p = KV.PATHS[name]
    assert 1e-12 <= p.tol <= 1e-6 and p.N >= 1.5 * KV.KERNEL1[p.m]      # tol = 100 x spread: held where PATHS is defined
    cfg, P, W0 = KV.path_inputs(p)
    L, h = _handle(cfg, p.max_iter, p.B + 1, 0)
    try:
        rc, got, _ = _variant(L, h, p.B, 0, 0)
        assert rc == 0 and got == (1, p.m, 0, 0, 64 if p.m <= 6 else 128), got
        out = _abi_solve(L, h, cfg, P, W0, None, None)
    finally:
        L.nmpc_destroy(h)
    ref = KV.oracle_solve(cfg, P, W0, None, p.max_iter)
    dev = KV.path_deviation(out, ref)
    with capsys.disabled():
        print("\n  path %s variant %s: status %s iterations %s (oracle %s), deviation %.2e against tolerance %.1e (oracle spread %.1e)"
              % (name, got, out["status"].tolist(), out["iters"].tolist(), ref["iters"].tolist(), dev, p.tol, p.spread), end="")
    assert (out["status"] == ref["status"]).all() and (out["iters"] == ref["iters"]).all(), (out["status"], ref["status"], out["iters"], ref["iters"])
    assert (out["iters"] == p.max_iter).all()      # the path is cut, not converged
    assert dev <= p.tol, (dev, p.tol)
