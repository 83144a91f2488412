"""-m gpu: the LIDAR solve's own multipliers (nmpc_lidar_solve_batch_duals) and the device-side KKT certificate (nmpc_lidar_kkt_batch), raw C
ABI, every output carved out of sentinel-filled arrays (helpers.guarded_call: bands untouched, inputs unchanged, a second call bit-identical,
every element written).

Every assertion is tied to a solver-independent reference: tests/lidar_duals_ref.py (numpy, from oracle/lidar_ref.py) for the certificate,
the CPU oracle's re-solves for lam_p, and the certificate itself (held against numpy first) for the solver's multipliers.  The device runs
once per row (module cache); the tests below read that record.

Thresholds of test_solver_multipliers_certify_its_point: 10 x the worst value measured on an MI355X per row (MEASURED, also DESIGN.md), never
above 1e-6, the tolerance at which this project calls a point a KKT point of the NLP."""
import ctypes as C

import numpy as np
import pytest

from oracle import lidar_ref as LR
from tests import helpers as Hh
from tests import lidar_duals_ref as D
from tests import lidar_variants as LV
from tests.test_gpu_lidar import _product
from tests.test_gpu_lidar_variants import _handle, _two_wave_threshold, _variant

pytestmark = pytest.mark.gpu

KKT_POINT = 1e-6
LAM_P_TOL = 1e-5       # a decade above the 7.2e-7 measured on the CPU between the oracle's finite differences and least-squares multipliers
CASES = [(k, False) for k in D.ROWS] + [(D.W2_ROW, True)]
IDS = ["%s-N%d-Nc%d-R%d-%s" % ("w2" if w2 else "w1", *k) for k, w2 in CASES]
# worst (stat, eq, bnd, compl) over the status-0 instances of each row, measured on an MI355X
MEASURED = {"w1-N1-Nc1-R0-base": (2.23e-21, 2.78e-17, 0.0, 9.33e-11), "w1-N3-Nc1-R2-base": (6.09e-12, 1.07e-11, 0.0, 8.85e-09),
            "w1-N5-Nc2-R10-base": (3.02e-10, 3.52e-13, 0.0, 3.14e-09), "w1-N9-Nc4-R5-base": (2.76e-09, 1.63e-12, 0.0, 9.39e-09),
            "w1-N3-Nc1-R16-lw0": (7.13e-12, 1.06e-11, 0.0, 8.81e-09), "w1-N9-Nc4-R5-th2": (1.71e-09, 1.25e-12, 0.0, 7.95e-09),
            "w1-N9-Nc4-R5-dmax_inf": (2.76e-09, 1.66e-12, 0.0, 9.40e-09), "w1-N9-Nc4-R5-lw0_free": (2.67e-09, 1.60e-12, 0.0, 9.15e-09),
            "w1-N65-Nc32-R11-base": (7.03e-09, 8.18e-13, 0.0, 8.99e-09), "w1-N64-Nc64-R10-base": (7.91e-09, 1.00e-12, 0.0, 9.41e-09),
            "w2-N5-Nc2-R10-base": (3.14e-09, 3.77e-12, 0.0, 9.74e-09)}


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


SOLVE_OUTS = lambda cfg, B: dict(x=(B * cfg.n_var, "f8"), f=(B, "f8"), kkt=(B, "f8"), status=(B, "i4"), iters=(B, "i4"))


def _abi_plain(L, h, cfg, p, w0):
    B = p.shape[0]
    out = Hh.guarded_call(SOLVE_OUTS(cfg, B), [p, w0], lambda q: L.nmpc_lidar_solve_batch(h, B, p.data_ptr(), w0.data_ptr(), q["x"], q["f"], q["status"], q["iters"],
                                                                                         q["kkt"], _stream()))
    out["x"] = out["x"].reshape(B, cfg.n_var)
    return out


def _abi_duals(L, h, cfg, p, w0, null=False):
    import nmpc_amd
    B = p.shape[0]
    outs = SOLVE_OUTS(cfg, B)
    if not null:
        outs.update(lam_g=(B * cfg.n_g, "f8"), lam_x=(B * cfg.n_var, "f8"), lam_p=(B * cfg.n_p, "f8"))

    def call(q):
        d = None if null else C.byref(nmpc_amd._lib.CDuals(q["lam_g"], q["lam_x"], q["lam_p"]))
        return L.nmpc_lidar_solve_batch_duals(h, B, p.data_ptr(), w0.data_ptr(), q["x"], q["f"], q["status"], q["iters"], q["kkt"], d, _stream())
    out = Hh.guarded_call(outs, [p, w0], call)
    for k, n in (("x", cfg.n_var), ("lam_g", cfg.n_g), ("lam_x", cfg.n_var), ("lam_p", cfg.n_p)):
        if k in out:
            out[k] = out[k].reshape(B, n)
    return out


def _abi_kkt(L, h, cfg, P, W, LG, LX):
    import torch
    t = [torch.as_tensor(np.ascontiguousarray(a), device=_dev()) for a in (P, W, LG, LX)]
    B = P.shape[0]
    out = Hh.guarded_call(dict(res=(B * 6, "f8"), grad=(B * cfg.n_var, "f8")), t,
                          lambda q: L.nmpc_lidar_kkt_batch(h, B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), q["res"], q["grad"], _stream()))
    only = Hh.guarded_call(dict(res=(B * 6, "f8")), t,
                           lambda q: L.nmpc_lidar_kkt_batch(h, B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), q["res"], None, _stream()))
    assert np.array_equal(out["res"].view(np.int64), only["res"].view(np.int64)), "res depends on whether grad_lag is asked for"
    return out["res"].reshape(B, 6), out["grad"].reshape(B, cfg.n_var)


def _random_point(cfg, B, seed):
    """seeded (w, lam_g, lam_x) strictly inside the bounds and away from any solution: no term of the Lagrangian gradient vanishes"""
    rng = np.random.default_rng(seed)
    lbx, ubx, _, _ = LR.bounds(cfg)
    W = rng.normal(size=(B, cfg.n_var))
    W[:, : cfg.ns * (cfg.N + 1)].reshape(B, cfg.N + 1, cfg.ns)[:, :, 3:] = rng.uniform(0.3, 3.0, (B, cfg.N + 1, cfg.R))
    W[:, cfg.ns * (cfg.N + 1):] = rng.uniform(-0.9, 0.9, (B, 2 * cfg.Nc)) * ubx[cfg.ns * (cfg.N + 1):]
    W = np.clip(W, lbx + 0.05, ubx - 0.05)
    W[0, -2] = ubx[-2] + 0.25      # one variable beyond its bound: bnd is not zero on instance 0
    return W, rng.normal(size=(B, cfg.n_g)), rng.normal(size=(B, cfg.n_var))


_RUNS = {}


def _run(key, w2):
    """every device call of one row, once per process"""
    import torch
    if (key, w2) in _RUNS:
        return _RUNS[(key, w2)]
    r = D.row(key, two_wave=w2)
    B = r.B if r.B is not None else _two_wave_threshold() + 1
    cfg, P, W0 = LV.inputs(r, B)
    nb = min(B, 16)
    L, h = _handle(cfg, r.max_iter, B + 3)
    try:
        assert _variant(L, h, B)[1] == r.inst
        p = torch.as_tensor(P, device=_dev()).contiguous(); w0 = torch.as_tensor(W0, device=_dev()).contiguous()
        # the slots of the workspace hold a previous solve's values: the batch in reverse order puts a feasible instance into slot 1
        stale = _abi_duals(L, h, cfg, p.flip(0).contiguous(), w0.flip(0).contiguous())
        dual = _abi_duals(L, h, cfg, p, w0)
        plain = _abi_plain(L, h, cfg, p, w0)
        null = _abi_duals(L, h, cfg, p, w0, null=True)
        small = _abi_duals(L, h, cfg, p[:nb].contiguous(), w0[:nb].contiguous()) if w2 else None
        res, grad = _abi_kkt(L, h, cfg, P, dual["x"], dual["lam_g"], dual["lam_x"])
        Wr, LGr, LXr = _random_point(cfg, nb, 7)
        res_r, grad_r = _abi_kkt(L, h, cfg, P[:nb], Wr, LGr, LXr)
        LGn = LGr.copy(); nan_row = 3 * min(2, cfg.N); LGn[0, nan_row] = np.nan
        res_n, grad_n = _abi_kkt(L, h, cfg, P[:nb], Wr, LGn, LXr)
    finally:
        L.nmpc_lidar_destroy(h)
    _RUNS[(key, w2)] = dict(r=r, cfg=cfg, B=B, nb=nb, P=P, W0=W0, stale=stale, dual=dual, plain=plain, null=null, small=small, res=res, grad=grad,
                            rand=(Wr, LGr, LXr, res_r, grad_r), nan=(nan_row, res_n, grad_n))
    return _RUNS[(key, w2)]


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("key,w2", CASES, ids=IDS)
def test_duals_call_leaves_the_solve_bit_identical(built, key, w2):
    """x, f, status, iters and kkt of the duals call equal those of nmpc_lidar_solve_batch on the same handle bit for bit, and so does the duals
    call with duals = NULL; the multipliers of the call on a workspace that held another batch equal those of the repeated call (the second
    call inside guarded_call is bit-identical already); beyond the two-wave threshold the multipliers of the first 16 instances equal those of
    the one-wave build at B = 16."""
    g = _run(key, w2)
    for k in ("x", "f", "status", "iters", "kkt"):
        assert np.array_equal(_bits(g["dual"][k]), _bits(g["plain"][k])), k
        assert np.array_equal(_bits(g["null"][k]), _bits(g["plain"][k])), k
    for k in ("lam_g", "lam_x", "lam_p"):
        assert np.array_equal(_bits(g["stale"][k][::-1]), _bits(g["dual"][k])), k
        if w2:
            assert np.array_equal(_bits(g["small"][k]), _bits(g["dual"][k][: g["nb"]])), k
    if w2:
        assert g["B"] > 16 and np.array_equal(g["small"]["status"], g["dual"]["status"][: g["nb"]])


@pytest.mark.parametrize("key,w2", CASES, ids=IDS)
def test_infeasible_stage0_returns_zero_multipliers(built, key, w2):
    """instance 1 (status 3) has all three rows exactly zero, also in the slot that held a feasible instance's multipliers before"""
    g = _run(key, w2)
    n = LV.distinct(g["r"])
    stopped = np.arange(g["B"]) % n == 1
    assert (g["dual"]["status"][stopped] == 3).all() and (g["dual"]["status"][~stopped] == 0).all(), g["dual"]["status"]
    for k in ("lam_g", "lam_x", "lam_p"):
        a = g["dual"][k][stopped]
        assert a.size and (a == 0.0).all() and not np.isnan(a).any(), k
        assert (g["stale"][k][::-1][stopped] == 0.0).all(), k
    assert np.abs(g["dual"]["lam_g"][~stopped]).max() > 0.0


def _parity_tol(cfg, lam_g, lam_x):
    return 1e-12 * (cfg.N + 1) * (1.0 + np.abs(lam_g).max() + np.abs(lam_x).max())


@pytest.mark.parametrize("key,w2", CASES, ids=IDS)
def test_certificate_matches_numpy(built, capsys, key, w2):
    """nmpc_lidar_kkt_batch against tests/lidar_duals_ref.py on the same numbers: at the device's own (w, lam_g, lam_x) and at a seeded random
    point inside the bounds where no term vanishes; |difference| <= 1e-12 (N + 1) (1 + |lam_g|_inf + |lam_x|_inf) on grad_lag and on every
    entry of res: the 1e-12 of the eval pins scaled by the length of the longest sum and the size of its terms.  One NaN in lam_g reaches
    stat and the columns of its row and nothing else."""
    g = _run(key, w2)
    cfg, P, nb = g["cfg"], g["P"], g["nb"]
    worst = [0.0, 0.0]
    Wr, LGr, LXr, res_r, grad_r = g["rand"]
    for b in range(nb):
        for which, (w, lg, lx, res, grad) in enumerate(((g["dual"]["x"][b], g["dual"]["lam_g"][b], g["dual"]["lam_x"][b], g["res"][b], g["grad"][b]),
                                                        (Wr[b], LGr[b], LXr[b], res_r[b], grad_r[b]))):
            if not np.isfinite(lg).all():
                continue
            ref_res, ref_grad = D.residuals(cfg, w, P[b], lg, lx)
            tol = _parity_tol(cfg, lg, lx)
            dg, dr = np.abs(grad - ref_grad).max(), np.abs(res - ref_res).max()
            worst[which] = max(worst[which], max(dg, dr) / tol)
            assert dg <= tol and dr <= tol, (b, which, dg, dr, tol, res, ref_res)
            assert res[2] == 0.0
    lbx, ubx, _, _ = LR.bounds(cfg)
    one_sided = (np.isfinite(lbx) != np.isfinite(ubx)).any()
    assert res_r[:, [0, 1, 4]].min() > 0.0 and res_r[0, 3] > 0.2 and (res_r[1:, 3] == 0.0).all()      # the random point exercises every residual
    assert (res_r[:, 5] > 0.0).all() if one_sided else (res_r[:, 5] == 0.0).all()
    with capsys.disabled():
        print("\n  %s: certificate vs numpy, largest |difference| / tolerance: own point %.2f, random point %.2f" % (LV.row_id(g["r"]), *worst), end="")
    # the NaN
    row, res_n, grad_n = g["nan"]
    cols = np.flatnonzero(LR.jacobian(cfg, Wr[0], P[0])[row])
    assert cols.size >= 3
    hit = np.zeros(cfg.n_var, dtype=bool); hit[cols] = True
    assert np.isnan(grad_n[0][hit]).all() and np.array_equal(_bits(grad_n[0][~hit]), _bits(grad_r[0][~hit]))
    assert np.isnan(res_n[0, 0]) and np.array_equal(_bits(res_n[0, 1:]), _bits(res_r[0, 1:]))
    assert np.array_equal(_bits(res_n[1:]), _bits(res_r[1:])) and np.array_equal(_bits(grad_n[1:]), _bits(grad_r[1:]))


@pytest.mark.parametrize("key,w2", CASES, ids=IDS)
def test_solver_multipliers_certify_its_point(built, capsys, key, w2):
    """On every status-0 instance: sign == 0 exactly; lam_x == 0 exactly on stage 0 and on entries without a finite bound; lam_p[0:3] ==
    lam_g[0:3] and the scan part of lam_p == the stage-0 gd multipliers bit for bit; lam_p equals the reference's definition evaluated at the
    device's (w, lam_g); stat, eq, bnd and compl of the device certificate (held against numpy above) below 10 x the worst value measured on
    an MI355X for the row, never above 1e-6."""
    g = _run(key, w2)
    cfg, P, d = g["cfg"], g["P"], g["dual"]
    ok = d["status"] == 0
    res = g["res"][ok]
    worst = res[:, [0, 1, 3, 4]].max(axis=0)
    with capsys.disabled():
        print("\n  %s: worst over %d converged instances: stat %.2e eq %.2e bnd %.2e compl %.2e, |lam_g| up to %.1f"
              % (IDS[CASES.index((key, w2))], ok.sum(), *worst, np.abs(d["lam_g"][ok]).max()), end="")
    assert (res[:, 5] == 0.0).all() and (res[:, 2] == 0.0).all()
    lbx, ubx, _, _ = LR.bounds(cfg)
    free = ~np.isfinite(lbx) & ~np.isfinite(ubx); free[: cfg.ns] = True
    assert (d["lam_x"][ok][:, free] == 0.0).all()
    go = 3 * (cfg.N + 1)
    assert np.array_equal(_bits(d["lam_p"][ok][:, :3]), _bits(d["lam_g"][ok][:, :3]))
    assert np.array_equal(_bits(d["lam_p"][ok][:, 6: 6 + cfg.R]), _bits(d["lam_g"][ok][:, go: go + cfg.R]))
    for b in np.flatnonzero(ok)[: g["nb"]]:
        lp = D.lam_p(cfg, d["x"][b], P[b], d["lam_g"][b])
        # the certificate's tolerance, times the size of the stage-0 ranges and poses that multiply the multipliers in lam_p
        assert np.abs(lp - d["lam_p"][b]).max() <= _parity_tol(cfg, d["lam_g"][b], d["lam_x"][b]) * max(1.0, np.abs(d["x"][b]).max()), b
    bound = np.minimum(10.0 * np.asarray(MEASURED[IDS[CASES.index((key, w2))]]), KKT_POINT)
    assert (worst <= bound).all(), (worst, bound)


@pytest.mark.parametrize("key", D.LSQ_ROWS, ids=str)
def test_lam_p_is_the_derivative_of_the_oracles_optimal_cost(built, capsys, key):
    """-lam_p of the device against the central difference (h = 1e-5) of the CPU oracle's optimal cost under re-solves at p +- h e_i, every
    component of p, instances 0, 2 and 3: relative to max(1, |lam_p,i|) the error is at most 1e-5.  The reference is the CPU oracle alone."""
    g = _run(key, False)
    worst = 0.0
    for b in D.LSQ_INSTANCES:
        assert g["dual"]["status"][b] == 0
        lp = g["dual"]["lam_p"][b]
        err = np.abs(D.oracle_dfdp(key, b) + lp) / np.maximum(1.0, np.abs(lp))
        worst = max(worst, err.max())
        assert err.max() <= LAM_P_TOL, (b, int(err.argmax()), err.max(), lp)
    with capsys.disabled():
        print("\n  %s: |df*/dp + lam_p| / max(1, |lam_p|) %.1e" % (key, worst), end="")


def test_python_surface_returns_the_abi_numbers(built):
    """LidarSolver.solve_batch(want_duals=True), kkt_batch and the keyword call return the numbers of the raw ABI calls."""
    import torch
    import nmpc_amd
    key = (9, 4, 5, "base")
    g = _run(key, False)
    cfg, P, W0, d = g["cfg"], g["P"], g["W0"], g["dual"]
    lbx, ubx, _, _ = LR.bounds(cfg)
    s = nmpc_amd.LidarSolver(_product(cfg, max_iter=g["r"].max_iter), lbx=lbx, ubx=ubx, max_batch=g["B"])
    r = s.solve_batch(P, W0, want_duals=True)
    r0 = s.solve_batch(P, W0)
    assert set(r) - set(r0) == {"lam_g", "lam_x", "lam_p"}
    for k in ("x", "f", "status", "iters", "kkt", "lam_g", "lam_x", "lam_p"):
        assert np.array_equal(_bits(r[k].cpu().numpy()), _bits(d[k])), k
        if k in r0:
            assert np.array_equal(_bits(r[k].cpu().numpy()), _bits(r0[k].cpu().numpy())), k
    res, grad = s.kkt_batch(P, r["x"], r["lam_g"], r["lam_x"], want_grad=True)
    assert np.array_equal(_bits(res.cpu().numpy()), _bits(g["res"])) and np.array_equal(_bits(grad.cpu().numpy()), _bits(g["grad"]))
    assert torch.equal(s.kkt_batch(P, r["x"], r["lam_g"], r["lam_x"]), res)
    sol = s(x0=W0[0], p=P[0], lbx=lbx, ubx=ubx)
    for k, n in (("lam_g", cfg.n_g), ("lam_x", cfg.n_var), ("lam_p", cfg.n_p)):
        assert sol[k].shape == (n, 1) and np.array_equal(_bits(sol[k][:, 0].copy()), _bits(d[k][0])), k
    assert np.array_equal(sol["x"][:, 0], d["x"][0])


def test_closed_loop_certify_keeps_the_loop_and_reports_the_certificate(built):
    """simulate_lidar_closed_loop(certify=True) on 8 robots for 5 periods (N = 9, R = 5): the poses of certify=False bit for bit, and finite
    worst_stat / worst_eq / worst_compl per robot."""
    import nmpc_amd
    cfg = LR.LidarConfig(N=9, Nc=4, R=5, aligned_bounds=True)
    lbx, ubx, _, _ = LR.bounds(cfg)
    pose0, goals, world = Hh.lidar_episode_batch(20210141 + 67, 8)
    s = nmpc_amd.LidarSolver(_product(cfg, max_iter=600), lbx=lbx, ubx=ubx, max_batch=8)
    a = nmpc_amd.simulate_lidar_closed_loop(s, pose0, goals, world, max_steps=5, keep_poses=True)
    b = nmpc_amd.simulate_lidar_closed_loop(s, pose0, goals, world, max_steps=5, keep_poses=True, certify=True)
    assert a.steps == b.steps == 5 and np.array_equal(_bits(a.poses), _bits(b.poses)) and a.failed_solves == b.failed_solves
    assert np.array_equal(a.mean_iters_by_step, b.mean_iters_by_step)
    assert a.worst_stat is None and a.worst_eq is None and a.worst_compl is None
    for v in (b.worst_stat, b.worst_eq, b.worst_compl):
        assert v.shape == (8,) and np.isfinite(v).all() and (v >= 0.0).all()
    if b.failed_solves == 0:
        assert b.worst_stat.max() <= KKT_POINT and b.worst_eq.max() <= KKT_POINT and b.worst_compl.max() <= KKT_POINT
