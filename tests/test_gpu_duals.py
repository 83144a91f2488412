"""-m gpu: the solver's own multipliers (nmpc_solve_batch_duals / nmpc_step_batch_duals) and the device-side KKT certificate (nmpc_kkt_batch).

The multipliers are held to account as they are, in CasADi's convention (include/nmpc.h), by tests/duals_ref.py: nothing is fitted.  Bounds of
the checks: 1e-6 on the stationarity residual and on complementarity is the figure of every kkt_report assertion of the project (the kernel's
own test guarantees tol * s_d = 1e-8 * s_d); 1e-12 between nmpc_kkt_batch and numpy is the tolerance of the eval pins (two fp64 summation orders
of O(1) terms)."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import duals_ref as D
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO

pytestmark = pytest.mark.gpu

GUARD = 64
SENT64 = 0x7FF4DEADBEEF0123             # a NaN payload no solve produces
SENT32 = 0x5A5A5A5A
COLUMN_ROWS = [r for r in KV.TABLE if r.row[0] == 3]
BOUND = 1e-6


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
    return rc, (v.kernel, v.m, v.thb, v.flags, v.threads)


def _solve(L, h, cfg, P, W0, F=None, order=None, duals="gxp", expect=0):
    """One solve through the raw C ABI with every output in the middle of a sentinel-filled buffer.  duals = None: the EXISTING call
    (nmpc_solve_batch / _ordered / _obs); else nmpc_solve_batch_duals with the members named in `duals` ('g', 'x', 'p') given and the others
    NULL.  Returns the outputs as int64 / int32 bit patterns under 'x', 'f', 'kkt', 'status', 'iters', 'lam_g', 'lam_x', 'lam_p'."""
    import nmpc_amd
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    B = P.shape[0]
    p = torch.as_tensor(P, device=dev).contiguous(); w0 = torch.as_tensor(W0, device=dev).contiguous()
    od = torch.as_tensor(order, device=dev).to(torch.int32).contiguous() if order is not None else None
    ob = torch.as_tensor(F, device=dev).contiguous() if F is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    size = dict(x=B * cfg.n_var, f=B, kkt=B, status=B, iters=B)
    if duals is not None:
        size.update({k: n for k, n, c in (("lam_g", B * cfg.n_g, "g"), ("lam_x", B * cfg.n_var, "x"), ("lam_p", B * 2 * cfg.nx, "p")) if c in duals})
    bufs = {k: (torch.full((2 * GUARD + n,), SENT32, dtype=torch.int32, device=dev) if k in ("status", "iters") else
                torch.full((2 * GUARD + n,), SENT64, dtype=torch.int64, device=dev)) for k, n in size.items()}
    ptr = {k: t.data_ptr() + GUARD * t.element_size() for k, t in bufs.items()}
    if duals is None:
        if ob is not None:
            rc = L.nmpc_solve_batch_obs(h, B, p.data_ptr(), ob.data_ptr(), int(ob.shape[1]), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"],
                                        ptr["kkt"], od.data_ptr() if od is not None else None, stream)
        elif od is not None:
            rc = L.nmpc_solve_batch_ordered(h, B, p.data_ptr(), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"], ptr["kkt"], od.data_ptr(), stream)
        else:
            rc = L.nmpc_solve_batch(h, B, p.data_ptr(), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"], ptr["kkt"], stream)
    else:
        d = nmpc_amd._lib.CDuals(ptr.get("lam_g"), ptr.get("lam_x"), ptr.get("lam_p"))
        rc = L.nmpc_solve_batch_duals(h, B, p.data_ptr(), ob.data_ptr() if ob is not None else None, int(ob.shape[1]) if ob is not None else 0, w0.data_ptr(),
                                      ptr["x"], ptr["f"], ptr["status"], ptr["iters"], ptr["kkt"], od.data_ptr() if od is not None else None, C.byref(d), stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    if rc != 0:
        return None
    out = {}
    for k, t in bufs.items():
        a = t.cpu().numpy()
        sent = np.int64(SENT64) if a.dtype == np.int64 else np.int32(SENT32)
        assert (a[:GUARD] == sent).all() and (a[-GUARD:] == sent).all(), "the call wrote outside its %s output" % k
        out[k] = a[GUARD:-GUARD].copy()
        assert not (out[k] == sent).any(), "the call left elements of %s unwritten" % k
    return out


def _f64(out, cfg, B):
    return dict(x=out["x"].view(np.float64).reshape(B, cfg.n_var), lam_g=out["lam_g"].view(np.float64).reshape(B, cfg.n_g),
                lam_x=out["lam_x"].view(np.float64).reshape(B, cfg.n_var), lam_p=out["lam_p"].view(np.float64).reshape(B, 2 * cfg.nx),
                status=out["status"], f=out["f"].view(np.float64))


def _kkt(L, h, cfg, P, W, LG, LX, F=None, want_grad=True):
    """nmpc_kkt_batch through the raw ABI, guarded outputs: (res [B, 6], grad_lag [B, n_var] or None)"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    B = P.shape[0]
    t = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (P, W, LG, LX)]
    ob = torch.as_tensor(F, device=dev).contiguous() if F is not None else None
    res = torch.full((2 * GUARD + 6 * B,), SENT64, dtype=torch.int64, device=dev)
    grad = torch.full((2 * GUARD + B * cfg.n_var,), SENT64, dtype=torch.int64, device=dev)
    rc = L.nmpc_kkt_batch(h, B, t[0].data_ptr(), ob.data_ptr() if ob is not None else None, int(ob.shape[1]) if ob is not None else 0, t[1].data_ptr(),
                          t[2].data_ptr(), t[3].data_ptr(), res.data_ptr() + 8 * GUARD, grad.data_ptr() + 8 * GUARD if want_grad else None,
                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = []
    for a in (res.cpu().numpy(), grad.cpu().numpy()):
        assert (a[:GUARD] == np.int64(SENT64)).all() and (a[-GUARD:] == np.int64(SENT64)).all(), "nmpc_kkt_batch wrote outside an output"
        out.append(a[GUARD:-GUARD])
    if not want_grad:
        assert (out[1] == np.int64(SENT64)).all()
        return out[0].view(np.float64).reshape(B, 6), None
    assert not (out[1] == np.int64(SENT64)).any()
    return out[0].view(np.float64).reshape(B, 6), out[1].view(np.float64).reshape(B, cfg.n_var)


def _field_of(F, b):
    return None if F is None else (F[b, 0] if F.shape[1] == 1 else F[b])


def _check_multipliers(cfg, P, F, o, nb):
    """Check 1 on instances 0..nb-1 of a solve's output (all of them status 0): numpy residuals within the bounds, the structural zeros, lam_p's
    x0 part.  Returns res [nb, 6]."""
    zg, zx = D.structural_zeros(cfg)
    res = np.empty((nb, 6))
    for b in range(nb):
        res[b], _ = D.residuals(cfg, o["x"][b], P[b], o["lam_g"][b], o["lam_x"][b], _field_of(F, b))
        assert res[b, 0] <= BOUND, ("stat", b, res[b])
        assert res[b, 5] == 0.0, ("sign", b, res[b])
        assert res[b, 4] <= BOUND, ("compl", b, res[b])
        assert (o["lam_g"][b, zg] == 0.0).all() and (o["lam_x"][b, zx] == 0.0).all(), b
        assert np.array_equal(o["lam_p"][b, : cfg.nx].view(np.int64), o["lam_g"][b, : cfg.nx].view(np.int64)), b
    return res


@pytest.mark.parametrize("r", COLUMN_ROWS, ids=[KV.row_id(r) for r in COLUMN_ROWS])
def test_every_column_shape_returns_its_multipliers(built, capsys, r):
    """Every instantiation of the column kernel (named by nmpc_debug_variant before the solve): the multiplier call returns bit for bit the
    point of the existing call, writes inside its three outputs only, and on EVERY instance — all must be status 0, the recipes are screened —
    its multipliers give stat <= 1e-6, sign == 0, compl <= 1e-6 with exact zeros where the convention has them.  Instances beyond the 16
    distinct ones of a tiled batch must repeat them bit for bit (so the numpy check of the 16 covers them) and are all certified on the device."""
    cfg, P, W0, F = KV.inputs(r)
    B, nb = r.B, min(r.B, 16)
    order = np.random.default_rng(3).permutation(B).astype(np.int32) if r.ordered else None
    L, h = _handle(cfg, r.max_iter, B + 3, r.pin)
    try:
        rc, got = _variant(L, h, B, r.ordered, r.obs_field)
        assert rc == 0 and got == r.row, ("the recipe launches another instantiation", r.row, rc, got)
        plain = _solve(L, h, cfg, P, W0, F, order, duals=None)
        out = _solve(L, h, cfg, P, W0, F, order)
        for k in plain:
            assert np.array_equal(plain[k], out[k]), "asking for the multipliers changed " + k
        assert (out["status"] == 0).all(), out["status"]
        o = _f64(out, cfg, B)
        dres, _ = _kkt(L, h, cfg, P, o["x"], o["lam_g"], o["lam_x"], F, want_grad=False)
    finally:
        L.nmpc_destroy(h)
    idx = np.arange(B) % nb
    for k in ("lam_g", "lam_x", "lam_p"):
        assert np.array_equal(o[k].view(np.int64), o[k][idx].view(np.int64)), "a repeated instance got other bits in " + k
    res = _check_multipliers(cfg, P, F, o, nb)
    with capsys.disabled():
        print("\n  variant %s B %d: worst stat %.2e compl %.2e (device, all %d: stat %.2e compl %.2e), largest |lam_g| %.2e"
              % (got, B, res[:, 0].max(), res[:, 4].max(), B, dres[:, 0].max(), dres[:, 4].max(), np.abs(o["lam_g"]).max()), end="")
    assert np.abs(dres[:nb] - res).max() <= 1e-12, (dres[:nb], res)      # the device certificate reproduces the numpy numbers
    assert (dres[:, 0] <= BOUND).all() and (dres[:, 4] <= BOUND).all() and (dres[:, 5] == 0.0).all()


def _oracle(cfg, P, W0, max_iter=400):
    from oracle import oracle_lib as O
    return O.solve_batch(O.make_config(cfg, max_iter=max_iter), P, W0)


OBS3_START = np.array([0.05, 1.6, np.pi / 2])      # below the obstacle at (0, 2.3), facing it; the goal lies behind it
OBS3_GOAL = np.array([0.0, 3.0, np.pi / 2])


@pytest.mark.parametrize("name", ["six_swap", "obs3_facing"])
def test_multipliers_of_binding_rows_are_not_trivially_zero(built, capsys, name):
    """The literal six-robot swap (C6:364-388) and the third scenario from a start facing an obstacle: at the oracle's point at least one pair
    (obstacle) row lies within 1e-6 of its bound and one control on its bound — confirmed on the CPU first — and the GPU's multipliers of
    exactly those rows and controls exceed 1e-3 in magnitude."""
    if name == "six_swap":
        cfg, p, kind = R.cfg_six(20), np.concatenate([R.C6_START, R.C6_GOAL]), "pair"
    else:
        cfg, p, kind = R.cfg_obs3(20), np.concatenate([OBS3_START, OBS3_GOAL]), "obs"
    P, W0 = p[None], R.cold_start(cfg, p[: cfg.nx])[None]
    ref = _oracle(cfg, P, W0)
    assert ref["status"][0] == 0
    lbx, ubx, lbg, _ = R.bounds(cfg)
    g = R.constraints(cfg, ref["x"][0], p)
    rows = D.row_kinds(cfg)[kind]
    act = rows[g[rows] - lbg[rows] <= 1e-6]
    uo = cfg.nx * (cfg.N + 1)
    wu = ref["x"][0][uo:]
    act_u = uo + np.flatnonzero((wu - lbx[uo:] <= 1e-6) | (ubx[uo:] - wu <= 1e-6))
    assert act.size >= 1 and act_u.size >= 1, (name, act.size, act_u.size)
    L, h = _handle(cfg, 400, 1, 0)
    try:
        o = _f64(_solve(L, h, cfg, P, W0), cfg, 1)
    finally:
        L.nmpc_destroy(h)
    assert o["status"][0] == 0 and np.abs(o["x"][0] - ref["x"][0]).max() <= 1e-6
    _check_multipliers(cfg, P, None, o, 1)
    with capsys.disabled():
        print("\n  %s: %d binding %s rows, lam_g there %.3e .. %.3e; %d controls on a bound, |lam_x| there >= %.3e"
              % (name, act.size, kind, o["lam_g"][0, act].min(), o["lam_g"][0, act].max(), act_u.size, np.abs(o["lam_x"][0, act_u]).min()), end="")
    assert (o["lam_g"][0, act] < -1e-3).all(), o["lam_g"][0, act]
    assert (np.abs(o["lam_x"][0, act_u]) > 1e-3).all(), o["lam_x"][0, act_u]
    up = ubx[act_u] - ref["x"][0][act_u] <= 1e-6
    assert (o["lam_x"][0, act_u][up] > 0).all() and (o["lam_x"][0, act_u][~up] < 0).all()


def test_same_multipliers_in_every_shape(built, capsys):
    """Six robots solved by the throughput shape (pin 3), the latency shapes with two and four wavefronts (4, 5) and the library's choice: each
    passes check 1; the largest difference between the shapes' multipliers is printed, not bounded (the shapes sum in different orders)."""
    cfg = R.cfg_six(20)
    P, W0 = Hh.batch(cfg, 16, 6)
    outs = {}
    for pin in (3, 4, 5, 0):
        L, h = _handle(cfg, 400, 16, pin)
        try:
            o = _f64(_solve(L, h, cfg, P, W0), cfg, 16)
        finally:
            L.nmpc_destroy(h)
        assert (o["status"] == 0).all(), (pin, o["status"])
        _check_multipliers(cfg, P, None, o, 16)
        outs[pin] = o
    diff = {k: max(np.abs(outs[a][k] - outs[3][k]).max() for a in (4, 5, 0)) for k in ("lam_g", "lam_x", "lam_p", "x")}
    with capsys.disabled():
        print("\n  six robots, pins 3 / 4 / 5 / 0: largest difference between the shapes " + ", ".join("%s %.2e" % kv for kv in diff.items()), end="")


def _mix3_10():
    return Hh.cfg_mix3(10)


@pytest.mark.parametrize("name", ["two", "three_obstacles"])
def test_lam_p_is_minus_the_gradient_of_the_optimal_cost(built, capsys, name):
    """d f* / d p = -lam_p against central differences of f* in ONE launch: the instance, p +- h e_i and p +- (h/2) e_i for every i (4 n_p + 1
    instances, h = 1e-4), all status 0.  |D_h + lam_p_i| <= 10 |D_h - D_{h/2}| + 1e-6 max(1, |lam_p_i|): the first term is the measured
    truncation and noise of the difference itself, the second the project's parity tolerance."""
    if name == "two":
        cfg, p = R.cfg_two(10), np.concatenate([R.C2_START, R.C2_GOAL])
    else:
        cfg = _mix3_10()
        p = Hh.batch(cfg, 1, 5)[0][0]
    n_p, h_ = 2 * cfg.nx, 1e-4
    P = np.tile(p, (4 * n_p + 1, 1))
    for i in range(n_p):
        P[1 + 4 * i, i] += h_; P[2 + 4 * i, i] -= h_; P[3 + 4 * i, i] += h_ / 2; P[4 + 4 * i, i] -= h_ / 2
    W0 = np.stack([R.cold_start(cfg, q[: cfg.nx]) for q in P])
    L, h = _handle(cfg, 400, P.shape[0], 0)
    try:
        o = _f64(_solve(L, h, cfg, P, W0), cfg, P.shape[0])
    finally:
        L.nmpc_destroy(h)
    assert (o["status"] == 0).all(), o["status"]
    f, lam_p = o["f"], o["lam_p"][0]
    Dh = np.array([(f[1 + 4 * i] - f[2 + 4 * i]) / (P[1 + 4 * i, i] - P[2 + 4 * i, i]) for i in range(n_p)])
    Dh2 = np.array([(f[3 + 4 * i] - f[4 + 4 * i]) / (P[3 + 4 * i, i] - P[4 + 4 * i, i]) for i in range(n_p)])
    err, allow = np.abs(Dh + lam_p), 10.0 * np.abs(Dh - Dh2) + 1e-6 * np.maximum(1.0, np.abs(lam_p))
    with capsys.disabled():
        print("\n  %s: lam_p %s\n    |D_h + lam_p| max %.2e (worst ratio to its allowance %.2f), |D_h - D_h/2| max %.2e"
              % (name, np.array2string(lam_p, precision=4), err.max(), (err / allow).max(), np.abs(Dh - Dh2).max()), end="")
    assert np.abs(lam_p).max() > 1e-3
    assert (err <= allow).all(), (err, allow)


def _random_case(cfg, B, seed, S):
    """random bound-feasible points, random multipliers on EVERY row and variable, a random field: every term of the kernel is exercised"""
    rng = np.random.default_rng(seed)
    lbx, ubx, _, _ = R.bounds(cfg)
    lo, hi = np.maximum(lbx, -2.0), np.minimum(ubx, 2.0)
    W = rng.uniform(lo, hi, (B, cfg.n_var))
    P = rng.uniform(-2.0, 2.0, (B, 2 * cfg.nx))
    LG, LX = rng.standard_normal((B, cfg.n_g)), rng.standard_normal((B, cfg.n_var))
    F = None
    if S:
        F = np.concatenate([rng.uniform(-2.0, 2.0, (B, S, cfg.K, 2)), rng.uniform(0.05, 0.2, (B, S, cfg.K, 1))], axis=3)
    return P, W, LG, LX, F


KKT_CASES = {   # m, N, obstacles, heading bound, pad_rows, field stages S (0: the handle's field, 1, "N"), kernel pin
    "one_thb_obstacles": (1, 7, 2, True, False, 0, 0),
    "two_pad_element_kernel": (2, 5, 0, False, True, 0, 2),
    "two_nopad_field1_hbm_kernel": (2, 5, 2, True, False, 1, 1),
    "three_nopad_fieldN": (3, 6, 2, False, False, "N", 0),
    "six_pad_field1": (6, 5, 2, False, True, 1, 0),
    "six_nopad_obstacles": (6, 4, 2, True, False, 0, 0),
    "ten_pad_hbm_kernel": (10, 4, 0, False, True, 0, 1),
    "ten_nopad_fieldN": (10, 3, 1, True, False, "N", 0),
}


@pytest.mark.parametrize("name", list(KKT_CASES), ids=list(KKT_CASES))
def test_kkt_batch_matches_numpy(built, name):
    """grad_lag elementwise and the six numbers against tests/duals_ref.py to 1e-12, with random multipliers and random points; B = 300 spans
    more than one workgroup of the streaming kernel (300 (N + 1) threads of 256)."""
    m, N, K, thb, pad, S, pin = KKT_CASES[name]
    cfg = R.NLPConfig(**KV._cfg(m, N, int(thb), K, pad))
    B = 300
    P, W, LG, LX, F = _random_case(cfg, B, 11 + m, N if S == "N" else S)
    L, h = _handle(cfg, 10, 4, pin)      # max_batch does not bound nmpc_kkt_batch: it uses no workspace (as nmpc_eval_batch)
    try:
        res, grad = _kkt(L, h, cfg, P, W, LG, LX, F)
        res2, none = _kkt(L, h, cfg, P, W, LG, LX, F, want_grad=False)
    finally:
        L.nmpc_destroy(h)
    assert none is None and np.array_equal(res.view(np.int64), res2.view(np.int64))
    for b in list(range(8)) + [B - 1]:
        rr, gg = D.residuals(cfg, W[b], P[b], LG[b], LX[b], _field_of(F, b))
        assert np.abs(grad[b] - gg).max() <= 1e-12, (b, np.abs(grad[b] - gg).max())
        assert np.abs(res[b] - rr).max() <= 1e-12, (b, res[b], rr)
        assert rr[0] > 0.1 and rr[4] > 0.1 and (rr[5] > 0.1 or cfg.n_g == cfg.nx * (cfg.N + 1))      # nothing near zero: the terms are there
    assert np.isfinite(res).all() and np.isfinite(grad).all()


def test_kkt_batch_propagates_a_nan_and_checks_its_arguments(built):
    cfg = R.NLPConfig(**KV._cfg(2, 4, 0, 2, True))
    P, W, LG, LX, F = _random_case(cfg, 3, 5, 1)
    LG[1, cfg.rows0 + 2] = np.nan
    L, h = _handle(cfg, 10, 4, 0)
    try:
        res, _ = _kkt(L, h, cfg, P, W, LG, LX, F)
        assert np.isnan(res[1, 0]) and np.isfinite(res[[0, 2]]).all()
        import torch
        t = torch.zeros(8, dtype=torch.float64, device="cuda")
        q = t.data_ptr()
        assert L.nmpc_kkt_batch(h, 1, q, None, 0, q, None, q, q, None, None) == -1      # lam_g missing
        assert L.nmpc_kkt_batch(h, 1, q, q, 3, q, q, q, q, None, None) == -1             # a field that is neither static nor per stage
        assert L.nmpc_kkt_batch(h, 1, q, None, 1, q, q, q, q, None, None) == -1          # stages without a field
        assert L.nmpc_kkt_batch(h, 0, None, None, 0, None, None, None, None, None, None) == 0
    finally:
        L.nmpc_destroy(h)


def test_infeasible_x0_returns_zero_rows(built):
    cfg = R.cfg_two(10)
    P, W0 = Hh.batch(cfg, 2, 5)
    P[1, 3:5] = P[1, 0:2] + 0.05      # the second robot inside dmin of the first
    W0[1] = R.cold_start(cfg, P[1, : cfg.nx])
    L, h = _handle(cfg, 400, 2, 0)
    try:
        o = _f64(_solve(L, h, cfg, P, W0), cfg, 2)
    finally:
        L.nmpc_destroy(h)
    assert o["status"].tolist() == [0, 3]
    assert (o["lam_g"][1] == 0).all() and (o["lam_x"][1] == 0).all() and (o["lam_p"][1] == 0).all()
    assert np.abs(o["lam_g"][0]).max() > 1e-3


def test_null_members_and_dispatch_order_leave_the_others_identical(built):
    cfg = Hh.cfg_mix3(10)
    P, W0 = Hh.batch(cfg, 16, 5)
    for pin in (3, 4):
        L, h = _handle(cfg, 400, 16, pin)
        try:
            full = _solve(L, h, cfg, P, W0)
            for sub in ("xp", "gp", "gx", "g", ""):
                part = _solve(L, h, cfg, P, W0, duals=sub)
                for k in part:
                    assert np.array_equal(part[k], full[k]), (pin, sub, k)
            rev = _solve(L, h, cfg, P, W0, order=np.arange(16, dtype=np.int32)[::-1].copy())
            for k in full:
                assert np.array_equal(rev[k], full[k]), (pin, "reversed order", k)
            scr = _solve(L, h, cfg, P, W0, order=np.random.default_rng(1).permutation(16).astype(np.int32))
            for k in full:
                assert np.array_equal(scr[k], full[k]), (pin, "shuffled order", k)
        finally:
            L.nmpc_destroy(h)


def test_step_batch_duals_returns_the_multipliers_of_each_period(built):
    import nmpc_amd
    import torch
    cfg = Hh.cfg_mix3(10)
    P, W0 = Hh.batch(cfg, 16, 5)
    solver = nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=400), max_batch=16)
    p = torch.as_tensor(P, device=solver.device).contiguous(); w = torch.as_tensor(W0, device=solver.device).contiguous()
    order = torch.arange(16, dtype=torch.int32, device=solver.device)
    for period in range(3):
        p0, w0 = p.clone(), w.clone()
        st = solver.step_batch(p, w, order=order if period else None, want_duals=True)
        ref = solver.solve_batch(p0, w0, want_duals=True)
        plain = solver.step_batch(p0.clone(), w0.clone())
        torch.cuda.synchronize()
        for k in ("x", "f", "status", "iters", "kkt", "lam_g", "lam_x", "lam_p"):
            assert torch.equal(st[k], ref[k]), (period, k)
        assert torch.equal(st["x"], plain["x"])
        assert not torch.equal(p, p0) and float(st["lam_g"].abs().max()) > 1e-3


def test_handles_off_the_column_kernel_are_unsupported(built):
    import nmpc_amd
    cfg = R.cfg_two(10)
    P, W0 = Hh.batch(cfg, 2, 5)
    for pin in (1, 2):
        L, h = _handle(cfg, 50, 2, pin)
        try:
            assert _solve(L, h, cfg, P, W0, expect=-2) is None
            assert _solve(L, h, cfg, P, W0, duals=None) is not None
            d = nmpc_amd._lib.CDuals(None, None, None)
            assert L.nmpc_step_batch_duals(h, 0, None, None, None, None, 0, None, None, None, None, None, C.byref(d), None) == -2
        finally:
            L.nmpc_destroy(h)
        s = nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=300), max_batch=1, kernel=pin)
        sol = s(x0=W0[0], p=P[0])
        assert set(sol) == {"x", "f", "g"} and not s.duals_supported()


def test_nlpsol_call_returns_the_three_keys(built):
    import nmpc_amd
    cfg = nmpc_amd.centralized_two_robots(N=10)
    p = np.concatenate([R.C2_START, R.C2_GOAL])
    solver = nmpc_amd.nlpsol("solver", "ipopt", cfg, {"ipopt": {"max_iter": 300}})
    sol = solver(x0=nmpc_amd.cold_start(cfg, p[: cfg.nx]), p=p)
    assert solver.stats()["success"]
    assert sol["lam_g"].shape == (cfg.n_g, 1) and sol["lam_x"].shape == (cfg.n_var, 1) and sol["lam_p"].shape == (cfg.n_p, 1)
    ocfg = R.cfg_two(10)
    res, _ = D.residuals(ocfg, sol["x"], p, sol["lam_g"], sol["lam_x"])
    assert res[0] <= BOUND and res[4] <= BOUND and res[5] == 0.0, res
    pipe = nmpc_amd.PipelinedSolver(cfg, max_batch=2, depth=2)
    r = pipe.solve_batch(p[None], nmpc_amd.cold_start(cfg, p[: cfg.nx])[None], want_duals=True)
    pipe.synchronize()
    assert np.array_equal(r["lam_g"][0].cpu().numpy(), sol["lam_g"][:, 0])
