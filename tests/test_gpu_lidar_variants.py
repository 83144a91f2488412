"""-m gpu: every LIDAR solve-kernel instantiation (the table of tests/lidar_variants.py) solves like the CPU oracle at the edges of its shape
handling: ray counts 0..16 around the unroll chunks, horizons around the unroll remainder and the 64-lane stride, one held control and none,
the bound branches, and the two-waves-per-SIMD build one instance beyond its threshold.

Per row: nmpc_debug_lidar_variant() must name the row's instantiation for the recipe's batch (so the launch below runs that instantiation
and no other), then nmpc_lidar_solve_batch through the raw C ABI is compared with oracle_lib.lidar_solve_batch on the same seeded, screened
inputs (tests/test_lidar_variants_host.py), and nmpc_lidar_eval_batch / nmpc_lidar_shift_batch on the same handle with oracle/lidar_ref.py.
Every call is made with its outputs carved out of the middle of larger sentinel-filled arrays on a handle with max_batch = B + 3
(helpers.guarded_call): the bands around every output stay untouched, the inputs come back bit-identical, a second call returns bit-identical
outputs, no output element is left unwritten."""
import ctypes as C

import numpy as np
import pytest

from oracle import lidar_ref as LR
from tests import helpers as Hh
from tests import lidar_variants as LV
from tests.test_gpu_lidar import _product

pytestmark = pytest.mark.gpu

W_TOL = 1e-6
F_RTOL = 1e-6
EVAL_TOL = 1e-12
# Active-set tolerance of lidar_ref.kkt_report, from its own threshold: a point with reported kkt <= 1e-8 has slack x multiplier <= 1e-8 on every
# bound, so a bound further than 1e-8 / 1e-5 = 1e-3 away carries a multiplier below the stationarity threshold of 1e-5 and may be left out of
# the least-squares fit, and a nearer one may not.  (At 1e-4 the ORACLE's own point fails on two rows: N = 65, R = 16, Nc = 32 / 65,
# instance 0, stat 5.1e-5 / 2.5e-5 from a bound 2e-4 away; at 1e-3 the oracle's points pass on the first three converged instances of all
# 254 rows, worst stat 2.2e-6.)  The multipliers of the fit stay sign-constrained.
KKT_ACTIVE = 1e-3
W2_ROWS = [r for r in LV.TABLE if r.inst == (10, 2)]


def _handle(cfg, max_iter, max_batch):
    import nmpc_amd
    L = nmpc_amd._lib.load()
    lbx, ubx, _, _ = LR.bounds(cfg)
    lbx = np.ascontiguousarray(lbx, dtype=np.float64); ubx = np.ascontiguousarray(ubx, dtype=np.float64)
    cc = _product(cfg, max_iter=max_iter).to_c()
    h = C.c_void_p(); dp = C.POINTER(C.c_double)
    nmpc_amd._lib.check(L.nmpc_lidar_create(C.byref(cc), lbx.ctypes.data_as(dp), ubx.ctypes.data_as(dp), max_batch, C.byref(h)), "nmpc_lidar_create")
    return L, h


def _variant(L, h, B):
    import nmpc_amd
    v = nmpc_amd._lib.CDebugLidarVariant()
    rc = L.nmpc_debug_lidar_variant(h, B, C.byref(v))
    return rc, (v.rays, v.waves), v


_THRESHOLD = []


def _two_wave_threshold():
    """the batch size above which a ten-ray handle launches the two-wave build on this device, from the descriptor"""
    if not _THRESHOLD:
        L, h = _handle(LR.LidarConfig(N=1, Nc=1, R=10, aligned_bounds=True), 1, 1)
        try:
            rc, _, v = _variant(L, h, 1)
            assert rc == 0
            _THRESHOLD.append(int(v.two_wave_above))
        finally:
            L.nmpc_lidar_destroy(h)
    return _THRESHOLD[0]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _abi_solve(L, h, cfg, P, W0):
    """nmpc_lidar_solve_batch with guarded outputs, twice"""
    import torch
    dev = _dev()
    B = P.shape[0]
    p = torch.as_tensor(P, device=dev).contiguous(); w0 = torch.as_tensor(W0, device=dev).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = Hh.guarded_call(dict(x=(B * cfg.n_var, "f8"), f=(B, "f8"), kkt=(B, "f8"), status=(B, "i4"), iters=(B, "i4")), [p, w0],
                          lambda ptr: L.nmpc_lidar_solve_batch(h, B, p.data_ptr(), w0.data_ptr(), ptr["x"], ptr["f"], ptr["status"], ptr["iters"], ptr["kkt"], stream))
    out["x"] = out["x"].reshape(B, cfg.n_var)
    return out


def _abi_eval_and_shift(L, h, cfg, P, W):
    import torch
    dev = _dev()
    B = P.shape[0]
    p = torch.as_tensor(P, device=dev).contiguous(); w = torch.as_tensor(W, device=dev).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ev = Hh.guarded_call(dict(f=(B, "f8"), g=(B * cfg.n_g, "f8")), [p, w],
                         lambda ptr: L.nmpc_lidar_eval_batch(h, B, p.data_ptr(), w.data_ptr(), ptr["f"], ptr["g"], stream))
    sh = Hh.guarded_call(dict(w=(B * cfg.n_var, "f8")), [w], lambda ptr: L.nmpc_lidar_shift_batch(h, B, w.data_ptr(), ptr["w"], stream))
    return ev["f"], ev["g"].reshape(B, cfg.n_g), sh["w"].reshape(B, cfg.n_var)


def _eval_point(cfg, B, seed):
    """a point away from any solution: every entry standard normal, the distance states in [0.3, 3] (the 1/d^2 term stays tame)"""
    rng = np.random.default_rng(seed)
    W = rng.normal(size=(B, cfg.n_var))
    W[:, : cfg.ns * (cfg.N + 1)].reshape(B, cfg.N + 1, cfg.ns)[:, :, 3:] = rng.uniform(0.3, 3.0, (B, cfg.N + 1, cfg.R))
    return W


def _pinned_guess(cfg, P, W0):
    """what a solve that stops at stage 0 returns: the guess with X_0 pinned to the pose and the scan of p"""
    w = W0.copy()
    w[:, :3] = P[:, :3]; w[:, 3: 3 + cfg.R] = P[:, 6: 6 + cfg.R]
    return w


@pytest.mark.parametrize("r", LV.TABLE, ids=[LV.row_id(r) for r in LV.TABLE])
def test_lidar_variant_solves_like_the_oracle(built, capsys, r):
    """Descriptor: exactly this row's instantiation for the recipe's batch (a two-wave row: the descriptor's threshold + 1).
    Solve: status equal on every instance; instance 1 (and its repeats) status 3 with the guess returned, X_0 pinned; every other instance
    converged with reported kkt <= 1e-8, the oracle's point (1e-6) and objective (1e-6 relative) on EVERY instance, iteration counts equal on
    at least 0.9 of the row and within 3 elsewhere, X_0 equal to p bit for bit, bounds held to 1e-12, lidar_ref.kkt_report on the first three
    converged instances.  eval / shift on the same handle: f and g at 1e-12 against lidar_ref, the shifted guess bit-exact."""
    import torch
    n = LV.distinct(r)
    B = r.B if r.B is not None else _two_wave_threshold() + 1
    cfg, P, W0 = LV.inputs(r, B)
    L, h = _handle(cfg, r.max_iter, B + 3)
    try:
        rc, got, v = _variant(L, h, B)
        assert rc == 0 and got == r.inst, ("the recipe launches another instantiation", r.inst, rc, got)
        if r.B is None:      # include/nmpc_lidar.h: the one-wave build "up to one robot per SIMD (4 x the device's compute units)"
            assert v.two_wave_above == B - 1 == 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count, v.two_wave_above
        assert v.threads == 64 and v.lds_bytes == 8 * (16 * (cfg.N + 1) + 16 * cfg.Nc + 12 * cfg.N + 32)      # the LDS need stated in include/nmpc_lidar.h
        assert _variant(L, h, B + 4)[0] == -1 and _variant(L, h, -1)[0] == -1 and L.nmpc_debug_lidar_variant(h, B, None) == -1
        out = _abi_solve(L, h, cfg, P, W0)
        nb = min(B, 16)
        We = _eval_point(cfg, nb, 3)
        f, g, wn = _abi_eval_and_shift(L, h, cfg, P[:nb], We)
    finally:
        L.nmpc_lidar_destroy(h)
    ref_n = LV.oracle_solve(cfg, P[:n], W0[:n], r.max_iter)
    ref = {k: a[np.arange(B) % n] for k, a in ref_n.items()}      # a batch beyond the distinct instances repeats them: so does the reference
    stopped = np.arange(B) % n == 1
    conv = ~stopped
    dw = np.max(np.abs(out["x"] - ref["x"]), axis=1)
    rel = np.abs(out["f"] - ref["f"]) / np.maximum(1.0, np.abs(ref["f"]))
    it_eq = out["iters"] == ref["iters"]
    with capsys.disabled():
        print("\n  %s variant %s lds %d B %d: max |dw| %.1e, max rel df %.1e, iterations equal %d/%d (largest gap %d), hip %d..%d oracle %d..%d"
              % (LV.row_id(r), got, v.lds_bytes, B, dw[conv].max(), rel[conv].max(), it_eq[conv].sum(), conv.sum(),
                 np.abs(out["iters"] - ref["iters"])[conv].max(), out["iters"][conv].min(), out["iters"][conv].max(), ref["iters"][conv].min(),
                 ref["iters"][conv].max()), end="")
    assert (out["status"] == ref["status"]).all(), (out["status"], ref["status"])
    assert (out["status"][stopped] == 3).all() and (out["status"][conv] == 0).all(), out["status"]
    assert np.array_equal(out["x"][stopped], _pinned_guess(cfg, P, W0)[stopped]) and (out["iters"][stopped] == 0).all()
    assert (out["kkt"][conv] <= 1e-8).all(), out["kkt"][conv].max()
    assert (dw[conv] <= W_TOL).all(), (np.flatnonzero(conv & (dw > W_TOL)), dw.max())
    assert (rel[conv] <= F_RTOL).all(), (np.flatnonzero(conv & (rel > F_RTOL)), rel[conv].max())
    assert it_eq[conv].mean() >= 0.9, (out["iters"], ref["iters"])
    assert (np.abs(out["iters"] - ref["iters"])[conv] <= 3).all(), (out["iters"], ref["iters"])
    assert np.array_equal(out["x"][:, :3], P[:, :3]) and np.array_equal(out["x"][:, 3: 3 + cfg.R], P[:, 6: 6 + cfg.R])
    lbx, ubx, _, _ = LR.bounds(cfg)
    assert (out["x"][conv] >= lbx - 1e-12).all() and (out["x"][conv] <= ubx + 1e-12).all()
    for b in np.flatnonzero(conv)[:3]:
        k = LR.kkt_report(cfg, out["x"][b], P[b], tol_active=KKT_ACTIVE)
        assert k["stat"] < 1e-5 and k["eq"] < 1e-9 and k["bnd"] == 0.0, (b, k)
    # eval and shift
    fo = np.array([LR.objective(cfg, We[b], P[b]) for b in range(nb)])
    go = np.stack([LR.constraints(cfg, We[b], P[b]) for b in range(nb)])
    assert np.abs(g - go).max() <= EVAL_TOL * max(1.0, np.abs(go).max()), np.abs(g - go).max()
    assert np.max(np.abs(f - fo) / np.maximum(1.0, np.abs(fo))) < EVAL_TOL
    assert np.array_equal(wn, np.stack([LR.shift_guess(cfg, w) for w in We]))      # pure data movement: bit-exact


@pytest.mark.parametrize("r", W2_ROWS, ids=[LV.row_id(r) for r in W2_ROWS])
def test_lidar_result_does_not_depend_on_the_register_budget(built, capsys, r):
    """include/nmpc_lidar.h: the one-wave and the two-wave build of the ten-ray kernel return the same results.  On one handle the first T
    instances of the recipe are solved with B = T (T = the descriptor's threshold: the descriptor must say one wave) and the first T + 1 with
    B = T + 1 (two waves).  On the common T instances: statuses and iteration counts equal, the points within 100 x the oracle's own
    rounding-level spread on this recipe (lidar_variants.screen / budget_tolerance; at least 1e-12).
    Measured on an MI355X (T = 1024): every output of the two builds is bit-identical on all eight recipes (the spilled values of the
    two-wave build are stored and reloaded, not recomputed), so bit identity of x, f, kkt, status and iters is asserted on top."""
    T = _two_wave_threshold()
    cfg, P, W0 = LV.inputs(r, T + 1)
    L, h = _handle(cfg, r.max_iter, T + 4)
    try:
        rc1, got1, _ = _variant(L, h, T)
        rc2, got2, _ = _variant(L, h, T + 1)
        assert (rc1, got1) == (0, (10, 1)) and (rc2, got2) == (0, (10, 2)), (got1, got2)
        one = _abi_solve(L, h, cfg, P[:T], W0[:T])
        two = _abi_solve(L, h, cfg, P, W0)
    finally:
        L.nmpc_lidar_destroy(h)
    tol = LV.budget_tolerance(LV.screen(r).spread)
    conv = one["status"] == 0
    d = np.max(np.abs(one["x"] - two["x"][:T]), axis=1)
    same_bits = np.array([np.array_equal(a, b) for a, b in zip(one["x"].view(np.int64), two["x"][:T].view(np.int64))])
    with capsys.disabled():
        print("\n  %s T %d: bit-identical points %d/%d (%.4f), max |dw| %.2e (tolerance %.1e, oracle spread %.1e), f bit-identical %d/%d"
              % (LV.row_id(r), T, same_bits.sum(), T, same_bits.mean(), d[conv].max(), tol, LV.screen(r).spread,
                 (one["f"].view(np.int64) == two["f"][:T].view(np.int64)).sum(), T), end="")
    assert np.array_equal(one["status"], two["status"][:T]) and np.array_equal(one["iters"], two["iters"][:T])
    assert conv.sum() == T - len(np.flatnonzero(np.arange(T) % LV.distinct(r) == 1))
    assert (d[conv] <= tol).all(), (d[conv].max(), tol)
    assert same_bits[~conv].all()      # the early return moves data only
    for k in ("x", "f", "kkt"):
        assert np.array_equal(one[k].view(np.int64), two[k][:T].view(np.int64)), "the two register budgets return other bits in %s" % k


def test_lidar_descriptor_threshold_is_one_robot_per_simd(built):
    """the threshold the descriptor reports is 4 x the device's compute units on a ten-ray handle; any other ray count has one build"""
    import torch
    T = _two_wave_threshold()
    assert T == 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    L, h = _handle(LR.LidarConfig(N=3, Nc=1, R=9, aligned_bounds=True), 1, T + 2)
    try:
        rc, got, v = _variant(L, h, T + 2)
        assert rc == 0 and got == (-1, 1) and v.two_wave_above == 2 ** 31 - 1
        assert _variant(L, h, 0)[0] == 0
    finally:
        L.nmpc_lidar_destroy(h)
