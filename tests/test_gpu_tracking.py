"""-m gpu: pose references per stage in the cost and in the KKT certificate (nmpc_eval_batch_ref / nmpc_kkt_batch_ref, reference= of
NmpcSolver.eval_batch / kkt_batch).

The checker is tests/tracking_ref.py — oracle.nlp_ref with the cost restated per stage — and its scipy-SLSQP fixtures
(tests/golden/slsqp_track.npz).  Bounds: 1e-12 relative between the device's numbers and numpy's (two fp64 summation orders of O(1) terms, the
tolerance of the eval pins and of nmpc_kkt_batch against numpy in tests/test_gpu_duals.py); exact equality where the reference is the goal and
only read from another place (g, and every output of the KKT kernel, which adds nothing across threads but maxima)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import duals_ref as D
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO
from tests import tracking_ref as TR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slsqp_track.npz")


def _solver(cfg, B, pin=0, max_iter=600):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=max_iter), max_batch=B, kernel=pin)


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _nan_goal(P, nx):
    """p with the xs half NaN: a *_ref call may not read it"""
    Q = P.copy()
    Q[:, nx:] = np.nan
    return Q


# ---- eval against the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 6, 10])
def test_eval_matches_the_restatement(built, m):
    """f of random w against random moving paths equals tracking_ref.objective to 1e-12 relative, for N in {2, 3, 20}, with and without a moving
    obstacle field, on the library's own kernel choice and on a handle pinned to kernel 1; g does not depend on the reference: it equals the
    g of eval_batch / eval_batch(obstacles=) exactly.  S = 1 is checked against the one-row restatement as well."""
    B = 5
    rng = np.random.default_rng(100 + m)
    worst = 0.0
    for N in (2, 3, 20):
        for K in (0, 2):
            cfg = MO.team_cfg(m, N, K)
            if K:
                P, _, F = MO.moving_batch(cfg, B, 300 + N)
            else:
                P, _ = Hh.batch(cfg, B, 300 + N); F = None
            W = rng.uniform(-2.0, 2.0, (B, cfg.n_var))
            REF = rng.uniform(-2.0, 2.0, (B, N, cfg.nx))
            Pn = _nan_goal(P, cfg.nx)
            for pin in (0, 1):
                s = _solver(cfg, B, pin)
                f, g = (t.cpu().numpy() for t in s.eval_batch(Pn, W, obstacles=F, reference=REF))
                f1, g1 = (t.cpu().numpy() for t in s.eval_batch(Pn, W, obstacles=F, reference=REF[:, 0]))
                _, g0 = s.eval_batch(P, W, obstacles=F)
                g0 = g0.cpu().numpy()
                assert np.array_equal(g, g0) and np.array_equal(g1, g0)
                for b in range(B):
                    for got, ref in ((f[b], REF[b]), (f1[b], REF[b, 0])):
                        want = TR.objective(cfg, W[b], ref)
                        worst = max(worst, abs(got - want) / abs(want))
                        assert abs(got - want) <= 1e-12 * abs(want), (m, N, K, pin, b, got, want)
                assert np.max(np.abs(f - f1)) > 1e-3      # the path is read: its frozen row 0 gives another cost
    print("m = %d: worst relative error of f %.2e" % (m, worst))


# ---- the fixtures: SLSQP's optimal cost -----------------------------------------------------------------------------------------------------
def test_eval_reproduces_the_cost_of_the_slsqp_fixtures(built):
    """f of eval_batch(reference=) at the stored SLSQP solutions equals the stored optimal cost to 1e-12 relative, and g there is feasible
    to the generator's limits (1e-9)."""
    z = np.load(GOLDEN)
    for name, cfg in TR.families().items():
        P, REF, wp, fp = (z[name + k] for k in ("_p", "_ref", "_w_pol", "_f_pol"))
        f, g = (t.cpu().numpy() for t in _solver(cfg, len(P)).eval_batch(P, wp, reference=REF))
        assert (np.abs(f - fp) <= 1e-12 * np.abs(fp)).all(), (name, f, fp)
        _, _, lbg, ubg = R.bounds(cfg)
        assert (g >= lbg - 1e-9).all() and (g <= ubg + 1e-9).all(), name


# ---- the KKT certificate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 4, 6, 10])
def test_kkt_certificate_reads_the_reference(built, m):
    """nmpc_kkt_batch_ref on random (w, lam_g, lam_x) and random moving paths, N in {2, 5, 20}, with a moving obstacle field up to six robots,
    on the library's own kernel choice and on a handle pinned to kernel 1: grad_lag equals numpy's grad f + J' lam_g + lam_x with the
    restatement's gradient, and res the numpy residuals (tests/duals_ref.py; only `stat` depends on the reference), to 1e-12 relative to the
    size of the terms.  With the goal as the reference, one row or N equal rows, every output equals nmpc_kkt_batch's exactly."""
    B = 4
    rng = np.random.default_rng(200 + m)
    for N in (2, 5, 20):
        cfg = MO.team_cfg(m, N, 2 if m <= 6 else 0)
        if cfg.K:
            P, _, F = MO.moving_batch(cfg, B, 400 + N)
        else:
            P, _ = Hh.batch(cfg, B, 400 + N); F = None
        W = rng.uniform(-2.0, 2.0, (B, cfg.n_var))
        LG = rng.uniform(-1.0, 1.0, (B, cfg.n_g)); LX = rng.uniform(-1.0, 1.0, (B, cfg.n_var))
        REF = rng.uniform(-2.0, 2.0, (B, N, cfg.nx))
        xs = P[:, cfg.nx:]
        Pn = _nan_goal(P, cfg.nx)
        for pin in (0, 1):
            s = _solver(cfg, B, pin)
            res, grad = (t.cpu().numpy() for t in s.kkt_batch(Pn, W, LG, LX, obstacles=F, want_grad=True, reference=REF))
            for b in range(B):
                fld = None if F is None else F[b]
                rr, gg = D.residuals(cfg, W[b], P[b], LG[b], LX[b], fld)      # with the goal's gradient: replace it by the path's
                gg = gg - R.grad_objective(cfg, W[b], P[b]) + TR.grad_objective(cfg, W[b], REF[b])
                scale = max(1.0, np.abs(gg).max())
                assert np.abs(grad[b] - gg).max() <= 1e-12 * scale, (m, N, pin, b, np.abs(grad[b] - gg).max())
                assert abs(res[b, 0] - np.abs(gg).max()) <= 1e-12 * scale
                assert np.abs(res[b, 1:] - rr[1:]).max() <= 1e-12 * max(1.0, np.abs(rr[1:]).max()), (res[b], rr)
            plain = [t.cpu().numpy() for t in s.kkt_batch(P, W, LG, LX, obstacles=F, want_grad=True)]
            assert np.abs(plain[1] - grad).max() > 1e-3      # the rows are read
            for ref in (xs, np.repeat(xs[:, None, :], N, axis=1)):
                same = [t.cpu().numpy() for t in s.kkt_batch(Pn, W, LG, LX, obstacles=F, want_grad=True, reference=ref)]
                assert np.array_equal(_bits(same[0]), _bits(plain[0])) and np.array_equal(_bits(same[1]), _bits(plain[1]))


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(built):
    """-1: ref_stages neither 1 nor N, ref NULL with B > 0, a field on a handle without obstacle rows, NULL inputs; 0: an empty batch, and
    every handle — a pin to kernel 2 included."""
    import torch
    cfg = MO.team_cfg(2, 5, 0)
    P, W0 = Hh.batch(cfg, 2, 9)
    for pin in (0, 2):
        s = _solver(cfg, 2, pin)
        dev = s.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        p, w, rf = t(P), t(W0), t(np.repeat(P[:, None, cfg.nx:], cfg.N, axis=1))
        lg, lx = torch.zeros((2, s.n_g), dtype=torch.float64, device=dev), torch.zeros((2, s.n_var), dtype=torch.float64, device=dev)
        f, g = torch.empty(2, dtype=torch.float64, device=dev), torch.empty((2, s.n_g), dtype=torch.float64, device=dev)
        res = torch.empty((2, 6), dtype=torch.float64, device=dev)
        ob = torch.zeros((2, 1, 1, 3), dtype=torch.float64, device=dev)
        ev = lambda B, rp, S, o=None, os_=0: s.lib.nmpc_eval_batch_ref(s._h, B, p.data_ptr(), w.data_ptr(), rp, S, o, os_, f.data_ptr(), g.data_ptr(), s._stream())
        kk = lambda B, rp, S, o=None, os_=0: s.lib.nmpc_kkt_batch_ref(s._h, B, p.data_ptr(), rp, S, o, os_, w.data_ptr(), lg.data_ptr(), lx.data_ptr(), res.data_ptr(), None, s._stream())
        for call in (ev, kk):
            assert call(2, rf.data_ptr(), cfg.N) == 0 and call(2, rf.data_ptr(), 1) == 0
            assert call(2, rf.data_ptr(), 2) == -1 and call(2, rf.data_ptr(), 0) == -1      # ref_stages = 2 with N = 5; 0
            assert call(2, None, 1) == -1                                                      # NULL ref
            assert call(0, None, 1) == 0                                                       # an empty batch reads nothing
            assert call(-1, rf.data_ptr(), 1) == -1
            assert call(2, rf.data_ptr(), cfg.N, ob.data_ptr(), 1) == -1                       # a field on a handle without obstacle rows
        assert s.lib.nmpc_eval_batch_ref(s._h, 2, None, w.data_ptr(), rf.data_ptr(), 1, None, 0, f.data_ptr(), g.data_ptr(), s._stream()) == -1
        assert s.lib.nmpc_kkt_batch_ref(s._h, 2, p.data_ptr(), rf.data_ptr(), 1, None, 0, w.data_ptr(), None, lx.data_ptr(), res.data_ptr(), None, s._stream()) == -1
        torch.cuda.synchronize()
