"""CPU: the oracle's per-instance obstacle field (nmpc_oracle_solve_batch_obs / nmpc_oracle_eval_batch_obs, oracle.oracle_lib.solve_batch_obs /
eval_batch_obs), the checker of the product's *_obs entry points.  Given the config's own field it is the plain oracle bit for bit; its
constraint values are the independent restatement's (tests/moving_obstacles_ref.py) at every team size and row layout; its moving-field
solutions are KKT points of the restated NLP; the stage-0 pre-check reads entry 0; the argument rules are those of include/nmpc.h."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp_ref as R, oracle_lib as O
from tests import helpers as Hh
from tests import moving_obstacles_ref as MO


def _composite(N=25):
    rng = np.random.default_rng(7)
    c = R.cfg_six(N); c.rob_dim = 0.2; c.margin = 0.1
    c.obstacles = [(float(x), float(y), float(r)) for x, y, r in zip(rng.uniform(-1.5, 1.5, 8), rng.uniform(-1.5, 1.5, 8), rng.uniform(0.125, 0.2, 8))]
    return c


def _third(N=100):
    return R.NLPConfig(m=1, N=N, T=0.2, dmin=0.0, v_max=0.2, w_max=1.0, th_max=2 * np.pi, pad_rows=False, rob_dim=0.2, margin=0.1,
                       obstacles=[(-0.6, 3.3, 0.2), (0.6, 3.3, 0.125), (0.0, 2.3, 0.15), (1.0, 2.3, 0.15), (-0.6, 1.3, 0.2), (0.6, 1.3, 0.175)])


def _same(a, b, what):
    for k in ("x", "f", "status", "iters", "kkt"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, np.flatnonzero([not np.array_equal(u, v, equal_nan=True) for u, v in zip(a[k], b[k])])[:20])


@pytest.mark.parametrize("name,mk,B,idx", [("composite", _composite, 48, 4), ("third", _third, 24, 5), ("mix3", Hh.cfg_mix3, 48, 6)])
def test_config_field_as_parameter_is_the_plain_oracle(name, mk, B, idx):
    """The config's field given per instance as S = 1 and as S = N (the entry repeated): x, f, status, iters and kkt equal to the plain
    oracle bit for bit; f and g of eval_batch_obs likewise."""
    ocfg = mk()
    P, W0 = Hh.batch(ocfg, B, idx)
    oc = O.make_config(ocfg, max_iter=2000)
    K, N = ocfg.K, ocfg.N
    f1 = np.broadcast_to(np.array(ocfg.obstacles), (B, K, 3)).copy()
    fN = np.broadcast_to(np.array(ocfg.obstacles), (B, N, K, 3)).copy()
    ref = O.solve_batch(oc, P, W0)
    assert (ref["status"] == 0).mean() >= 0.9, ref["status"]
    _same(O.solve_batch_obs(oc, P, f1, W0), ref, "S=1")
    _same(O.solve_batch_obs(oc, P, fN, W0), ref, "S=N")
    fe, ge = O.eval_batch(oc, P, ref["x"])
    for fld in (f1, fN):
        fo, go = O.eval_batch_obs(oc, P, ref["x"], fld)
        assert np.array_equal(fo, fe) and np.array_equal(go, ge)


EVAL_CFGS = [("m%d" % m, (lambda m=m: MO.team_cfg(m, 6, 3))) for m in range(1, 11)] + [
    ("m4_no_pad_rows", lambda: MO.team_cfg(4, 6, 3, pad_rows=False)),
    ("m4_no_pair_rows", lambda: MO.team_cfg(4, 6, 3, pad_rows=False, pair_rows=False)),
    ("m3_pair_rows_no_pad", lambda: MO.team_cfg(3, 5, 2, pad_rows=False)),
    ("m1_heading_bound", lambda: MO.team_cfg(1, 7, 4, th_max=2 * np.pi)),
]


@pytest.mark.parametrize("name,mk", EVAL_CFGS)
def test_eval_batch_obs_matches_the_restatement(name, mk):
    """g of eval_batch_obs at random w, for moving fields [B, N, K, 3] and static ones [B, K, 3] (a different field per instance), equals
    moving_obstacles_ref.constraints to 1e-12 and f equals nlp_ref.objective, for every team size 1..10 and with pad / pair rows off (the
    obstacle rows' offsets inside a stage block move with M)."""
    cfg = mk()
    B = 6
    P, W0, F = MO.moving_batch(cfg, B, 100 + cfg.m)
    rng = np.random.default_rng(cfg.m)
    W = W0 + rng.normal(0.0, 0.3, W0.shape)
    oc = O.make_config(cfg)
    for fld in (F, F[:, 2]):
        f, g = O.eval_batch_obs(oc, P, W, fld)
        for b in range(B):
            gr = MO.constraints(cfg, W[b], P[b], fld[b])
            assert g[b].shape == gr.shape
            assert np.all(np.abs(g[b] - gr) <= 1e-12 * np.maximum(1.0, np.abs(gr))), (name, b, np.abs(g[b] - gr).max())
            assert abs(f[b] - R.objective(cfg, W[b], P[b])) <= 1e-12 * max(1.0, abs(f[b]))
    # the field is read per instance and per stage: instance 0's field on every instance gives other rows
    _, g0 = O.eval_batch_obs(oc, P, W, np.broadcast_to(F[:1], F.shape))
    assert np.array_equal(g0[0], O.eval_batch_obs(oc, P, W, F)[1][0]) and not np.array_equal(g0[1:], O.eval_batch_obs(oc, P, W, F)[1][1:])


@pytest.mark.parametrize("m,N,K,B", [(6, 10, 4, 512), (2, 20, 3, 128), (1, 40, 6, 64)])
def test_moving_field_solves_are_kkt_points(m, N, K, B):
    """Moving, growing fields (moving_obstacles_ref.moving_batch): >= 99 % status 0 with kkt <= 1e-8, and on a sample of 48 of them the
    independent KKT check of the restated NLP (stationarity <= 1e-6, equality and inequality <= 1e-8, bounds exact) with every obstacle row
    clear at that obstacle's stage position.  The six-robot batch is the one of the GPU test test_moving_obstacles_solve_kkt (seed 7).
    Measured: status 0 on every instance of the three batches."""
    cfg = MO.team_cfg(m, N, K, **({"th_max": 2 * np.pi} if m == 1 else {}))
    P, W0, F = MO.moving_batch(cfg, B, 7)
    r = O.solve_batch_obs(O.make_config(cfg, max_iter=2000), P, F, W0)
    ok = r["status"] == 0
    print(f"m={m}: status 0 on {ok.mean():.4f} of {B}, mean iterations {r['iters'].mean():.2f}")
    assert ok.mean() >= 0.99 and (r["kkt"][ok] <= 1e-8).all()
    for b in np.flatnonzero(ok)[:: max(1, ok.sum() // 48)][:48]:
        k = MO.kkt_report(cfg, r["x"][b], P[b], F[b], tol_active=1e-2)
        assert k["stat"] <= 1e-6 and k["eq"] <= 1e-8 and k["ineq"] <= 1e-8 and k["bnd"] == 0.0, (b, k)
        assert MO.obstacle_values(cfg, r["x"][b], F[b]).min() >= cfg.margin - 1e-8, b
    # a moving field is another problem than its entry 0 held still
    r0 = O.solve_batch_obs(O.make_config(cfg, max_iter=2000), P, F[:, 0], W0)
    assert not np.array_equal(r0["x"], r["x"])


def test_stage0_precheck_reads_entry_0():
    """An x0 covered by entry 0 of its field is status 3 (iterations 0, NaN objective); covered only by entry 1 it is solved (the stage-1
    rows, at X_1, hold it off instead); covered by a static field (S = 1) it is status 3.  The other instances are untouched."""
    cfg = MO.team_cfg(3, 10, 2)
    B = 8
    P, W0, F = MO.moving_batch(cfg, B, 3)
    oc = O.make_config(cfg, max_iter=2000)
    base = O.solve_batch_obs(oc, P, F, W0)
    assert (base["status"] == 0).all()
    e0, e1 = F.copy(), F.copy()
    e0[2, 0, 1] = (P[2, 3], P[2, 4], 0.25)          # entry 0 of obstacle 1 on robot 1 of instance 2
    e1[2, 1, 1] = (P[2, 3], P[2, 4], 0.05)          # entry 1 only, small enough for X_1 to clear it
    a, b = O.solve_batch_obs(oc, P, e0, W0), O.solve_batch_obs(oc, P, e1, W0)
    assert a["status"][2] == 3 and a["iters"][2] == 0 and np.isnan(a["f"][2])
    assert b["status"][2] != 3 and b["iters"][2] > 0
    keep = np.arange(B) != 2
    _same({k: v[keep] for k, v in a.items()}, {k: v[keep] for k, v in base.items()}, "rest of the batch")
    s1 = O.solve_batch_obs(oc, P, e0[:, 0], W0)
    assert s1["status"][2] == 3


def test_argument_errors():
    """NMPC_E_ARG (-1), as nmpc_solve_batch_obs / nmpc_eval_batch_obs: a config without obstacle rows, obs == NULL with B > 0, S neither 1
    nor N.  B = 0 with obs == NULL is accepted."""
    L = O.lib()
    cfg = Hh.cfg_mix3(10)
    oc = O.make_config(cfg)
    B, N, K = 2, cfg.N, cfg.K
    P, W0 = Hh.batch(cfg, B, 6)
    fld = np.ascontiguousarray(np.broadcast_to(np.array(cfg.obstacles), (B, N, K, 3)))
    w = np.empty_like(W0); g = np.empty((B, L.nmpc_oracle_n_g(C.byref(oc)))); f = np.empty(B)
    dp = O._dp

    def solve(c, obs, S, nb=B):
        return L.nmpc_oracle_solve_batch_obs(C.byref(c), nb, dp(P), obs, S, dp(W0), dp(w), None, None, None, None, 1)

    def ev(c, obs, S, nb=B):
        return L.nmpc_oracle_eval_batch_obs(C.byref(c), nb, dp(P), dp(W0), obs, S, dp(f), dp(g))
    for fn in (solve, ev):
        assert fn(oc, dp(fld), N) == 0 and fn(oc, dp(fld), 1) == 0
        for S in (0, 2, N - 1, N + 1, -1):
            assert fn(oc, dp(fld), S) == -1, (fn.__name__, S)
        assert fn(oc, None, 1) == -1
        assert fn(oc, None, 1, nb=0) == 0
    c0 = O.make_config(R.cfg_six(10))
    P6, W6 = Hh.batch(R.cfg_six(10), B, 2)
    assert L.nmpc_oracle_solve_batch_obs(C.byref(c0), B, dp(P6), dp(fld), 1, dp(W6), dp(np.empty_like(W6)), None, None, None, None, 1) == -1
    assert L.nmpc_oracle_eval_batch_obs(C.byref(c0), B, dp(P6), dp(W6), dp(fld), 1, None, None) == -1
    with pytest.raises(AssertionError):
        O.solve_batch_obs(oc, P, fld[:, : N - 1], W0)
