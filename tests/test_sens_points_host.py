"""CPU: the table of sens_kernel instantiations (tests/sens_points.py) is exactly the set of sens_kernel symbols in the built gfx950 code object,
and the constructed points the GPU test runs are good inputs on the reference alone: the recursion of tests/sens_ref.py is its dense solve on
every point, every term class of the barrier KKT system is visible at 1000 x the parity bound on at least two points of every recipe, an
emulated wrong pair index is, the entries that carry nothing carry nothing, and the verdict batch has the verdicts it was built for.

The parity bound is the project's: 100 x the spread of the recursion against itself under +-4 ulp moves of (w, lam_g, lam_x), + 1e-12,
relative to max|G| (max|dw|)."""
import functools
import re
from collections import Counter

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import kernel_variants as KV
from tests import moving_obstacles_ref as MO
from tests import sens_points as SP
from tests import sens_ref as S

ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
VISIBLE = 1000.0


def test_table_equals_the_sens_kernels_of_the_code_object(built, tmp_path):
    got = []
    for name in Hh.kernel_notes(tmp_path):
        m = re.search(r"^_ZN4nmpc11sens_kernelILi(\d+)ELi0EEE", name)
        if m:
            ms = int(m.group(1))
            got.append((ms % 16, ms // 16))
            continue
        assert not re.search(r"sens_(adjoint_|fwd_)?kernel(?!ILi\d+ELi[012]EEE)", name), "sens kernel with an unknown template signature: " + name
    rows = [(r.m, r.field) for r in ROWS]
    assert len(got) == len(set(got)) == 20 and len(rows) == len(set(rows)) == 20, (sorted(got), sorted(rows))
    assert set(got) == set(rows), (sorted(set(got) - set(rows)), sorted(set(rows) - set(got)))
    assert Counter(m for m, _ in rows) == Counter({m: 2 for m in range(1, 11)})


def test_table_covers_what_the_kernel_branches_on(built):
    cf = {(r.m, r.field): r for r in ROWS}
    for r in ROWS:
        assert r.cfg.m == r.m and bool(r.field) == (r.kind in ("static", "moving")) and (r.cfg.K > 0) == (r.kind is not None), SP.row_id(r)
        assert r.cfg.K in (0, 1, 2, 8) and (2 <= r.cfg.N <= 4 or r.cfg.N == 12), SP.row_id(r)
        # the sensitivity call needs a column-kernel handle: the library's own plan for the recipe's batch is one
        rc, got, _, _ = KV.variant_of_config(KV.c_config(r.cfg, 10), 0, 256, 2 * SP.NPOINTS, 0, 0)
        assert rc == 0 and got[0] == 3, (SP.row_id(r), rc, got)
    for m in range(1, 11):
        assert any(r.cfg.pair_rows for r in ROWS if r.m == m), m
    assert len({r.m for r in ROWS if r.m > 1 and not r.cfg.pair_rows}) >= 2
    assert any(not r.cfg.pair_rows and r.cfg.K and r.m > 1 for r in ROWS)      # the NX + npairs + rob * K + o indexing with npairs = 0
    assert {r.cfg.pad_rows for r in ROWS if r.m > 1} == {True, False}
    assert len({r.m for r in ROWS if r.m > 1 and np.isfinite(r.cfg.th_max)}) >= 3
    assert cf[(10, 1)].cfg.K == 8 and any(r.cfg.K == 8 and r.m <= 4 for r in ROWS)
    assert len({r.m for r in ROWS if r.kind == "static"}) >= 3 and len({r.m for r in ROWS if r.kind == "moving"}) >= 3
    assert len([r for r in ROWS if r.kind == "own"]) >= 3
    assert sum(r.cfg.N == 12 for r in ROWS) == 1
    assert {SP.row_id(r) for r in SP.VERDICT_ROWS} == {"m3_moving_field", "m10_moving_field"}


@functools.lru_cache(maxsize=None)
def screened(i):
    """per point of row i: the reference, its verdict on the inputs, recursion against dense solve and the spread"""
    r = ROWS[i]
    out = []
    for pt in SP.points(r):
        a = (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        ref = S.stage_recursion(*a, dp=pt.dp)
        eg, sg, ew, sw = S.recursion_against_dense(*a, dp=pt.dp)
        out.append(dict(ref=ref, bad=S.kkt_system(*a)[2], eg=eg, sg=sg, ew=ew, sw=sw, bg=100.0 * sg + 1e-12, bw=100.0 * sw + 1e-12))
    return out


def _factor(r, o, pt2):
    """how far the reference moves when it gets pt2, in units of the point's parity bound (gains or dw, whichever shows more)"""
    dg, dw = SP.deviation(o["ref"], SP.reference(r, pt2))
    return max(dg / o["bg"], dw / o["bw"])


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_points_pass_on_the_reference_alone(i):
    r = ROWS[i]; cfg = r.cfg
    pts = SP.points(r)
    assert 4 <= len(pts) <= 6
    for n, (pt, o) in enumerate(zip(pts, screened(i))):
        ref = o["ref"]
        print("%s %d: gains %.2e (spread %.2e), dw %.2e (spread %.2e), min eig %.2e, max|G| %.2e" % (
            SP.row_id(r), n, o["eg"], o["sg"], o["ew"], o["sw"], ref["min_eig"], np.abs(ref["gains"]).max()))
        assert ref["info"] == 0 and ref["min_eig"] >= 1e-6, (n, ref["info"], ref["min_eig"])
        assert not o["bad"], n
        assert o["eg"] <= o["bg"] and o["ew"] <= o["bw"], (n, o["eg"], o["sg"], o["ew"], o["sw"])
        assert S.linearised_defect(cfg, pt.w, ref["dw"]) <= 1e-12 * max(1.0, np.abs(ref["dw"]).max()), n
        assert abs(np.linalg.norm(pt.dp) - 1.0) <= 1e-12
        assert pt.obs is None or pt.obs.shape == ((cfg.K, 3) if r.kind == "static" else (cfg.N, cfg.K, 3))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_points_are_what_the_construction_says(i):
    """the slacks and multipliers the constructor promises, read back from (w, lam_g, lam_x) with the oracle's g and bounds"""
    r = ROWS[i]; cfg = r.cfg; N, nx = cfg.N, cfg.nx
    lbx, ubx, lbg, _ = R.bounds(cfg)
    sides = set()
    xn_points = zeros = tiny = 0
    for pt in SP.points(r):
        g = R.constraints(cfg, pt.w, pt.p) if pt.obs is None else MO.constraints(cfg, pt.w, pt.p, pt.obs)
        s = g - lbg
        for k in range(1, N):
            o = cfg.rows0 + k * cfg.rows_k + nx
            sp, lp = s[o: o + cfg.M], pt.lam_g[o: o + cfg.M]
            assert (sp > 0).all()      # no pair row is violated
            if cfg.M:
                b = lp <= -0.005
                assert b.sum() >= min(2, cfg.m - 1) and (sp[b] >= 0.9e-6 * cfg.dmin ** 2).all() and (sp[b] <= 1.1e-1 * cfg.dmin ** 2).all(), (k, sp[b])
                assert (lp[~b] <= 0).all() and (lp[~b] >= -1e-4).all()
                zeros += int((lp == 0).sum()); tiny += int(((lp < 0) & ~b).sum())
            so, lo = s[o + cfg.M: o + cfg.M + cfg.m * cfg.K].reshape(cfg.m, cfg.K), pt.lam_g[o + cfg.M: o + cfg.M + cfg.m * cfg.K].reshape(cfg.m, cfg.K)
            assert (so > 0).all()
            for q in range(cfg.K):      # every obstacle presses on one robot
                b = lo[:, q] <= -0.005
                assert b.sum() == 1 and 0.9e-7 <= so[b, q][0] <= 1.1e-2, (k, q, so[:, q], lo[:, q])
        U = slice((N + 1) * nx, cfg.n_var)
        su, sl, lu = (ubx - pt.w)[U], (pt.w - lbx)[U], pt.lam_x[U]
        up, dn = lu >= 0.01, lu <= -0.01
        assert up.any() and dn.any() and (su[up] <= 1.1e-2).all() and (sl[dn] <= 1.1e-2).all() and (su > 0).all() and (sl > 0).all()
        assert lu.size < 20 or 0.15 <= (up | dn).mean() <= 0.6, (up | dn).mean()      # about a third
        X = slice(nx, (N + 1) * nx)
        act = np.flatnonzero((np.abs(pt.lam_x[X]) >= 0.01) & (np.arange(nx, (N + 1) * nx) % 3 != 2)) + nx
        assert act.size == 1      # one robot under an x or y bound
        j = act[0]
        slack = (ubx[j] - pt.w[j]) if pt.lam_x[j] > 0 else (pt.w[j] - lbx[j])
        assert 0.9e-5 <= slack <= 1.1e-2, slack
        sides.add((j % 3, pt.lam_x[j] > 0)); xn_points += j >= N * nx
        if np.isfinite(cfg.th_max):
            for k in range(1, N + 1):
                th = np.arange(k * nx + 2, (k + 1) * nx, 3)
                b = np.abs(pt.lam_x[th]) >= 0.01
                sl_ = np.where(pt.lam_x[th] > 0, cfg.th_max - pt.w[th], pt.w[th] + cfg.th_max)
                assert b.sum() == 1 and 0.9e-6 <= sl_[b][0] <= 1.1e-2, (k, sl_)
        assert ((ubx - pt.w)[X] > 0).all() and ((pt.w - lbx)[X] > 0).all()
        viol = SP.stage0_violation(cfg, pt)
        assert viol is None or viol      # a violated stage-0 row that carries a multiplier, where the configuration has stage-0 rows
        mg, mx = SP.null_masks(cfg)
        assert (pt.lam_g[mg] != 0).all() and (pt.lam_x[mx] != 0).all()
    assert cfg.M < 3 or (zeros and tiny), (zeros, tiny)      # the pair rows that do not bind: exact zeros on some, tiny multipliers on the rest
    assert sides == {(0, True), (0, False), (1, True), (1, False)} and xn_points >= 2, (sides, xn_points)


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_every_term_class_is_visible(i):
    r = ROWS[i]
    pts, scr = SP.points(r), screened(i)
    for cls in SP.classes_of(r.cfg):
        f = sorted(_factor(r, o, SP.zero_class(r.cfg, pt, cls)) for pt, o in zip(pts, scr))
        print("%s %-8s: factors %s" % (SP.row_id(r), cls, " ".join("%.1e" % v for v in f)))
        assert f[-2] >= VISIBLE, (cls, f)
    want = {"defect", "control", "xy", "xN"} | ({"pair"} if r.cfg.M else set()) | ({"obstacle"} if r.cfg.K else set()) | (
        {"heading"} if np.isfinite(r.cfg.th_max) else set())
    assert set(SP.classes_of(r.cfg)) == want


@pytest.mark.parametrize("i", [i for i, r in enumerate(ROWS) if r.cfg.M and r.m >= 3], ids=[SP.row_id(r) for r in ROWS if r.cfg.M and r.m >= 3])
def test_a_wrong_pair_index_is_visible(i):
    r = ROWS[i]
    f = []
    for pt, o in zip(SP.points(r), screened(i)):
        dg, _ = SP.deviation(o["ref"], SP.reference(r, SP.reverse_pairs(r.cfg, pt)))
        f.append(dg / o["bg"])
    print("%s: gains moved by %s x the bound" % (SP.row_id(r), " ".join("%.1e" % v for v in f)))
    assert min(f) >= VISIBLE, f


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_rows_that_carry_nothing_carry_nothing(i):
    r = ROWS[i]
    for pt, o in zip(SP.points(r), screened(i)):
        z = SP.reference(r, SP.zero_nulls(r.cfg, pt))
        assert z["info"] == 0
        assert np.array_equal(z["gains"].view(np.int64), o["ref"]["gains"].view(np.int64)) and np.array_equal(z["dw"].view(np.int64), o["ref"]["dw"].view(np.int64))


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdict_batch_on_the_reference(r):
    cases = SP.verdict_cases(r, SP.points(r)[0])
    names = [c[0] for c in cases]
    assert len(names) == len(set(names)) == 11
    for name, pt, want in cases:
        ref = SP.reference(r, pt)
        assert ref["info"] == want, (name, ref["info"], want)
        if want:
            assert not ref["gains"].any() and not ref["dw"].any(), name
        if name.startswith("indefinite"):
            assert ref["min_eig"] <= -1.0, ref["min_eig"]
        if name == "pair row of the wrong sign":
            assert ref["min_eig"] >= 1e-6
            base = SP.reference(r, SP.points(r)[0])
            assert SP.deviation(base, ref)[0] > 1e-3      # the row that lost its Sigma was a binding one
    assert Counter(c[2] for c in cases) == Counter({2: 8, 1: 1, 0: 2})
