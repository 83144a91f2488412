"""-m gpu: every instantiation of sens_kernel<MS> (csrc/nmpc_sens.hip) against tests/sens_ref.py on the constructed points of
tests/sens_points.py — binding pair and obstacle rows at every stage, controls at both bounds, x / y and heading bounds, the bounds of X_N,
defect multipliers of size: a dropped or mis-indexed term moves the answer by 1000 x the bound or more (tests/test_sens_points_host.py).

One handle per table row and two calls: gains="N" with dp on [the points; the points with the entries that carry nothing zeroed], then
gains=1 on the same batch in reverse order.  Bounds as tests/test_gpu_sens.py: parity within 100 x that point's spread + 1e-12 relative to
max|G| / max|dw|, the linearised dynamics of dw to 1e-12.  The verdict batches mix instances built for verdict 2, 1 and 0 with clean
neighbours; the reference says which verdict each gets."""
import numpy as np
import pytest

from tests import helpers as Hh
from tests import sens_points as SP
from tests import sens_ref as S

pytestmark = pytest.mark.gpu

ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
_CACHE = {}


def _np(t):
    return None if t is None else t.cpu().numpy()


def _solver(cfg, max_batch):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=10, pair_rows=cfg.pair_rows), max_batch=max_batch)


def _call(s, r, pts, gains):
    obs = np.stack([pt.obs for pt in pts]) if r.field else None      # an "own" row calls with (NULL, 0): the handle's field
    out = s.sens_batch(np.stack([pt.p for pt in pts]), np.stack([pt.w for pt in pts]), np.stack([pt.lam_g for pt in pts]),
                       np.stack([pt.lam_x for pt in pts]), dp=np.stack([pt.dp for pt in pts]), gains=gains, obstacles=obs)
    return {k: _np(v) for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def ran(i):
    """row i: its handle, the two calls and the reference with its spread per point — once per session"""
    if i in _CACHE:
        return _CACHE[i]
    r = ROWS[i]
    pts = SP.points(r); n = len(pts)
    batch = pts + [SP.zero_nulls(r.cfg, pt) for pt in pts]
    s = _solver(r.cfg, 2 * n + 2)
    full = _call(s, r, batch, "N")
    back = _call(s, r, batch[::-1], 1)
    ref = [SP.reference(r, pt) for pt in pts]
    spread = [S.spread(r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=pt.dp) for pt in pts]
    _CACHE[i] = dict(row=r, pts=pts, n=n, solver=s, full=full, back=back, ref=ref, spread=spread)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_parity_against_numpy(i):
    o = ran(i); r = o["row"]; cfg = r.cfg
    G, dw, info = o["full"]["gains"], o["full"]["dw"], o["full"]["info"]
    assert G.shape == (2 * o["n"], cfg.N, cfg.nu, cfg.nx) and dw.shape == (2 * o["n"], cfg.n_var)
    worst = (0.0, 0.0)
    for b, pt in enumerate(o["pts"]):
        ref, (sg, sw) = o["ref"][b], o["spread"][b]
        assert info[b] == ref["info"] == 0, (b, info[b], ref["info"])
        eg = np.abs(G[b] - ref["gains"]).max() / np.abs(ref["gains"]).max()
        ew = np.abs(dw[b] - ref["dw"]).max() / np.abs(ref["dw"]).max()
        print("%s %d: gains %.2e (spread %.2e), dw %.2e (spread %.2e), max|G| %.2e" % (SP.row_id(r), b, eg, sg, ew, sw, np.abs(ref["gains"]).max()))
        worst = max(worst, (max(eg, ew), max(sg, sw)))
        assert eg <= 100.0 * sg + 1e-12, (b, eg, sg)
        assert ew <= 100.0 * sw + 1e-12, (b, ew, sw)
        assert np.array_equal(dw[b, : cfg.nx], pt.dp[: cfg.nx]), b      # dw[:n_x] is dx0, copied
        res = S.linearised_defect(cfg, pt.w, dw[b])
        assert res <= 1e-12 * max(1.0, np.abs(dw[b]).max()), (b, res)
    print("%s: largest parity error %.2e at spread %.2e" % (SP.row_id(r), worst[0], worst[1]))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_rows_that_carry_nothing_change_no_bit(i):
    """stage-0 pair / obstacle rows (one of them violated, with a multiplier), the initial block and its pad rows, lam_x of X_0 and of an unbounded
    heading hold arbitrary non-zero values in the points: zeroing them returns the same bits, and the violated stage-0 row gives info 0"""
    o = ran(i); n = o["n"]
    f = o["full"]
    assert (f["info"] == 0).all(), f["info"]
    assert np.array_equal(_bits(f["gains"][n:]), _bits(f["gains"][:n])) and np.array_equal(_bits(f["dw"][n:]), _bits(f["dw"][:n]))
    viol = [SP.stage0_violation(o["row"].cfg, pt) for pt in o["pts"]]
    assert all(v is None or v for v in viol), viol


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_reversed_batch_and_first_stage_gains(i):
    """the same batch in reversed order gives each instance's bits back, and gains=1 is stage 0 of gains="N" bit for bit"""
    o = ran(i); f, k = o["full"], o["back"]
    assert k["gains"].shape == (2 * o["n"], 1, o["row"].cfg.nu, o["row"].cfg.nx)
    assert np.array_equal(k["info"][::-1], f["info"])
    assert np.array_equal(_bits(k["dw"][::-1]), _bits(f["dw"]))
    assert np.array_equal(_bits(k["gains"][::-1, 0]), _bits(f["gains"][:, 0]))


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_in_a_mixed_batch(r):
    """each verdict case is one instance between clean points: its outputs are zeros and its neighbours keep the bits of the parity call"""
    i = ROWS.index(r)
    o = ran(i); cfg = r.cfg
    cases = SP.verdict_cases(r, o["pts"][0])[1:]
    batch, clean = [], []
    for c, (name, pt, want) in enumerate(cases):
        clean.append(c % o["n"])
        batch += [o["pts"][clean[-1]], pt]
    s = _solver(cfg, len(batch))
    got = _call(s, r, batch, "N")
    refs = [SP.reference(r, pt) for _, pt, _ in cases]
    info = got["info"]
    print("verdicts", info[1::2].tolist(), "reference", [x["info"] for x in refs])
    for c, (name, pt, want) in enumerate(cases):
        b = 2 * c + 1
        assert info[b] == refs[c]["info"] == want, (name, info[b], refs[c]["info"], want)
        if want:
            assert not got["gains"][b].any() and not got["dw"][b].any(), name
        else:      # the pair row of the wrong sign: no Sigma, its Hessian term stays in
            sg, sw = S.spread(cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs, dp=pt.dp)
            eg = np.abs(got["gains"][b] - refs[c]["gains"]).max() / np.abs(refs[c]["gains"]).max()
            ew = np.abs(got["dw"][b] - refs[c]["dw"]).max() / np.abs(refs[c]["dw"]).max()
            print("%s: gains %.2e (spread %.2e), dw %.2e (spread %.2e)" % (name, eg, sg, ew, sw))
            assert eg <= 100.0 * sg + 1e-12 and ew <= 100.0 * sw + 1e-12, (name, eg, sg, ew, sw)
        a = clean[c]
        assert info[2 * c] == 0
        assert np.array_equal(_bits(got["gains"][2 * c]), _bits(o["full"]["gains"][a])) and np.array_equal(_bits(got["dw"][2 * c]), _bits(o["full"]["dw"][a])), name
