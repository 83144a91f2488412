"""-m gpu: nmpc_sens_update_batch_multi_duals (csrc/nmpc_sens_dual_multi.hip), NmpcSolver.sens_update_multi / plan_jacobian with want_duals and
AdvancedStepController.correct_scenarios(update_duals=True) / commit_scenario.

Every instantiation of dual_dirs_kernel<MS> against tests/sens_dual_ref.stage_duals per direction (tests/sens_dual_multi_ref.py) on the constructed
points of tests/sens_points.py.  With c = nmpc_query(NMPC_QUERY_SENS_DIRS_PER_PASS) the calls run at D in {1, c + 1, 64}: the six distinct
directions of a point stand round-robin in the D slots under a seeded permutation (tests/sens_multi_ref.slots), and every slot is held to the
reference of its direction by the project's bound — tests/sens_dual_ref.parity(...)["worst"] <= 1: 100 x that direction's spread + 1e-12, for
the whole outputs and per stage block — and alpha_dual to bounds["a"]; two directions exchanged are at least 1000 bounds apart
(tests/test_sens_dual_multi_host.py).  dlam_p: the x0 part bit-equal to dlam_g[:n_x], the xs part against 2 Q (sum_k dX_k - N dxs) formed in
numpy from the device's own dw within the summation bound 4 (N + 2) 2^-53 2 q (sum_k |dX_k| + N |dxs|).  Then the bit-level properties, the zero
direction, the verdict batches, the argument errors, the workspace, the single-direction call, the Jacobian of the multipliers and the
controller."""
import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import sens_dual_multi_ref as DM
from tests import sens_dual_ref as DR
from tests import sens_multi_ref as MR
from tests import sens_points as SP
from tests import sens_update_ref as UR

pytestmark = pytest.mark.gpu

ROWS = SP.SENS_TABLE
IDS = [SP.row_id(r) for r in ROWS]
NEW = ("dlam_g", "dlam_x", "dlam_p", "alpha_dual")
OUT = ("dw", "alpha") + NEW
_CACHE = {}
BIT_EQUAL = {}      # row id -> (entries of dlam_g, dlam_x bit-equal to nmpc_sens_update_batch_duals, entries)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _solver(cfg, max_batch, **kw):
    import nmpc_amd
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, max_iter=10, pair_rows=cfg.pair_rows), max_batch=max_batch, **kw)


def _product_solver(cfg, max_batch, **kw):
    import nmpc_amd
    solver_kw = {k: kw.pop(k) for k in ("kernel",) if k in kw}
    return nmpc_amd.NmpcSolver(Hh.to_product_cfg(cfg, pair_rows=cfg.pair_rows, **kw), max_batch=max_batch, **solver_kw)


def _point_arrays(r, pts):
    obs = np.stack([pt.obs for pt in pts]) if r.field else None      # an "own" row calls with (NULL, 0): the handle's field, no dobs
    return [np.stack([getattr(pt, k) for pt in pts]) for k in ("p", "w", "lam_g", "lam_x")], obs


def _call(s, r, pts, stacks, want_duals=True, **kw):
    """stacks: per point (dp [D, n_p], dobs [D, ...] or None, rhs [D, n_var])"""
    a, obs = _point_arrays(r, pts)
    dobs = None if stacks[0][1] is None else np.stack([x[1] for x in stacks])
    out = s.sens_update_multi(*a, dp=np.stack([x[0] for x in stacks]), dobs=dobs, rhs=np.stack([x[2] for x in stacks]), obstacles=obs, want_duals=want_duals, **kw)
    return {k: _np(v) for k, v in out.items()}


def _raw(s, r, pts, stacks, want):
    """the C call itself with the outputs named in `want` (dw always) and NULL for the others, every output between guard bands
    (tests/helpers.guarded_call: nothing written outside, every element written, a second call the same bits): {name: array}, info included"""
    import torch
    B = len(pts); D = stacks[0][0].shape[0]; cfg = r.cfg
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=s.device)
    ptr = lambda x: None if x is None else x.data_ptr()
    (p, w, lg, lx), obs = _point_arrays(r, pts)
    obs = t(obs)
    S_ = 0 if obs is None else (1 if obs.dim() == 3 else cfg.N)
    a = [t(p), t(w), t(lg), t(lx)]
    dp_, rh_ = t(np.stack([x[0] for x in stacks])), t(np.stack([x[2] for x in stacks]))
    do_ = None if stacks[0][1] is None else t(np.stack([x[1] for x in stacks]))
    size = dict(dw=B * D * cfg.n_var, alpha=B * D, dlam_g=B * D * cfg.n_g, dlam_x=B * D * cfg.n_var, dlam_p=B * D * 2 * cfg.nx, alpha_dual=B * D)
    outs = {k: (size[k], "f8") for k in ("dw",) + tuple(want)}
    outs["info"] = (B, "i4")

    def call(q):
        return s.lib.nmpc_sens_update_batch_multi_duals(s._h, B, D, ptr(a[0]), ptr(obs), S_, ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(dp_), ptr(do_), ptr(rh_), q["dw"],
                                                        q.get("alpha"), q.get("dlam_g"), q.get("dlam_x"), q.get("dlam_p"), q.get("alpha_dual"), q["info"], s._stream())
    got = Hh.guarded_call(outs, a + [x for x in (obs, dp_, do_, rh_) if x is not None], call)
    return {k: (v.reshape(B, D, -1) if v.size > B * D else (v.reshape(B, D) if k != "info" else v)) for k, v in got.items()}


def _slot_seed(r, D):
    return 100 * r.seed + D


def ran(i):
    """row i: its handle, the call at D in {1, c + 1, 64} on the row's points, and the stacked reference — once per session"""
    if i in _CACHE:
        return _CACHE[i]
    r = ROWS[i]
    pts = SP.points(r); n = len(pts)
    s = _solver(r.cfg, 2 * n + 20)
    c = s.sens_dirs_per_pass
    assert c == 64 - 5 * r.m
    calls = {}
    for D in sorted({1, c + 1, 64}):
        sl = MR.slots(D, _slot_seed(r, D))
        stacks = [MR.stack(r, k, sl) for k in range(n)]
        calls[D] = dict(slots=sl, stacks=stacks, out=_call(s, r, pts, stacks))
    ref = [DM.reference(r, k) for k in range(n)]
    _CACHE[i] = dict(row=r, pts=pts, n=n, solver=s, c=c, calls=calls, ref=ref)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_parity_of_every_slot_against_numpy(i):
    o = ran(i); r = o["row"]; cfg = r.cfg
    mg, mx = SP.null_masks(cfg)
    mg = mg.copy(); mg[: cfg.nx] = False      # the initial block carries dnu_init
    rows = DR.S.ineq_rows(cfg)
    worst = (0.0, 0.0, 0)
    for D, call in o["calls"].items():
        out = call["out"]
        assert out["dlam_g"].shape == (o["n"], D, cfg.n_g) and out["dlam_x"].shape == (o["n"], D, cfg.n_var)
        assert out["dlam_p"].shape == (o["n"], D, 2 * cfg.nx) and out["alpha_dual"].shape == (o["n"], D)
        for b, pt in enumerate(o["pts"]):
            assert out["info"][b] == 0
            for slot, d in enumerate(call["slots"]):
                ref = o["ref"][b][d]; bd = ref["bd"]
                g, x, ad = out["dlam_g"][b, slot], out["dlam_x"][b, slot], out["alpha_dual"][b, slot]
                e = DR.parity(cfg, g, x, ref, bd)
                ea = abs(ad - ref["alpha_dual"]) / ref["alpha_dual"]
                worst = max(worst, (max(e["worst"], ea / bd["a"]), ea, D))
                assert ref["info"] == 0 and e["worst"] <= 1.0, (D, b, slot, d, e, bd)
                assert ea <= bd["a"], (D, b, slot, d, ea, bd["a"])
                assert 0.0 < ad <= 1.0
                # the structural zeros are exact
                assert not g[mg].any() and not x[mx].any() and g[: cfg.nx].any(), (D, b, slot)
                assert not g[rows][pt.lam_g[rows] >= 0.0].any() and not x[pt.lam_x == 0.0].any(), (D, b, slot)
                assert not np.signbit(g[g == 0.0]).any() and not np.signbit(x[x == 0.0]).any(), (D, b, slot)
    print("%s (c = %d, D in %s): largest error %.3f of its bound (alpha_dual %.2e, at D = %d)" % (SP.row_id(r), o["c"], sorted(o["calls"]), worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_dlam_p_is_the_change_of_lam_p(i):
    o = ran(i); r = o["row"]; cfg = r.cfg; nx = cfg.nx
    worst = 0.0
    for D, call in o["calls"].items():
        out = call["out"]
        assert np.array_equal(_bits(out["dlam_p"][:, :, :nx]), _bits(out["dlam_g"][:, :, :nx])), D
        for b in range(o["n"]):
            dirs = MR.directions(r, b)
            for slot, d in enumerate(call["slots"]):
                dp = dirs[d][0]
                want = DM.dlam_p(cfg, out["dw"][b, slot], out["dlam_g"][b, slot], dp)
                tol = DM.dlam_p_tol(cfg, out["dw"][b, slot], dp)
                err = np.abs(out["dlam_p"][b, slot, nx:] - want[nx:])
                worst = max(worst, float((err / tol).max()))
                assert (err <= tol).all() and np.abs(want[nx:]).max() > 0.0, (D, b, slot, err.max(), tol.min())
    print("%s: xs part of dlam_p at most %.3f of the summation bound" % (SP.row_id(r), worst))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_same_bits_in_every_slot_and_d_reversed_repeated_and_with_outputs_left_out(i):
    o = ran(i); r = o["row"]
    first = {}      # (point, direction) -> bits of every output where the direction was first seen
    for D, call in o["calls"].items():
        out = call["out"]
        for b in range(o["n"]):
            for slot, d in enumerate(call["slots"]):
                got = [_bits(out[k][b, slot: slot + 1]) for k in OUT]
                want = first.setdefault((b, d), got)
                for k, x, y in zip(OUT, got, want):
                    assert np.array_equal(x, y), (D, b, slot, d, k)
    call = o["calls"][64]; f = call["out"]
    back = _call(o["solver"], r, o["pts"][::-1], call["stacks"][::-1])
    again = _call(o["solver"], r, o["pts"], call["stacks"])
    assert np.array_equal(back["info"][::-1], f["info"]) and np.array_equal(again["info"], f["info"])
    for key in OUT:
        assert np.array_equal(_bits(back[key][::-1]), _bits(f[key])), key
        assert np.array_equal(_bits(again[key]), _bits(f[key])), key
    # dw, alpha and info are those of the call without multipliers
    plain = _call(o["solver"], r, o["pts"], call["stacks"], want_duals=False)
    assert set(plain) == {"dw", "alpha", "info"} and np.array_equal(plain["info"], f["info"])
    for key in ("dw", "alpha"):
        assert np.array_equal(_bits(plain[key]), _bits(f[key])), key
    # every output in turn left out, every new output alone, and none of them: the bits of the full call, between guard bands
    D = o["c"] + 1; call = o["calls"][D]; f = call["out"]
    every = ("alpha",) + NEW
    for want in [tuple(k for k in every if k != x) for x in every] + [(x,) for x in NEW] + [()]:
        got = _raw(o["solver"], r, o["pts"], call["stacks"], want)
        assert np.array_equal(got["info"], f["info"]), want
        for key in ("dw",) + want:
            assert np.array_equal(_bits(got[key]), _bits(f[key])), (want, key)


def test_a_zero_direction_among_others():
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); o = ran(ROWS.index(r)); cfg = r.cfg
    call = o["calls"][o["c"] + 1]
    stacks = []
    for dp, dobs, rhs in call["stacks"]:
        dp, dobs, rhs = dp[:5].copy(), dobs[:5].copy(), rhs[:5].copy()
        dp[2] = 0.0; dobs[2] = 0.0; rhs[2] = 0.0
        stacks.append((dp, dobs, rhs))
    got = _call(o["solver"], r, o["pts"], stacks)
    assert (got["info"] == 0).all()
    assert (got["alpha_dual"][:, 2] == 1.0).all() and (got["alpha"][:, 2] == 1.0).all()
    for key in ("dw", "dlam_g", "dlam_x", "dlam_p"):
        assert (got[key][:, 2] == 0.0).all(), key
    for key in OUT:      # the neighbours are those of the parity call
        for slot in (0, 1, 3, 4):
            assert np.array_equal(_bits(got[key][:, slot]), _bits(call["out"][key][:, slot])), (key, slot)


@pytest.mark.parametrize("r", SP.VERDICT_ROWS, ids=[SP.row_id(r) for r in SP.VERDICT_ROWS])
def test_verdicts_in_a_mixed_batch(r):
    """each verdict case is one instance between clean points: all D slots of it are zeros with alpha_dual = 0, and its neighbours keep the bits
    of the parity call"""
    i = ROWS.index(r)
    o = ran(i); cfg = r.cfg
    D = o["c"] + 1
    par = o["calls"][D]; sl = par["slots"]
    cases = SP.verdict_cases(r, o["pts"][0])[1:]
    batch, stacks, clean = [], [], []
    for c, (name, pt, want) in enumerate(cases):
        a = c % o["n"]; clean.append(a)
        batch += [o["pts"][a], pt]
        stacks += [par["stacks"][a], par["stacks"][0]]      # the case is point 0 moved: it takes point 0's directions
    s = _solver(cfg, len(batch))
    got = _call(s, r, batch, stacks)
    dirs0 = MR.directions(r, 0)
    for c, (name, pt, want) in enumerate(cases):
        b = 2 * c + 1
        a = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        ref0 = DR.stage_duals(*a, dp=dirs0[0][0], dobs=dirs0[0][1], rhs=dirs0[0][2])
        assert got["info"][b] == ref0["info"] == want, (name, got["info"][b], ref0["info"], want)
        if want:
            for key in ("dw", "dlam_g", "dlam_x", "dlam_p"):
                assert not got[key][b].any(), (name, key)
            assert (got["alpha_dual"][b] == 0.0).all() and (got["alpha"][b] == 0.0).all() and got["alpha_dual"][b].shape == (D,), name
        else:      # the pair row of the wrong sign: no Sigma and no multiplier step on it, its Hessian term stays in
            for d in range(MR.NDIRS):
                kw = dict(dp=dirs0[d][0], dobs=dirs0[d][1], rhs=dirs0[d][2])
                ref = DR.stage_duals(*a, **kw)
                bd = DR.bounds(DR.spread(*a, **kw))
                for slot in [k for k, x in enumerate(sl) if x == d]:
                    e = DR.parity(cfg, got["dlam_g"][b, slot], got["dlam_x"][b, slot], ref, bd)
                    ea = abs(got["alpha_dual"][b, slot] - ref["alpha_dual"]) / ref["alpha_dual"]
                    assert e["worst"] <= 1.0 and ea <= bd["a"], (name, d, slot, e, ea, bd)
        a = clean[c]
        assert got["info"][2 * c] == 0
        for key in OUT:
            assert np.array_equal(_bits(got[key][2 * c]), _bits(par["out"][key][a])), (name, key)


def test_argument_errors_leave_the_outputs_as_they_were():
    import torch
    r = next(x for x in ROWS if x.kind == "moving" and x.m == 3); o = ran(ROWS.index(r)); cfg = r.cfg; s = o["solver"]
    B, D = 2, 3
    d = s.device
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=d)
    p, w, lg, lx, dp, rh = t(B, 2 * cfg.nx), t(B, cfg.n_var), t(B, cfg.n_g), t(B, cfg.n_var), t(B, 65, 2 * cfg.nx), t(B, 65, cfg.n_var)
    ob, dob = t(B, cfg.N, cfg.K, 3), t(B, 65, cfg.N, cfg.K, 3)
    MARK, IMARK = 0x7FF4DEADBEEF0123, 0x5A5A5A5A
    m = lambda *shape: torch.full(shape, MARK, dtype=torch.int64, device=d)
    dw, al, dg, dx, dpp, ad = m(B, 65, cfg.n_var), m(B, 65), m(B, 65, cfg.n_g), m(B, 65, cfg.n_var), m(B, 65, 2 * cfg.nx), m(B, 65)
    info = torch.full((B,), IMARK, dtype=torch.int32, device=d)
    new = (dg, dx, dpp, ad)
    ptr = lambda x: None if x is None else x.data_ptr()

    def raw(lib_s, B_, D_, p_, obs_, S_, w_, lg_, lx_, dp_, dob_, rh_, dw_, al_, info_, new_=new):
        rc = lib_s.lib.nmpc_sens_update_batch_multi_duals(lib_s._h, B_, D_, ptr(p_), ptr(obs_), S_, ptr(w_), ptr(lg_), ptr(lx_), ptr(dp_), ptr(dob_), ptr(rh_),
                                                          ptr(dw_), ptr(al_), ptr(new_[0]), ptr(new_[1]), ptr(new_[2]), ptr(new_[3]), ptr(info_), lib_s._stream())
        torch.cuda.synchronize()
        assert all((x == MARK).all() for x in (dw, al) + new) and (info == IMARK).all(), "an argument error wrote to an output"
        return rc
    ok = (p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, info)
    assert raw(s, B, 0, *ok) == -1                                                     # D = 0
    assert raw(s, B, 65, *ok) == -1                                                    # D beyond NMPC_SENS_MAX_DIRS
    assert raw(s, B, -1, *ok) == -1
    assert raw(s, B, D, p, ob, cfg.N, w, lg, lx, dp, dob, rh, None, al, info) == -1    # dw is required
    assert raw(s, B, D, p, None, 0, w, lg, lx, dp, dob, rh, dw, al, info) == -1        # dobs without obs
    assert raw(s, s.max_batch + 1, D, *ok) == -1
    for k in range(4):      # null p, w, lam_g, lam_x — with all, with each and with none of the new outputs
        a = [p, w, lg, lx]; a[k] = None
        for new_ in [new, (None,) * 4] + [tuple(x if n == q else None for n, x in enumerate(new)) for q in range(4)]:
            assert raw(s, B, D, a[0], ob, cfg.N, a[1], a[2], a[3], dp, dob, rh, dw, al, info, new_) == -1, k
    assert raw(s, B, D, p, ob, cfg.N, w, lg, lx, dp, dob, rh, dw, al, None) == -1
    assert raw(s, B, D, p, ob, 2, w, lg, lx, dp, dob, rh, dw, al, info) == -1          # obs_stages neither 1 nor N
    assert raw(s, B, D, p, None, cfg.N, w, lg, lx, dp, None, rh, dw, al, info) == -1   # obs_stages without a field
    assert raw(s, 0, D, None, None, 0, None, None, None, None, None, None, dw, None, None) == 0
    k1 = _product_solver(R.cfg_two(8), 4, kernel=1)
    c2 = R.cfg_two(8)
    assert raw(k1, 0, D, None, None, 0, None, None, None, None, None, None, dw, None, None) == -2
    assert raw(k1, B, D, t(B, 2 * c2.nx), None, 0, t(B, c2.n_var), t(B, c2.n_g), t(B, c2.n_var), t(B, D, 2 * c2.nx), None, None, dw, al, info) == -2
    with pytest.raises(ValueError):
        s.sens_update_multi(_np(p), _np(w), _np(lg), _np(lx), dobs=_np(dob[:, :D]), want_duals=True)      # dobs without obstacles=
    with pytest.raises(ValueError):
        s.sens_update_multi(_np(p), _np(w), _np(lg), _np(lx), dp=_np(dp), want_duals=True)                # D = 65


@pytest.mark.parametrize("cfg", [R.cfg_two(8), R.cfg_six(6), R.cfg_ten(5)], ids=["m2", "m6", "m10"])
def test_solve_multi_duals_solve_returns_the_first_solves_bits(cfg):
    B, D = 4, 64
    P, W0 = Hh.batch(cfg, B, 11)
    s = _product_solver(cfg, B)
    before = s.workspace_bytes
    a = s.solve_batch(P, W0, want_duals=True)
    rng = np.random.default_rng(5)
    up = s.sens_update_multi(P, a["x"], a["lam_g"], a["lam_x"], dp=0.02 * UR._weights(rng, (B, D, 2 * cfg.nx)), rhs=UR._weights(rng, (B, D, cfg.n_var)), want_duals=True)
    b = s.solve_batch(P, W0, want_duals=True)
    assert up["dlam_g"].shape == (B, D, cfg.n_g) and up["dlam_p"].shape == (B, D, 2 * cfg.nx) and s.workspace_bytes == before
    for key in ("x", "f", "kkt", "lam_g", "lam_x", "lam_p"):
        assert np.array_equal(_bits(_np(a[key])), _bits(_np(b[key]))), key
    assert np.array_equal(_np(a["iters"]), _np(b["iters"])) and np.array_equal(_np(a["status"]), _np(b["status"]))


@pytest.mark.parametrize("i", range(20), ids=IDS)
def test_agrees_with_the_single_direction_call(i):
    """direction 0 is the input of tests/test_gpu_sens_dual.py: nmpc_sens_update_batch_duals on it and the slot that holds it agree to the sum of
    the two bounds (both are held to the same reference); how many entries are bit-equal is printed, a record"""
    o = ran(i); r = o["row"]; s = o["solver"]; cfg = r.cfg
    a, obs = _point_arrays(r, o["pts"])
    d0 = [MR.directions(r, k)[0] for k in range(o["n"])]
    single = s.sens_update_batch(*a, dp=np.stack([x[0] for x in d0]), dobs=None if d0[0][1] is None else np.stack([x[1] for x in d0]),
                                 rhs=np.stack([x[2] for x in d0]), obstacles=obs, want_duals=True)
    sg, sx, sa = _np(single["dlam_g"]), _np(single["dlam_x"]), _np(single["alpha_dual"])
    call = o["calls"][64]; slot = call["slots"].index(0)
    mg, mx, ma = call["out"]["dlam_g"][:, slot], call["out"]["dlam_x"][:, slot], call["out"]["alpha_dual"][:, slot]
    for b in range(o["n"]):
        ref = o["ref"][b][0]; bd = ref["bd"]
        two = {k: 2.0 * v for k, v in bd.items()}
        e = DR.parity(cfg, mg[b], mx[b], dict(dlam_g=sg[b], dlam_x=sx[b]), two)
        assert e["worst"] <= 1.0 and abs(ma[b] - sa[b]) <= two["a"] * ref["alpha_dual"], (b, e, two)
    BIT_EQUAL[SP.row_id(r)] = (int((_bits(mg) == _bits(sg)).sum()) + int((_bits(mx) == _bits(sx)).sum()), mg.size + mx.size, int((_bits(ma) == _bits(sa)).sum()), ma.size)
    print("%s: bit-equal to nmpc_sens_update_batch_duals: %d of %d dlam entries, %d of %d alpha_dual values" % ((SP.row_id(r),) + BIT_EQUAL[SP.row_id(r)]))
    if len(BIT_EQUAL) == 20:
        print("all rows: bit-equal to nmpc_sens_update_batch_duals: %d of %d dlam entries, %d of %d alpha_dual values" % tuple(np.array(list(BIT_EQUAL.values())).sum(axis=0)))


# ---- the Jacobian of the multipliers
JAC_ROWS = [i for i, r in enumerate(ROWS) if r.field and r.m in (1, 3, 6, 10)]      # the rows of tests/test_gpu_sens_multi.py's Jacobian test


@pytest.mark.parametrize("i", JAC_ROWS, ids=[IDS[i] for i in JAC_ROWS])
def test_plan_jacobian_with_duals_wrt_p(i):
    o = ran(i); r = o["row"]; cfg = r.cfg; s = o["solver"]
    pt = o["pts"][1]
    a, obs = _point_arrays(r, [pt])
    plain = s.plan_jacobian(*a, obstacles=obs)
    out = s.plan_jacobian(*a, obstacles=obs, want_duals=True)
    n_p = 2 * cfg.nx
    Jg, Jx, Jp = _np(out["J_lam_g"])[0], _np(out["J_lam_x"])[0], _np(out["J_lam_p"])[0]
    assert set(plain) == {"J", "info"} and np.array_equal(_bits(_np(plain["J"])), _bits(_np(out["J"]))) and _np(out["info"])[0] == 0
    assert Jg.shape == (cfg.n_g, n_p) and Jx.shape == (cfg.n_var, n_p) and Jp.shape == (n_p, n_p)
    assert np.array_equal(_bits(Jp[: cfg.nx]), _bits(Jg[: cfg.nx]))
    args = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
    worst = 0.0
    for c in range(n_p):
        dp = np.eye(n_p)[c]
        ref = DR.stage_duals(*args, dp=dp)
        bd = DR.bounds(DR.spread(*args, dp=dp))
        e = DR.parity(cfg, Jg[:, c], Jx[:, c], ref, bd)
        worst = max(worst, e["worst"])
        assert ref["info"] == 0 and e["worst"] <= 1.0, (c, e, bd)
        want = DM.dlam_p(cfg, _np(out["J"])[0][:, c], Jg[:, c], dp)
        assert (np.abs(Jp[cfg.nx:, c] - want[cfg.nx:]) <= DM.dlam_p_tol(cfg, _np(out["J"])[0][:, c], dp)).all(), c
    print("%s: the columns of J_lam_g, J_lam_x within %.3f of their bounds" % (SP.row_id(r), worst))


def test_plan_jacobian_with_duals_wrt_obstacles():
    """a static field (6 columns): the columns against stage_duals on the unit directions of the field"""
    i = ROWS.index(next(r for r in ROWS if r.kind == "static" and r.m == 2))
    o = ran(i); r = o["row"]; cfg = r.cfg; s = o["solver"]
    pt = o["pts"][2]
    a, obs = _point_arrays(r, [pt])
    out = s.plan_jacobian(*a, obstacles=obs, wrt="obstacles", want_duals=True)
    n = pt.obs.size
    Jg, Jx = _np(out["J_lam_g"])[0], _np(out["J_lam_x"])[0]
    assert Jg.shape == (cfg.n_g, n) and Jx.shape == (cfg.n_var, n) and "J_lam_p" not in out and _np(out["info"])[0] == 0
    args = (cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
    for c in range(n):
        dobs = np.eye(n)[c].reshape(pt.obs.shape)
        ref = DR.stage_duals(*args, dobs=dobs)
        e = DR.parity(cfg, Jg[:, c], Jx[:, c], ref, DR.bounds(DR.spread(*args, dobs=dobs)))
        assert ref["info"] == 0 and e["worst"] <= 1.0, (c, e)


# ---- the controller
def _six_with_a_field():
    cfg = R.cfg_six(8)
    cfg.obstacles = [(0.1, -0.2, 0.15)]
    return cfg


def _scenario_setup(B=3, D=3):
    """the six-robot configuration, batch and scenarios of tests/test_gpu_sens_multi.py's controller test"""
    cfg = _six_with_a_field()
    P, W0 = Hh.batch(cfg, B, 23)
    obs = np.tile(np.asarray(cfg.obstacles, float)[None], (B, 1, 1))
    rng = np.random.default_rng(9)
    amp = np.array([2e-3, 2e-3, 0.3])      # the last scenario is far enough for a step limit
    x0c = P[:, None, : cfg.nx] + amp[None, :, None] * rng.standard_normal((B, D, cfg.nx))
    obc = obs[:, None] + 2e-3 * rng.standard_normal((B, D) + obs.shape[1:])
    return cfg, P, W0, obs, x0c, obc


def _scenario_tolerances(cfg, tau, base, dp, dobs):
    """of one correction from the primal-dual point base = (p, w, lam_g, lam_x, obs), for two device results that are both held to the numpy
    reference: the tolerance of tests/test_gpu_sens_multi.py's controller test, (100 x spread + 1e-12) x max|d| x step, extended to lam_g and lam_x
    with the dual bounds; and, because the step is tau x the smaller of alpha and alpha_dual where one of them limits it, the difference of two
    steps that are each within the bound of the reference's alpha and alpha_dual, times max|d|.  dict(w, lam_g, lam_x, step, ref)"""
    p, w, lam_g, lam_x, obs = base
    a = (cfg, p, w, lam_g, lam_x, obs)
    ref = DR.stage_duals(*a, dp=dp, dobs=dobs)
    sw, sa = UR.spread(*a, dp=dp, dobs=dobs)
    bd = DR.bounds(DR.spread(*a, dp=dp, dobs=dobs))
    lim = lambda x: 1.0 if x == 1.0 else tau * x
    step = min(lim(ref["alpha"]), lim(ref["alpha_dual"]))
    dstep = 0.0 if step == 1.0 else 2.0 * tau * max((100.0 * sa + 1e-12) * ref["alpha"], bd["a"] * ref["alpha_dual"])      # two results, one bound each
    return dict(w=((100.0 * sw + 1e-12) * step + dstep) * np.abs(ref["dw"]).max(), lam_g=(bd["g"] * step + dstep) * np.abs(ref["dlam_g"]).max(),
                lam_x=(bd["x"] * step + dstep) * np.abs(ref["dlam_x"]).max(), step=dstep, ref=ref, ref_step=step)


def test_correct_scenarios_with_duals_is_correct_with_duals_per_scenario():
    import nmpc_amd
    cfg, P, W0, obs, x0c, obc = _scenario_setup()
    B, D = x0c.shape[:2]
    s = _product_solver(cfg, B)
    ctl = nmpc_amd.AdvancedStepController(s)
    pre = ctl.prepare(P, W0, obstacles=obs)
    plain = ctl.correct_scenarios(x0c, obstacles=obc)
    multi = ctl.correct_scenarios(x0c, obstacles=obc, update_duals=True)
    unc = ctl.last["uncorrected"]
    assert set(plain) == {"w", "u0", "step", "alpha", "info", "corrected"} and set(multi) == set(plain) | {"lam_g", "lam_x", "alpha_dual"}
    assert np.array_equal(_bits(_np(plain["alpha"])), _bits(_np(multi["alpha"])))
    w, lam_g, lam_x = (_np(pre[k]) for k in ("x", "lam_g", "lam_x"))
    assert multi["lam_g"].shape == (B, D, cfg.n_g) and multi["lam_x"].shape == (B, D, cfg.n_var) and multi["alpha_dual"].shape == (B, D)
    ok = _np(multi["corrected"])
    limited = 0
    for d in range(D):
        one = ctl.correct(x0c[:, d], obstacles=obc[:, d], update_duals=True)
        assert ctl.last["uncorrected"] == unc
        assert np.array_equal(_np(one["corrected"]), ok) and np.array_equal(_np(one["info"]), _np(multi["info"]))
        for b in range(B):
            got = {k: _np(multi[k])[b, d] for k in ("w", "lam_g", "lam_x")}
            if not ok[b]:
                for k, base in (("w", w), ("lam_g", lam_g), ("lam_x", lam_x)):
                    assert np.array_equal(_bits(got[k]), _bits(base[b])) and np.array_equal(_bits(_np(one[k])[b]), _bits(base[b])), (b, d, k)
                continue
            dp = np.concatenate([x0c[b, d] - P[b, : cfg.nx], np.zeros(cfg.nx)])
            tol = _scenario_tolerances(cfg, ctl.tau, (P[b], w[b], lam_g[b], lam_x[b], obs[b]), dp, obc[b, d] - obs[b])
            sm, so = float(_np(multi["step"])[b, d]), float(_np(one["step"])[b])
            al, ad = float(_np(multi["alpha"])[b, d]), float(_np(multi["alpha_dual"])[b, d])
            lim = lambda x: 1.0 if x == 1.0 else ctl.tau * x
            assert sm == min(lim(al), lim(ad)) and abs(sm - so) <= tol["step"], (b, d, sm, so, tol["step"])
            limited += sm < 1.0
            for k in ("w", "lam_g", "lam_x"):
                err = np.abs(got[k] - _np(one[k])[b]).max()
                print("instance %d scenario %d: |%s_multi - %s_correct| %.2e, tolerance %.2e, step %.6f / %.6f" % (b, d, k, k, err, tol[k], sm, so))
                assert err <= tol[k], (b, d, k, err, tol[k])
    assert ok.any() and limited > 0, "no scenario met a step limit: the tau * limit branch was not run"


def test_commit_scenario_then_correct_is_correct_with_commit_then_correct():
    import nmpc_amd
    cfg, P, W0, obs, x0c, obc = _scenario_setup()
    B, D = x0c.shape[:2]
    s = _product_solver(cfg, B)
    rng = np.random.default_rng(31)
    x1 = P[:, : cfg.nx] + 1e-3 * rng.standard_normal((B, cfg.nx))
    ob1 = obs + 1e-3 * rng.standard_normal(obs.shape)
    a, b_ = nmpc_amd.AdvancedStepController(s), nmpc_amd.AdvancedStepController(s)
    pre = a.prepare(P, W0, obstacles=obs)
    b_.prepare(P, W0, obstacles=obs)
    w, lam_g, lam_x = (_np(pre[k]) for k in ("x", "lam_g", "lam_x"))
    with pytest.raises(RuntimeError):
        a.commit_scenario(0)
    a.correct_scenarios(x0c, obstacles=obc)
    with pytest.raises(RuntimeError):
        a.commit_scenario(0)      # the scenarios carry no multipliers
    for d in (0, 2):      # a full step and a limited one
        a.prepare(P, W0, obstacles=obs); b_.prepare(P, W0, obstacles=obs)
        sc = a.correct_scenarios(x0c, obstacles=obc, update_duals=True)
        a.commit_scenario(d)
        one = b_.correct(x0c[:, d], obstacles=obc[:, d], commit=True)
        ok = _np(sc["corrected"])
        assert np.array_equal(ok, _np(one["corrected"])) and ok.any()
        ya = a.correct(x1, obstacles=ob1, update_duals=True)
        yb = b_.correct(x1, obstacles=ob1, update_duals=True)
        for b in range(B):
            pa, pb = ({k: _np(v)[b] for k, v in c._plan.items() if v is not None} for c in (a, b_))
            if not ok[b]:
                for k in ("p", "w", "lam_g", "lam_x", "obstacles"):
                    assert np.array_equal(_bits(pa[k]), _bits(pb[k])), (d, b, k)
                continue
            dp = np.concatenate([x0c[b, d] - P[b, : cfg.nx], np.zeros(cfg.nx)])
            dob = obc[b, d] - obs[b]
            t1 = _scenario_tolerances(cfg, a.tau, (P[b], w[b], lam_g[b], lam_x[b], obs[b]), dp, dob)
            # the base: scenario d's corrected point, and the parameters moved by the same step
            t1["p"] = t1["step"] * np.abs(dp).max(); t1["obstacles"] = t1["step"] * np.abs(dob).max()
            for k in ("p", "obstacles", "w", "lam_g", "lam_x"):
                err = np.abs(pa[k] - pb[k]).max()
                print("scenario %d instance %d: base %s differs by %.2e, tolerance %.2e" % (d, b, k, err, t1[k]))
                assert err <= t1[k], (d, b, k, err, t1[k])
            # the next correction from the two bases: the same tolerance at the committed point, on top of what the bases differ by
            dp2 = np.concatenate([x1[b] - pb["p"][: cfg.nx], np.zeros(cfg.nx)])
            t2 = _scenario_tolerances(cfg, a.tau, (pb["p"], pb["w"], pb["lam_g"], pb["lam_x"], pb["obstacles"]), dp2, ob1[b] - pb["obstacles"])
            for k in ("w", "lam_g", "lam_x"):
                err = np.abs(_np(ya[k])[b] - _np(yb[k])[b]).max()
                print("scenario %d instance %d: after the next correct() %s differs by %.2e, tolerance %.2e + %.2e" % (d, b, k, err, t1[k], t2[k]))
                assert err <= t1[k] + t2[k], (d, b, k, err, t1[k], t2[k])
        assert np.array_equal(_np(ya["corrected"]), _np(yb["corrected"]))


def test_correct_scenarios_with_duals_leaves_an_unconverged_plan_as_it_is():
    import nmpc_amd
    cfg = _six_with_a_field()
    B, D = 2, 3
    P, W0 = Hh.batch(cfg, B, 23)
    obs = np.tile(np.asarray(cfg.obstacles, float)[None], (B, 1, 1))
    ctl = nmpc_amd.AdvancedStepController(_product_solver(cfg, B, max_iter=1))
    pre = ctl.prepare(P, W0, obstacles=obs)
    out = ctl.correct_scenarios(P[:, None, : cfg.nx] + 1e-3 * np.ones((B, D, cfg.nx)), obstacles=np.tile(obs[:, None], (1, D, 1, 1)), update_duals=True)
    assert (_np(pre["status"]) != 0).all() and not _np(out["corrected"]).any() and ctl.last["uncorrected"] == B
    for d in range(D):
        for k, base in (("w", "x"), ("lam_g", "lam_g"), ("lam_x", "lam_x")):
            assert np.array_equal(_bits(_np(out[k])[:, d]), _bits(_np(pre[base]))), (d, k)
    ctl.commit_scenario(1)
    for k, base in (("w", "x"), ("lam_g", "lam_g"), ("lam_x", "lam_x")):
        assert np.array_equal(_bits(_np(ctl._plan[k])), _bits(_np(pre[base]))), k
