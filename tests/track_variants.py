"""The table of every tracking instantiation of the column kernel, nmpc::track_col_kernel<M, THB, DL, TPB>, and for each the recipe that makes
nmpc_solve_batch_ref launch it.

A row is the tuple of nmpc_debug_track_variant_of_config(): (3, m, thb, flags, threads) with flags = the DL template argument of the mangled
name | 8.  The tracking kernel is instantiated with the per-instance obstacle field only (DL | 4), in every shape and data layout the field
instantiations of solve_col_kernel have (tests/kernel_variants.py, the rows with flag 4): the rows here are those rows with 8 added.
tests/test_track_solve_host.py holds the table against the symbols of the built code object and every recipe against the descriptor;
tests/test_gpu_track_solve.py solves every recipe.

The horizon of a recipe is a rule, not a literal: "short" (duals, and for two robots factors, in LDS), "factors_out" / "duals_out" (the
shortest horizon at which the descriptor reports the stage factors / the duals out of LDS), 20 (the latency shapes and the larger teams),
"waves4" (the shortest horizon at which five / six robots among eight obstacles get four wavefronts).  recipe_cfg() resolves the rule by
asking the descriptor on the 256 compute units of an MI355X; it makes no launch and needs no device.

Inputs: four instances per recipe, built like tests/tracking_ref.family_inputs — starts as helpers.instance, a constant-velocity line path per
robot that starts up to 0.15 from it, the xs half of p NaN.  Rows with the heading bound pass the config's obstacles as an explicit static
per-instance field (S = 1); rows without it pass no field (the handle's own); the checker (tests/tracking_ipm.py) reads the config's.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import nlp_ref as R
from tests import kernel_variants as KV
from tests import tracking_ipm as TI
from tests import tracking_ref as TR

CUS = 256      # compute units of an MI355X
TRACK = 8      # bit of the descriptor's flags: the launch is track_col_kernel
NB = 4         # distinct instances per recipe; a larger batch repeats them in order

# row: (3, m, thb, flags | 8, threads); horizon: the rule above; K: obstacles of the config; pad: pad_rows; B: batch; pin: nmpc_options_t.kernel;
# ordered: solve with a dispatch-order hint; field: the call passes the config's obstacles as its own static field; max_iter
TrackRecipe = namedtuple("TrackRecipe", "row horizon K pad B pin ordered field max_iter")


def _rows():
    out = []
    for thb in (0, 1):
        K, pad, field = 2, thb == 1, thb == 1
        for m in range(1, 11):
            tpB = NB if m <= 3 else KV.TP_BATCH[m]      # from four robots on the throughput shape is the library's choice beyond twice the latency slots
            if m <= 4:
                out.append(TrackRecipe((3, m, thb, (2 if m == 2 else 1) | 4 | TRACK, 64), "short", K, pad, tpB, 0, 0, field, 400))
                if m == 2:
                    out.append(TrackRecipe((3, m, thb, 1 | 4 | TRACK, 64), "factors_out", K, pad, tpB, 0, 0, field, 400))
                out.append(TrackRecipe((3, m, thb, 0 | 4 | TRACK, 64), "duals_out", K, pad, tpB, 0, 0, field, 400))
            else:
                out.append(TrackRecipe((3, m, thb, 0 | 4 | TRACK, 64), 20, K, pad, tpB, 0, 0, field, 400))
            lat = 1 if m <= 6 else 0
            out.append(TrackRecipe((3, m, thb, lat | 4 | TRACK, 128), 20, K, pad, NB, 4 if m <= 3 else 0, int(m >= 4 and thb == 1), field, 400))
            if m in (5, 6):
                out.append(TrackRecipe((3, m, thb, lat | 4 | TRACK, 256), "waves4", 8, pad, NB, 0, 0, field, 600))
    return out


TRACK_TABLE = _rows()
SHORT = {1: 20, 2: 16, 3: 16, 4: 12}


def row_id(r):
    return "m%d-thb%d-dl%d-t%d" % r.row[1:]


def track_variant_of_config(cc, pin, cus, B, ordered, field):
    """nmpc_debug_track_variant_of_config on an nmpc_config_t: (return code, row, LDS bytes, kernel code)"""
    import ctypes as C
    import nmpc_amd
    lib = nmpc_amd._lib
    v, k = lib.CDebugVariant(), C.c_int32(0)
    rc = lib.load().nmpc_debug_track_variant_of_config(C.byref(cc), C.byref(lib.COptions(kernel=pin, trace_instance=-1)), cus, B, int(ordered), int(bool(field)),
                                                      C.byref(v), C.byref(k))
    return rc, (v.kernel, v.m, v.thb, v.flags, v.threads), int(v.lds_bytes), k.value


def _cfg_dict(r, N):
    return KV._cfg(r.row[1], N, r.row[2], r.K, r.pad)


@functools.lru_cache(maxsize=None)
def horizon(r):
    """the horizon of a recipe, by its rule, from the descriptor (no literal: where a layout flag flips is the library's to say)"""
    if isinstance(r.horizon, int):
        return r.horizon
    m = r.row[1]
    if r.horizon == "short":
        return SHORT[m]

    def flags_at(N):
        rc, got, _, _ = track_variant_of_config(KV.c_config(R.NLPConfig(**_cfg_dict(r, N)), 10), r.pin, CUS, r.B, r.ordered, r.field)
        assert rc == 0, (r.row, N, rc)
        return got
    for N in range(2, 400):
        got = flags_at(N)
        if r.horizon == "factors_out" and (got[3] & 3) < 2:
            return N
        if r.horizon == "duals_out" and (got[3] & 3) == 0:
            return N
        if r.horizon == "waves4" and got[4] == 256:
            return N
    raise AssertionError("no horizon up to 400 gives %s its rule %s" % (r.row, r.horizon))


def recipe_cfg(r):
    """the oracle config of a recipe"""
    return R.NLPConfig(**_cfg_dict(r, horizon(r)))


@functools.lru_cache(maxsize=None)
def inputs(r):
    """(cfg, P [NB, 2 n_x] with the xs half NaN, REF [NB, N, n_x], W0 [NB, n_var]) of a recipe's distinct instances"""
    cfg = recipe_cfg(r)
    P, REF, W0 = TR.family_inputs("track-" + row_id(r), cfg, count=NB)
    return cfg, P, REF, W0


def tiled(r, *arrays):
    """the recipe's batch: its NB distinct instances repeated in order"""
    idx = np.arange(r.B) % NB
    return [np.ascontiguousarray(a[idx]) for a in arrays]


def field_of(r, cfg, B):
    """the per-instance obstacle field a recipe passes: the config's obstacles, static (S = 1), or None"""
    if not r.field:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(cfg.obstacles, float).reshape(1, 1, -1, 3), (B, 1, len(cfg.obstacles), 3)))


@functools.lru_cache(maxsize=None)
def checker(r):
    """tests/tracking_ipm.py on the recipe's distinct instances, computed once per process: list of its result dicts"""
    cfg, P, REF, W0 = inputs(r)
    o = TI.Opts()
    o.max_iter = r.max_iter
    return [TI.solve(cfg, P[b], REF[b], W0[b], o) for b in range(NB)]


# ---- the multipliers of a tracking solve held to account in numpy (tests/duals_ref.residuals with the tracking gradient) ---------------------
def residuals(cfg, w, p, ref, lam_g, lam_x, obs=None):
    """(res [6] = (stat, eq, ineq, bnd, compl, sign), grad_lag) as tests/duals_ref.residuals defines them, with grad f of the tracking cost"""
    from tests import duals_ref as D
    w = np.asarray(w, float).reshape(-1)
    lbx, ubx, lbg, ubg = R.bounds(cfg)
    g, J = D.functions(cfg, w, p, obs)
    grad = TR.grad_objective(cfg, w, ref) + J.T @ lam_g + lam_x
    eq = lbg == ubg
    ineq = ~eq
    c = float(np.max(np.abs(lam_g[ineq]) * (g[ineq] - lbg[ineq]))) if ineq.any() else 0.0
    fl, fu = np.isfinite(lbx), np.isfinite(ubx)
    c = max(0.0, c, float(np.max(np.maximum(-lam_x[fl], 0.0) * (w[fl] - lbx[fl]))), float(np.max(np.maximum(lam_x[fu], 0.0) * (ubx[fu] - w[fu]))))
    res = np.array([np.max(np.abs(grad)), np.max(np.abs(g[eq] - lbg[eq])),
                    max(0.0, float(np.max(lbg[ineq] - g[ineq]))) if ineq.any() else 0.0,
                    max(0.0, float(np.max(lbx - w)), float(np.max(w - ubx))), c,
                    max(0.0, float(np.max(lam_g[ineq]))) if ineq.any() else 0.0])
    return res, grad
