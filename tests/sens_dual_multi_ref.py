"""The stacked reference of nmpc_sens_update_batch_multi_duals (csrc/nmpc_sens_dual_multi.hip).

No new mathematics: direction d of the call is nmpc_sens_update_batch_duals on (dp, dobs, rhs)_d, so the reference is
tests/sens_dual_ref.stage_duals per direction of tests/sens_multi_ref.directions, with that direction's spread and bounds; dlam_p is
include/nmpc.h's formula in numpy.  A (row, point, direction) that does not hold the input conditions of tests/test_sens_dual_multi_host.py
would be replaced by a seeded one in RESEED and listed there; none is.

  reference(r, n)      [dict(dw, alpha, info, dlam_g, dlam_x, alpha_dual, dlam_p, sp, bd)] * NDIRS, computed once per process
  dlam_p(cfg, dw, dlam_g, dp)      [x0 part: dlam_g[:n_x]; xs part: 2 Q (sum_{k<N} dX_k - N dxs)]
  dlam_p_tol(cfg, dw, dp)          the summation bound of the xs part, 4 (N + 2) 2^-53 2 q (sum_k |dX_k| + N |dxs|) per entry
"""
import functools

import numpy as np

from tests import sens_dual_ref as DR
from tests import sens_multi_ref as MR
from tests import sens_points as SP

NDIRS = MR.NDIRS
RESEED = {}      # (row index, point, direction) -> seed of the direction that replaces it; empty: all 600 hold the input conditions


def _q(cfg):
    return np.tile(np.asarray(cfg.q, float), cfg.m)


def dlam_p(cfg, dw, dlam_g, dp):
    nx, N = cfg.nx, cfg.N
    dX = np.asarray(dw, float)[: (N + 1) * nx].reshape(N + 1, nx)
    dxs = np.zeros(nx) if dp is None else np.asarray(dp, float)[nx:]
    return np.concatenate([np.asarray(dlam_g, float)[:nx], 2.0 * _q(cfg) * (dX[:N].sum(axis=0) - N * dxs)])


def dlam_p_tol(cfg, dw, dp):
    nx, N = cfg.nx, cfg.N
    dX = np.asarray(dw, float)[: (N + 1) * nx].reshape(N + 1, nx)
    dxs = np.zeros(nx) if dp is None else np.asarray(dp, float)[nx:]
    return 4.0 * (N + 2) * 2.0 ** -53 * 2.0 * _q(cfg) * (np.abs(dX[:N]).sum(axis=0) + N * np.abs(dxs))


@functools.lru_cache(maxsize=None)
def _reference(i, n):
    r = SP.SENS_TABLE[i]
    pt = SP.points(r)[n]
    out = []
    for dp, dobs, rhs in MR.directions(r, n):
        a = (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        ref = DR.stage_duals(*a, dp=dp, dobs=dobs, rhs=rhs)
        ref["sp"] = DR.spread(*a, dp=dp, dobs=dobs, rhs=rhs)
        ref["bd"] = DR.bounds(ref["sp"])
        ref["dlam_p"] = dlam_p(r.cfg, ref["dw"], ref["dlam_g"], dp)
        out.append(ref)
    return tuple(out)


def reference(r, n):
    """the stacked reference of the point's directions; callers do not change it"""
    return list(_reference(SP.SENS_TABLE.index(r), n))
