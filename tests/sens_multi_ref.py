"""The direction sets and the stacked reference of nmpc_sens_update_batch_multi (csrc/nmpc_sens_multi.hip).

No new mathematics: direction d of the call is nmpc_sens_update_batch on (dp, dobs, rhs)_d, so the reference is tests/sens_update_ref.stage_update
per direction, stacked, with that direction's spread.  Per point of tests/sens_points.SENS_TABLE there are NDIRS = 6 distinct directions:
direction 0 is the point's own (pt.dp, row_dobs, row_rhs) of the single-direction test, directions 1 .. 5 are seeded with the same generators
(0.02 * _weights for dp and dobs, _weights for rhs).  A (row, point, direction) whose seed gives a direction that does not hold the input
conditions of tests/test_sens_multi_host.py is given another seed in RESEED; none is left out.

  directions(r, n)     [(dp, dobs, rhs)] * NDIRS at point n of the row r
  reference(r, n)      [dict(dw, alpha, info, sw, sa)] * NDIRS, computed once per process
  bound(ref)           (100 sw + 1e-12, 100 sa + 1e-12): the project's bound, relative to max|dw| and to alpha
  slots(D, seed)       which of the NDIRS directions stands in each of D slots: round-robin under a seeded permutation
"""
import functools

import numpy as np

from tests import sens_points as SP
from tests import sens_update_ref as UR

NDIRS = 6
RESEED = {}      # (row index, point, direction) -> attempt number, where attempt 0 does not hold the input conditions


def _direction(r, n, d):
    if d == 0:
        pt = SP.points(r)[n]
        return pt.dp, UR.row_dobs(r, n), UR.row_rhs(r, n)
    cfg = r.cfg
    i = SP.SENS_TABLE.index(r)
    rng = np.random.default_rng([7000 * r.seed + n, d, RESEED.get((i, n, d), 0)])
    dp = 0.02 * UR._weights(rng, 2 * cfg.nx)
    dobs = None
    if r.kind in ("static", "moving"):
        dobs = 0.02 * UR._weights(rng, (cfg.K, 3) if r.kind == "static" else (cfg.N, cfg.K, 3))
    return dp, dobs, UR._weights(rng, cfg.n_var)


def directions(r, n):
    return [_direction(r, n, d) for d in range(NDIRS)]


@functools.lru_cache(maxsize=None)
def _reference(i, n):
    r = SP.SENS_TABLE[i]
    pt = SP.points(r)[n]
    out = []
    for dp, dobs, rhs in directions(r, n):
        a = (r.cfg, pt.p, pt.w, pt.lam_g, pt.lam_x, pt.obs)
        ref = UR.stage_update(*a, dp=dp, dobs=dobs, rhs=rhs)
        ref["sw"], ref["sa"] = UR.spread(*a, dp=dp, dobs=dobs, rhs=rhs)
        out.append(ref)
    return tuple(out)


def reference(r, n):
    """the stacked reference of the point's directions; callers do not change it"""
    return list(_reference(SP.SENS_TABLE.index(r), n))


def bound(ref):
    return 100.0 * ref["sw"] + 1e-12, 100.0 * ref["sa"] + 1e-12


def slots(D, seed):
    """direction index of each of D slots: the NDIRS directions round-robin, in a seeded order"""
    perm = np.random.default_rng(seed).permutation(NDIRS)
    return [int(perm[s % NDIRS]) for s in range(D)]


def stack(r, n, slot_dirs):
    """(dp [D, n_p], dobs [D, ...] or None, rhs [D, n_var]) of the slots"""
    ds = directions(r, n)
    dp = np.stack([ds[d][0] for d in slot_dirs])
    dobs = None if ds[0][1] is None else np.stack([ds[d][1] for d in slot_dirs])
    return dp, dobs, np.stack([ds[d][2] for d in slot_dirs])


def d_values(c):
    """the D of the parity calls for a kernel that carries c directions per pass: the group edges, one beyond two groups, and the largest"""
    return sorted({D for D in (1, 2, c - 1, c, c + 1, min(2 * c + 1, 64), 64) if 1 <= D <= 64})
