"""Generates tests/golden/slsqp_track.npz: (p, ref, w0, w_pol, f_pol) of the NLP with a pose reference per stage, solved by an INDEPENDENT solver.

    python tests/golden/gen_tracking_cases.py

The recipe of gen_golden.py — scipy-SLSQP with ftol 1e-14 from the cold start, polished once from its own solution — on
tests/tracking_ref.py's restatement (the cost of stage k measures X_k against row k of `ref`).  Every stored case passes the restatement's
kkt_report at gen_golden.py's limits.  Families (tests/tracking_ref.families): one robot N = 8, two robots N = 8, three robots N = 6, one
robot among two obstacles N = 8, one robot with a finite heading bound; three instances each.  The reference of every robot starts at an
offset from the robot and moves at a constant velocity (tracking_ref.family_inputs).  Keys of the file: <family>_p, _ref, _w0, _w, _f,
_w_pol, _f_pol.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import tracking_ref as TR  # noqa: E402

LIMITS = dict(stat=1e-4, eq=1e-9, ineq=1e-9, bnd=1e-12)      # gen_golden.make


def passes(k):
    return all(k[n] < LIMITS[n] for n in LIMITS)


if __name__ == "__main__":
    out = {}
    for name, cfg in TR.families().items():
        P, REF, W0 = TR.family_inputs(name, cfg)
        rows = []
        for p, ref, w0 in zip(P, REF, W0):
            r = TR.slsqp(cfg, p, ref, w0)
            r2 = TR.slsqp(cfg, p, ref, r.x)
            # status 8 ("positive directional derivative") is SLSQP's way of saying it cannot improve below ftol = 1e-14
            assert r.status in (0, 8) and r2.status in (0, 8), (name, r.message, r2.message)
            k = TR.kkt_report(cfg, r2.x, p, ref)
            assert passes(k), (name, k)
            rows.append((r.x, r.fun, r2.x, r2.fun))
            print(name, "f* = %.9f  (polish moved w by %.1e)  %s" % (r2.fun, np.max(np.abs(r.x - r2.x)), k))
        out.update({name + "_p": P, name + "_ref": REF, name + "_w0": W0, name + "_w": np.stack([r[0] for r in rows]),
                    name + "_f": np.array([r[1] for r in rows]), name + "_w_pol": np.stack([r[2] for r in rows]),
                    name + "_f_pol": np.array([r[3] for r in rows])})
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "slsqp_track.npz"), **out)
