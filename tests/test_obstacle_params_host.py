"""CPU: the per-instance obstacle field (nmpc_*_batch_obs) is declared, exported and bound; the library's fatbin holds its column-kernel and
eval-kernel instantiations (so the register and scratch checks of tests/test_abi_host.py see them); the moving-obstacle restatement of the
NLP (tests/moving_obstacles_ref.py) is the oracle's NLP for a time-invariant field and its Jacobian is the derivative of its rows."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import nlp_ref as R
from tests import helpers as Hh
from tests import moving_obstacles_ref as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nmpc_solve_batch_obs", "nmpc_step_batch_obs", "nmpc_eval_batch_obs")


def test_obstacle_entry_points_declared_and_exported(built):
    import nmpc_amd
    hdr = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in nmpc_amd._lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", nmpc_amd._lib.SO_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) <= exported
    L = nmpc_amd._lib.load()
    for n in NEW:
        assert len(getattr(L, n).argtypes) == {"nmpc_eval_batch_obs": 9}.get(n, 13), n


def test_fatbin_holds_the_obstacle_field_instantiations(built, tmp_path):
    """The per-instance field instantiations of the column kernel (bit 2 of DL: DL = 4..7) exist for every team size in every shape the plain
    ones have, under the solve_col_kernel name the build checks select; up to six robots they stay within 256 VGPRs in the throughput shape and
    within the plain ones' scratch limit, the six-robot ones without scratch; the eval kernel has one per team size (team size + 16)."""
    notes = Hh.kernel_notes(tmp_path)
    col = {}
    for k, v in notes.items():
        m = re.search(r"solve_col_kernelILi(\d+)ELi(\d)ELi(\d)ELi(\d+)E", k)
        if m:
            col[tuple(int(g) for g in m.groups())] = v
    plain = {k for k in col if k[2] < 4}
    obs = {k for k in col if k[2] >= 4}
    want = {(m, t, dl | 4, tpb) for (m, t, dl, tpb) in plain}
    assert obs == want, obs ^ want
    for (m, t, dl, tpb), v in col.items():
        if dl >= 4 and m <= 6:
            if tpb == 64:
                assert v["vgpr_count"] <= 256, ((m, t, dl, tpb), v)
            assert v.get("private_segment_fixed_size", 0) <= 32, ((m, t, dl, tpb), v)
        if dl >= 4 and m == 6:
            assert v.get("private_segment_fixed_size", 0) == 0 and v["vgpr_count"] <= 256, ((m, t, dl, tpb), v)
    ev = {int(re.search(r"eval_kernelILi(\d+)E", k).group(1)) for k in notes if "eval_kernelILi" in k}
    assert ev == set(range(1, 11)) | set(range(17, 27)), ev


def test_moving_obstacle_restatement():
    """Time-invariant field: g and J equal nlp_ref.constraints / jacobian exactly.  Moving field: J equals central finite differences of g
    to 1e-7."""
    rng = np.random.default_rng(1)
    for ocfg in (Hh.cfg_mix3(10), R.cfg_obs3(12)):
        P, W0 = Hh.batch(ocfg, 2, 6)
        for b in range(2):
            w = W0[b] + rng.normal(0.0, 0.2, W0[b].shape)
            static = np.array(ocfg.obstacles)
            assert np.array_equal(MO.constraints(ocfg, w, P[b], static), R.constraints(ocfg, w, P[b]))
            assert np.array_equal(MO.jacobian(ocfg, w, P[b], static), R.jacobian(ocfg, w, P[b]))
            assert np.array_equal(MO.constraints(ocfg, w, P[b], np.broadcast_to(static, (ocfg.N,) + static.shape)), R.constraints(ocfg, w, P[b]))
            moving = np.broadcast_to(static, (ocfg.N,) + static.shape).copy()
            moving[:, :, :2] += rng.normal(0.0, 0.3, (ocfg.N, ocfg.K, 2))
            moving[:, :, 2] *= 1.0 + np.linspace(0.0, 0.5, ocfg.N)[:, None]
            assert not np.array_equal(MO.constraints(ocfg, w, P[b], moving), R.constraints(ocfg, w, P[b]))
            J = MO.jacobian(ocfg, w, P[b], moving)
            h = 1e-6
            for j in range(w.size):
                e = np.zeros_like(w); e[j] = h
                fd = (MO.constraints(ocfg, w + e, P[b], moving) - MO.constraints(ocfg, w - e, P[b], moving)) / (2 * h)
                assert np.abs(fd - J[:, j]).max() <= 1e-7, (j, np.abs(fd - J[:, j]).max())
