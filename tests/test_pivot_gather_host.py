"""No GPU: the row-paired pivot step replicates its pivot row by two lane gathers from the register that holds it, instead of lane swaps on
copies (docs/PIVOT_GATHER.md).  tools/rp_emu.py writes both forms out lane by lane.

(1) For every team size of the row-paired sweep (2 .. 6; 3 and 5 leave the last robot slot of the upper half empty) and every pivot j, the
    two address vectors (+ 128 bytes for a row of the upper half) give `own` and `ur` equal to the swap form's lane for lane, on a register
    of distinct lane tags — and on a register whose OTHER half is NaN: neither replica may read a lane of the other row.
(2) The swaps leave the other row of the register in both of its halves; the gathers leave the register as it is.  A whole emulated sweep in
    either form — pivot diagonal, right-hand side and reciprocal read where the kernel reads them — leaves the same pivot rows, right-hand
    sides and cost-to-go, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rp_emu as E      # noqa: E402

TEAMS = (2, 3, 4, 5, 6)


def test_the_address_vectors_are_the_documented_permutations():
    gown, gur = E.gather_addrs()
    lanes = np.arange(64)
    assert (gown == 4 * (lanes % 32)).all() and (gur == 4 * (16 * (lanes // 32) + lanes % 16)).all()
    assert gown.max() + 128 < 256 and gur.max() + 128 < 256      # with the offset of the upper half the address stays inside the 64 lanes


@pytest.mark.parametrize("m", TEAMS)
def test_gathered_replicas_equal_the_swapped_ones(m):
    NU = 2 * m
    for j in range(NU):
        hj, ij = E.rp_half(j), E.rp_slot(j)
        assert ij < 2 * ((m + 1) // 2)
        tags = 1000.0 * (ij + 1) + np.arange(64)               # distinct per lane (and per register)
        own_s, ur_s, left_s = E.replicate_swap(tags, hj)
        own_g, ur_g, left_g = E.replicate_gather(tags, hj)
        assert np.array_equal(own_s, own_g) and np.array_equal(ur_s, ur_g), (m, j)
        row = tags[32 * hj:32 * hj + 32]
        assert np.array_equal(own_g, np.concatenate([row, row])), (m, j)
        assert np.array_equal(ur_g, np.concatenate([row[:16], row[:16], row[16:], row[16:]])), (m, j)
        # the register afterwards: the swaps put the other row in both halves, the gathers leave it alone; the other row's own half agrees
        o = 1 - hj
        assert np.array_equal(left_g, tags) and np.array_equal(left_s[32 * o:32 * o + 32], tags[32 * o:32 * o + 32])
        poisoned = tags.copy(); poisoned[32 * o:32 * o + 32] = np.nan
        own_p, ur_p, _ = E.replicate_gather(poisoned, hj)
        assert np.array_equal(own_p, own_g) and np.array_equal(ur_p, ur_g), "a replica reads a lane of the other row"


@pytest.mark.parametrize("m", TEAMS)
def test_a_sweep_without_rearranging_the_register_equals_the_swap_form(m):
    rng = np.random.default_rng(40 + m)
    N = 3
    pk, off = E.random_packs(m, N, rng)
    rows_s, P_s, p_s = E.rp_sweep(pk, m, N, off, form="swap")
    rows_g, P_g, p_g = E.rp_sweep(pk, m, N, off, form="gather")
    for k in range(N):
        assert np.array_equal(rows_s[k], rows_g[k]), (m, k)
    assert np.array_equal(P_s, P_g) and np.array_equal(p_s, p_g)
    assert np.isfinite(P_g).all() and np.abs(P_g).max() > 0
