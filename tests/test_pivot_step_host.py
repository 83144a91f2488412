"""No GPU: the cases of tests/test_gpu_pivot_step.py do what that file says of them — on the oracle, every case rejects pivots during its
solves, at N = 6 at least half of the instances reject in their first sweep and at least one of them at stage 0 only, and no sweep rejects
at stage N - 1 (tests/pivot_step_cases.py: how the oracle's counters show it)."""
import pytest

from tests import pivot_step_cases as PC

TEAMS = (2, 3, 5, 6)
HORIZONS = (3, 6)


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("m", TEAMS)
def test_the_oracle_rejects_where_the_cases_say(m, N):
    cfg, P, W0, ref, fs, whole = PC.select(m, N)
    assert (ref["status"] == 0).all() and ref["iters"].max() < PC.ITER_LIMIT
    rej, excess = fs[:, 0], fs[:, 1]
    assert whole.sum() > 0, "no sweep of the case rejects a pivot"
    assert (excess >= 2 * rej).all(), "a rejection at stage N - 1"      # a rejection there costs ONE stage more
    if N == 6:
        assert (rej > 0).sum() >= PC.B // 2, "first sweeps that reject"
        assert ((rej > 0) & (excess == N * rej)).any(), "a first sweep whose every rejection is at stage 0"
    print("\n  m %d N %d: first sweep rejects on %d instances (at stage 0 only on %d), %d rejections over the whole solves of %d instances"
          % (m, N, (rej > 0).sum(), ((rej > 0) & (excess == N * rej)).sum(), whole.sum(), (whole > 0).sum()), end="")
