"""CPU: the power of the playout-tree-search case set.  Every fault switch of tests/uct_model.py changes the expected outputs of the
runs of tests/uct_cases.py at every board size, so a kernel with that slip cannot pass tests/test_gpu_uct.py; and the runs are what
they claim to be."""
import numpy as np
import pytest

from tests import uct_cases as UC
from tests import uct_model as UM

POWER_SIZES = UM.SIZES
# runs tried in this order until one notices the switch; the cheap ones first
ORDER = ("short", "kos", "pool", "nil", "best", "komi", "games")
KEYS = ("visits", "wins2", "rave", "own", "sums", "info", "trace")


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize("S", POWER_SIZES)
def test_every_fault_switch_is_noticed(S):
    missed = []
    for fault in UM.FAULTS:
        if not any(_differs(UC.run_model(S, name), UC.run_model(S, name, fault)) for name in ORDER):
            missed.append(fault)
    assert not missed, (S, missed)


@pytest.mark.parametrize("S", POWER_SIZES)
def test_the_runs_are_what_they_claim(S):
    N = S * S
    kos = UC.run_model(S, "kos")
    depth = (kos["trace"][0] >> 9) & 127
    assert depth.tolist() == [min(s + 1, UM.MAX_DEPTH) for s in range(70)]           # depth 64 is reached and held
    assert kos["info"][0].tolist()[:3] == [UM.MAX_DEPTH, UM.MAX_DEPTH, 0] and (kos["trace"][0] >> 18).all()
    a0 = kos["trace"][0] & 511
    assert (a0 == (3 if S == 5 else 4) * S + 2).all()                                # black's one candidate
    for seed in (1, 2):                                              # a simulation there does not depend on its draws
        again = UM.search(S, UC.case_records(S)[1], **dict(UC.runs(S)["kos"], seed=seed, sims=8))
        assert np.array_equal(again["trace"][0], kos["trace"][0][:8])
    pool = UC.run_model(S, "pool")
    assert (pool["info"][:, 0] == 3 * 2).all() and (pool["info"][:, 2] == 2).all()   # both trees of a row full and refused
    short = UC.run_model(S, "short")
    assert short["sums"][:, 2].sum() > 0                             # draws occur under komi2 = 0
    assert ((short["trace"] >> 16) & 3 == 1).any()
    assert (short["info"][:, 1] == 2).any()                          # a game ends inside the tree: D == max_plies
    names = UC.case_records(S)[0]
    none = names.index("none")
    assert short["visits"][none, N] == 16 and short["info"][none, 3] == N             # nobody has a candidate: the pass
    komi = UC.run_model(S, "komi")
    assert UC.runs(S)["komi"]["komi2"] % 2 == 1 and not ((komi["trace"] >> 16) & 3 == 1).any()
    best = UC.run_model(S, "best")
    assert any(UM.best_of(v, w, "best_by_wins") != b for v, w, b in zip(best["visits"], best["wins2"], best["info"][:, 3]))
    games = UC.run_model(S, "games")
    assert games["info"][:, 1].max() >= 2 and (games["sums"][:, 7] == 48).all()
