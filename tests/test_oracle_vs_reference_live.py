"""Differential test beyond the main rules goldens: random playouts of the Python reference under NEW seeds (seed offsets
101 / 202 / 303, recorded by tests/golden/gen_golden.py --only seeded_rules as tests/golden/rules_S<S>_seed<seed>.npz) are
replayed through the oracle.  The fixtures are stored, so the test needs nothing outside the repository."""
import pytest

from tests.helpers import load
from tests.test_oracle_golden import _replay


@pytest.mark.parametrize("S,seed", [(5, 101), (9, 202), (13, 303)])
def test_fresh_reference_playouts(S, seed):
    z = load("rules_S%d_seed%d.npz" % (S, seed))
    assert int(z["n_games"]) >= 2
    for gi in range(int(z["n_games"])):
        _replay(z, gi, S)
