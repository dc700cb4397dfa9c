"""A sanity test of play for the playout tree search (include/sgo.h "playout tree search"): three constructed positions in which one
move decides a capturing race of large chains -- the side to move takes a chain that is in atari, or loses its own chain, which is in
atari too -- so that a search worth its name must find it.  The positions, komi, seeds and counts were chosen so that the MODEL's best
(tests/uct_model.py) is that move with a wide margin of visits; the CPU test says so, and the GPU test asserts the same of the device.
  cap5     5x5, black to move: white's three stones in the corner have the one liberty (0,0); black's walls around them are short
           of liberties themselves
  race7    7x7, black to move: white's three stones on the top edge and black's four stones under them share the one liberty (0,0)
  race7_w  the same with the colours exchanged and white to move; komi the other way"""
import functools

import numpy as np
import pytest

from tests import playout_model as PM
from tests import uct_model as UM
from tests.tactics_cases import diagram

RACE7 = [".OOOX..", "XXXXOO.", "OOOOX..", "....X..", "XXXX...", ".......", "......."]
SWAP = {"X": "O", "O": "X", ".": "."}
CASES = {                                                            # name: (S, rows, white to play, komi2, the move)
    "cap5": (5, [".OX..", "OOX..", "XXO..", "..O..", "....."], False, 1, 0),
    "race7": (7, RACE7, False, 25, 0),
    "race7_w": (7, ["".join(SWAP[c] for c in row) for row in RACE7], True, -25, 0),
}
ARGS = dict(trees=4, sims=48, seed=1, rules=1, expand_at=2, rave_equiv=64, prior=4)


def _record(name):
    S, rows, wtp, komi2, move = CASES[name]
    b, w = diagram(S, rows)
    return PM.build_record(S, b, w, wtp, None, None, np.random.RandomState(5))


@functools.lru_cache(maxsize=None)
def _model(name):
    S, rows, wtp, komi2, move = CASES[name]
    return UM.search(S, _record(name)[None], None, komi2=komi2, **ARGS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_finds_the_move(name):
    S, rows, wtp, komi2, move = CASES[name]
    m = _model(name)
    v = m["visits"][0]
    assert int(m["info"][0, 3]) == move and v[move] >= 2 * np.delete(v, move).max(), (name, v.tolist())
    assert m["wins2"][0, move] > v[move]                              # and the mover wins more often than not after it


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_device_finds_the_move(name):
    from sejonggo_amd import uct
    S, rows, wtp, komi2, move = CASES[name]
    m = _model(name)
    v = uct.search(S, _record(name)[None], None, komi=komi2 / 2.0, **ARGS)
    assert v.best(0) == move and v.winrate(0) > 0.5
    assert np.array_equal(v.visits, m["visits"]) and np.array_equal(v.wins2, m["wins2"])
    assert bool(v.white_to_play[0]) == wtp
