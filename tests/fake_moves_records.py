"""tests/fake_records.FakeRecords with the `moves` surface of records.DeviceRecords, served by the model (tests/moves_model.py) on
the records of the last replay: numpy out, no GPU, no library."""
import numpy as np

from tests import moves_model as M
from tests.fake_records import FakeRecords


class MovesRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(MovesRecords, self).__init__(size, max_games, max_entries)

    def moves(self, index, side=0, action=None, colour=None):
        self.calls.append(("moves", len(index)))
        recs, N = self.last["records"], self.S * self.S
        m = M.moves(self.S, recs, index, side)
        if action is None:
            return m["rows"], m["counts"]
        played = np.zeros((len(index), 8), np.int16)
        in_turn = np.ones(len(index), bool)
        for i, (r, a) in enumerate(zip(index, action)):
            if 0 <= a < N:
                played[i] = m["rows"][i, int(a)]
            if colour is not None:
                ok = 0 <= r < len(recs)
                white_to_play = ok and bool(int(recs[int(r)][(N + 31) // 32 - 1]) >> 31)
                in_turn[i] = ok and (-1 if white_to_play else 1) == int(colour[i])
        return played, m["counts"], in_turn
