"""tests/fake_records.FakeRecords with the `playouts` / `to_play` surface of records.DeviceRecords, served by the model
(tests/playout_model.py) on the records of the last replay: numpy out, no GPU, no library.  Every call's arguments are kept."""
import numpy as np

from tests import playout_model as PM
from tests.fake_records import FakeRecords


class PlayoutRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(PlayoutRecords, self).__init__(size, max_games, max_entries)
        self.asked = []

    def playouts(self, index, per_row=16, seed=0, rules=1, max_plies=0, amaf=True):
        index = [int(r) for r in index]
        self.calls.append(("playouts", len(index)))
        self.asked.append((index, int(per_row), int(seed), int(rules), int(max_plies)))
        m = PM.playouts(self.S, self.last["records"], index, int(per_row), int(seed), int(rules), int(max_plies))
        return m["own"], (m["amaf"] if amaf else None), m["sums"]

    def to_play(self, index):
        recs = self.last["records"]
        NW = recs.shape[1] // 16
        return np.array([0 if not 0 <= int(r) < len(recs) else (-1 if recs[int(r), NW - 1] >> 31 else 1) for r in index], np.int8)
