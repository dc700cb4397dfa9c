"""tests/fake_records.FakeRecords with the `life` / `stones` surface of records.DeviceRecords, served by the model
(tests/life_model.py) on the records of the last replay: numpy out, no GPU, no library."""
import numpy as np

from tests import life_model as M
from tests.fake_records import FakeRecords


class LifeRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(LifeRecords, self).__init__(size, max_games, max_entries)

    def life(self, index):
        self.calls.append(("life", len(index)))
        m = M.life(self.S, self.last["records"], index)
        return m["sets"], m["counts"]

    def stones(self, index):
        self.calls.append(("stones", len(index)))
        recs, N = self.last["records"], self.S * self.S
        out = np.zeros((len(index), N), np.int8)
        for i, r in enumerate(index):
            if 0 <= r < len(recs):
                black, white, _ = M.record_stones(self.S, recs[r])
                out[i, black], out[i, white] = 1, -1
        return out
