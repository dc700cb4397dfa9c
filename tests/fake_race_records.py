"""tests/fake_records.FakeRecords with the `race` surface of records.DeviceRecords, served by the model (tests/race_model.py) on the
records of the last replay: numpy out, no GPU, no library."""
import numpy as np

from tests import race_model as M
from tests.fake_records import FakeRecords


class RaceRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(RaceRecords, self).__init__(size, max_games, max_entries)

    def race(self, index, rules=1, max_libs=4, max_region=8, max_nodes=1024, max_pairs=64):
        self.calls.append(("race", len(index)))
        NW = (self.S * self.S + 31) // 32
        m = M.race(self.S, self.last["records"], index, rules=rules, max_libs=max_libs, max_region=max_region, max_nodes=max_nodes,
                   max_pairs=max_pairs)
        rows, regions = np.zeros((len(index), max_pairs, 16), np.int32), np.zeros((len(index), max_pairs, NW), np.uint32)
        for i, (r, g) in enumerate(zip(m["rows"], m["regions"])):
            rows[i, :len(r)], regions[i, :len(g)] = r, g
        return m["n_pairs"], rows, regions
