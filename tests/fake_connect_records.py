"""tests/fake_records.FakeRecords with the `connect` surface of records.DeviceRecords, served by the model (tests/connect_model.py) on
the records of the last replay: numpy out, no GPU, no library."""
import numpy as np

from tests import connect_model as M
from tests.fake_records import FakeRecords


class ConnectRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(ConnectRecords, self).__init__(size, max_games, max_entries)

    def connect(self, index, rules=1, cut_libs=1, max_region=8, max_nodes=1024, max_pairs=64):
        self.calls.append(("connect", len(index)))
        N, NW = self.S * self.S, (self.S * self.S + 31) // 32
        m = M.connect(self.S, self.last["records"], index, rules=rules, cut_libs=cut_libs, max_region=max_region, max_nodes=max_nodes,
                      max_pairs=max_pairs)
        rows, regions = np.zeros((len(index), max_pairs, M.W), np.int32), np.zeros((len(index), max_pairs, NW), np.uint32)
        groups, counts = np.full((len(index), N), -1, np.int16), np.zeros((len(index), 4), np.int32)
        for i, (r, g) in enumerate(zip(m["rows"], m["regions"])):
            rows[i, :len(r)], regions[i, :len(g)] = r, g
            if m["groups"][i] is not None:
                groups[i], counts[i] = m["groups"][i], m["counts"][i]
        return m["n_pairs"], rows, regions, groups, counts
