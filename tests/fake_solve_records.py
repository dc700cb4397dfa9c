"""tests/fake_records.FakeRecords with the `solve` and `stones` surface of records.DeviceRecords, served by the model
(tests/solve_model.py) on the records of the last replay: numpy out, no GPU, no library."""
import numpy as np

from tests import solve_model as M
from tests.fake_records import FakeRecords


class SolveRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(SolveRecords, self).__init__(size, max_games, max_entries)

    def solve(self, index, rules=1, max_region=12, max_nodes=4096, max_targets=16):
        self.calls.append(("solve", len(index)))
        NW = (self.S * self.S + 31) // 32
        m = M.solve(self.S, self.last["records"], index, rules=rules, max_region=max_region, max_nodes=max_nodes, max_targets=max_targets)
        rows, regions = np.zeros((len(index), max_targets, 8), np.int32), np.zeros((len(index), max_targets, NW), np.uint32)
        for i, (r, g) in enumerate(zip(m["rows"], m["regions"])):
            rows[i, :len(r)], regions[i, :len(g)] = r, g
        return m["n_targets"], rows, regions

    def stones(self, index):
        from sejonggo_amd.tactics import stones_of
        recs = np.asarray(self.last["records"])
        out = np.zeros((len(index), self.S * self.S), np.int8)
        ok = [i for i, r in enumerate(index) if 0 <= r < len(recs)]
        if ok:
            out[ok] = stones_of(self.S, recs[[int(index[i]) for i in ok]])
        return out
