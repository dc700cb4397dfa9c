"""tests/fake_records.FakeRecords with the `secure` and `to_play` surface of records.DeviceRecords, served by the model
(tests/secure_model.py) on the records of the last replay: numpy out, no GPU, no library."""
import numpy as np

from tests import secure_model as M
from tests.fake_records import FakeRecords


class SecureRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(SecureRecords, self).__init__(size, max_games, max_entries)

    def secure(self, index, side=0):
        self.calls.append(("secure", len(index)))
        m = M.secure(self.S, self.last["records"], index, side)
        return m["table"], m["sets"], m["counts"]

    def to_play(self, index):
        recs, NW = self.last["records"], (self.S * self.S + 31) // 32
        return np.array([0 if not 0 <= r < len(recs) else (-1 if int(recs[int(r)][NW - 1]) >> 31 else 1) for r in index], np.int8)
