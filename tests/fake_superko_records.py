"""tests/fake_records.FakeRecords with the `superko` surface of records.DeviceRecords, served by the model (tests/superko_model.py)
on the records of the last replay: numpy out, no GPU, no library.  Every call's index and first lists are kept."""
import numpy as np

from tests import superko_model as SM
from tests.fake_records import FakeRecords


class SuperkoRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(SuperkoRecords, self).__init__(size, max_games, max_entries)
        self.asked = []

    def superko(self, index, first, rule=0, n_records=None):
        index, first = [int(r) for r in index], [int(f) for f in first]
        self.calls.append(("superko", len(index)))
        self.asked.append((index, first, int(rule), n_records))
        recs = self.last["records"]
        used = len(recs) if n_records is None else int(n_records)
        m = SM.superko(self.S, recs[:used], list(zip(index, first)), int(rule))
        return m["sets"], m["back"], m["counts"]
