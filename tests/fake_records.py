"""A stand-in for records.DeviceRecords without a GPU: the replay is the model's (tests/records_model.py, the oracle's rules), the
boards are the oracle's.  It has the surface RecordSet.replay and RecordSet.write_samples drive, and records every call."""
import numpy as np

from tests import records_model as M


class FakeRecords(object):
    def __init__(self, size, max_games, max_entries):
        self.S, self.max_games, self.max_entries = size, int(max_games), int(max_entries)
        self.calls = []
        self.last = None

    def replay(self, n_entries, off, actions, colors):
        n_entries = [int(v) for v in n_entries]
        assert len(n_entries) <= self.max_games and sum(n_entries) <= self.max_entries
        games = [([int(a) for a in actions[o:o + n]], [int(c) for c in colors[o:o + n]]) for n, o in zip(n_entries, off)]
        self.last = M.replay(self.S, games)
        self.calls.append(("replay", len(games), sum(n_entries)))
        return self.last["status"].copy(), self.last["fail_at"].copy()

    def boards(self, index):
        self.calls.append(("boards", len(index)))
        for i in index:
            assert self.last["written"][int(i)], "a record the replay did not write was asked for"
        if not len(index):
            return np.zeros((0, self.S, self.S, 17), np.int32)
        return np.concatenate([self.last["boards"][int(i)] for i in index]).astype(np.int32)

    def close(self):
        self.calls.append(("close",))
