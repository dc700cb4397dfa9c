"""tests/fake_playout_records.PlayoutRecords with the `uct` surface of records.DeviceRecords, served by the model (tests/uct_model.py) on
the records of the last replay: numpy out, no GPU, no library.  Every call's arguments are kept."""
from tests import uct_model as UM
from tests.fake_playout_records import PlayoutRecords


class UctRecords(PlayoutRecords):
    def uct(self, index, trees, sims, seed=0, rules=1, max_plies=0, komi2=0, expand_at=2, rave_equiv=256, prior=4, max_nodes=None):
        index = [int(r) for r in index]
        self.calls.append(("uct", len(index)))
        self.asked.append((index, int(trees), int(sims), int(seed), int(rules), int(max_plies), int(komi2), int(expand_at), int(rave_equiv), int(prior),
                           max_nodes))
        m = UM.search(self.S, self.last["records"], index, int(trees), int(sims), int(seed), int(rules), int(max_plies), int(komi2), int(expand_at),
                      int(rave_equiv), int(prior), max_nodes)
        return m["visits"], m["wins2"], m["rave"], m["own"], m["sums"], m["info"]
