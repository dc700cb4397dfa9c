"""tests/fake_life_records.LifeRecords with the `influence` surface of records.DeviceRecords, served by the model
(tests/influence_model.py) on the records of the last replay: numpy out, no GPU, no library.  dead "life" lifts what the life
model proves dead, as the device route does: white stones in terr_black and black stones in terr_white."""
import numpy as np

from tests import influence_model as M
from tests import life_model
from tests.fake_life_records import LifeRecords


class InfluenceRecords(LifeRecords):
    def influence(self, index, dead=None, dilate=5, erode_moyo=10, erode_terr=21):
        self.calls.append(("influence", len(index), dead if dead is None or isinstance(dead, str) else "given",
                           (dilate, erode_moyo, erode_terr)))
        recs = np.asarray(self.last["records"], dtype=np.uint32)
        NW = (self.S * self.S + 31) // 32
        if isinstance(dead, str):
            assert dead == "life"
            sets = life_model.life(self.S, recs, index)["sets"]
            ok = (np.asarray(index) >= 0) & (np.asarray(index) < len(recs))
            planes = recs[np.where(ok, index, 0)][:, :2 * NW]
            dead = (sets[:, 2] & planes[:, NW:]) | (sets[:, 3] & planes[:, :NW])
        m = M.influence(self.S, recs, index, dead, dilate, erode_moyo, erode_terr)
        return m["values"], m["sets"], m["counts"]
