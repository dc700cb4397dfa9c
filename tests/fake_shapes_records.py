"""tests/fake_records.FakeRecords with the `shapes` surface of records.DeviceRecords, served by the model (tests/shapes_model.py)
on the records of the last replay: numpy out, no GPU, no library."""
from tests import shapes_model as M
from tests.fake_records import FakeRecords


def model_shape(shape):
    """the model's Shape of a sejonggo_amd.shapes.Shape (the cell codes are the header's in both)"""
    return M.Shape(shape.w, shape.h, shape.edges, tuple(tuple(r) for r in shape.cells))


class ShapesRecords(FakeRecords):
    def __init__(self, size, max_games, max_entries, device=0):
        super(ShapesRecords, self).__init__(size, max_games, max_entries)

    def shapes(self, index, shape):
        self.calls.append(("shapes", len(index)))
        m = M.shapes(self.S, self.last["records"], model_shape(shape), index)
        return m["hits"], m["cover"]
