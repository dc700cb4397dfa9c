"""CPU: the power of the light-playout case set.  Every fault switch of tests/playout_model.py changes the expected outputs of the
runs of tests/playout_cases.py at EVERY board size, so a kernel with that slip cannot pass tests/test_gpu_playout.py; and the
condition of the golden rows holds: under rules = 1 and the default cap the MODEL leaves at most 2 % of their playouts capped.

Found here (the model, every 16th position of the five golden 19x19 games, one playout each): see GOLDEN_CAPPED below.  The designed
runs (`end`, `short`, `counts`) notice every switch on their own; the whole games add the positions nobody designed."""
import numpy as np
import pytest

from tests import playout_cases as PC
from tests import playout_model as PM

# runs tried in this order until one notices the switch; the cheap ones first
ORDER = ("counts_2", "short_r1", "short_r0", "end_r1", "end_r0")
GOLDEN_CAPPED = 0          # of the golden playouts the model left capped when this file was written


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ("own", "amaf", "sums"))


@pytest.mark.parametrize("S", PM.SIZES)
def test_every_fault_switch_is_noticed(S):
    missed = []
    for fault in PM.FAULTS:
        if not any(_differs(PC.run_model(S, name), PC.run_model(S, name, fault)) for name in ORDER):
            missed.append(fault)
    assert not missed, (S, missed)


def test_the_cases_are_what_they_claim():
    """two passes, ply 2, not capped without a candidate; the root ko ban is read; rules 0 and 1 differ in the first ply of `connect`;
    max_plies = 1 caps every playout; the full board scores its stones"""
    for S in PM.SIZES:
        names, recs = PC.case_records(S)
        N = S * S
        at = lambda nm: names.index(nm)                                                   # noqa: E731
        for rules in (0, 1):
            bo, wo, first, ply, capped = PM.play_out(S, recs[at("none")], 1, 0, rules, 0)
            assert (ply, capped, int(first.sum())) == (2, False, 0)
            bo, wo, first, ply, capped = PM.play_out(S, recs[at("full")], 1, 0, rules, 0)
            assert (ply, capped) == (2, False) and int(bo.sum()) + int(wo.sum()) == N
            tr = []
            PM.play_out(S, recs[at("ko_ban")], 1, 0, rules, 0, trace=tr)
            assert tr[0] == N                                         # white may not retake: it passes
            tr = []
            PM.play_out(S, recs[at("ko_free")], 1, 0, rules, 0, trace=tr)
            assert tr[:2] == [2 * S + 1, N]                           # white retakes, black is banned inside the playout and passes
            tr = []
            PM.play_out(S, recs[at("connect")], 1, 0, rules, 0, trace=tr)
            assert tr[0] == (2 * S + 1 if rules else N)
            assert PM.play_out(S, recs[at("empty")], 1, 0, rules, 1)[3:] == (1, True)


def test_the_golden_rows_end_on_their_own():
    """the condition of the golden test: at most 2 % of the model's playouts capped under rules = 1 and the default cap"""
    want = PC.golden_model()
    total, capped = int(want["sums"][:, 7].sum()), int(want["sums"][:, 6].sum())
    print("golden rows %d, playouts %d, capped %d" % (len(want["sums"]), total, capped))
    assert total == PC.GOLDEN_PER_ROW * len(PC.golden_records()) and total >= 100
    assert capped * 50 <= total, (capped, total)
    assert capped == GOLDEN_CAPPED
