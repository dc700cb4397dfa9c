"""CPU: the superko case set (tests/superko_cases.py) can notice every fault switch of the model (tests/superko_model.py), and the
model gives what include/sgo.h "superko" states in words on the named cases."""
import time

import numpy as np
import pytest

from tests import superko_cases as SC
from tests import superko_model as SM


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ("sets", "back", "counts"))


def _row(S, game, r, f):
    recs, rows, names, bases = SC.case_set(S)
    return names.index("%s_%d_%d" % (game, r, f))


def _bit(sets, i, k, a):
    return bool((int(sets[i, k, a >> 5]) >> (a & 31)) & 1)


@pytest.mark.parametrize("fault", SM.FAULTS)
def test_every_fault_is_noticed_at_the_smallest_size(fault):
    """at 5x5 already, under at least one rule; flag_swapped under both"""
    recs, rows, _, _ = SC.case_set(5)
    hit = [_differs(SM.superko(5, recs, rows, rule, fault), SC.case_model(5, rule)) for rule in (0, 1)]
    assert any(hit), fault
    if fault == "flag_swapped":
        assert all(hit)


@pytest.mark.parametrize("S", (7, 9, 13, 19))
def test_faults_at_the_larger_sizes(S):
    recs, rows, _, _ = SC.case_set(S)
    for fault in SM.FAULTS:
        assert any(_differs(SM.superko(S, recs, rows, rule, fault), SC.case_model(S, rule)) for rule in (0, 1)), (S, fault)


@pytest.mark.parametrize("S", SM.SIZES)
def test_named_cases(S):
    """the figures the definition names, for both colours"""
    N = S * S
    P = lambda x, y: y * S + x                                                           # noqa: E731
    m0, m1 = SC.case_model(S, 0), SC.case_model(S, 1)
    for c in "bw":
        for m in (m0, m1):                                           # the simple ko: back 1, in repeat, not in extra
            i = _row(S, "ko_" + c, 1, 0)
            assert m["back"][i, P(2, 0)] == 1 and _bit(m["sets"], i, 0, P(2, 0)) and not _bit(m["sets"], i, 1, P(2, 0))
            assert m["counts"][i, :2].tolist() == [1, 0] and m["counts"][i, 3] == -1 and not _bit(m["sets"], i, 2, P(2, 0))
            assert _bit(m["sets"], i, 2, N) and m["counts"][i, 5] == 2
        i = _row(S, "send_two_" + c, 2, 0)                           # sending two, returning one tells the rules apart
        assert m0["back"][i, P(1, 0)] == 2 and _bit(m0["sets"], i, 1, P(1, 0)) and m0["counts"][i, 1:4].tolist() == [1, 2, P(1, 0)]
        assert m1["back"][i, P(1, 0)] == -1 and m1["counts"][i, :2].tolist() == [0, 0] and _bit(m1["sets"], i, 2, P(1, 0))
        if S >= 7:
            i = _row(S, "triple_ko_" + c, 5, 0)
            for m in (m0, m1):
                assert m["back"][i, P(S - 1, 2)] == 5 and m["counts"][i, 1:4].tolist() == [1, 5, P(S - 1, 2)]
            i = _row(S, "triple_ko_" + c, 5, 1)
            assert m0["counts"][i, 1] == 0
        i1, i2 = _row(S, "passes_" + c, 1, 0), _row(S, "passes_" + c, 2, 0)
        assert (m0["counts"][i1, 4], m1["counts"][i1, 4], m0["counts"][i2, 4], m1["counts"][i2, 4]) == (1, 0, 1, 2)
        # the single-stone suicide: the current stones, 0 back under rule 0, never in extra; under rule 1 only an EARLIER record
        # with the other side to move can hold it
        assert m0["back"][i2, 0] == 0 and not _bit(m0["sets"], i2, 1, 0) and m1["back"][i2, 0] == 1 and not _bit(m1["sets"], i2, 1, 0)
        i = _row(S, "passes_" + c, 0, 0)
        assert m0["back"][i, 0] == 0 and m1["back"][i, 0] == -1
        i = _row(S, "suicide2_" + c, 2, 0)
        assert m0["back"][i, 1] == 2 and m1["back"][i, 1] == 2 and m0["counts"][i, 1] == 0
        i = _row(S, "quiet_" + c, 4, 0)
        q = [N - 1, P(S // 2, S // 2), P(S - 1, 1)]
        assert [int(m0["back"][i, a]) for a in q] == [4, 2, 1] and [int(m1["back"][i, a]) for a in q] == [4, 2, -1]
        # the stone of one ply ago is gone, so the inherited rule takes its point for a ko: in repeat, not in extra
        assert m0["counts"][i, :4].tolist() == [3, 2, 4, N - 1] and not _bit(m0["sets"], i, 1, q[2])
        i = _row(S, "contact_" + c, 2, 0)
        assert m0["back"][i, P(3, 2)] == 2 and (m0["counts"][i, 4], m1["counts"][i, 4]) == (1, 0)
        i = _row(S, "neighbours_" + c, 1, 1)                          # f - 1 and r + 1 hold it, the history does not
        assert m0["counts"][i, 0] == 0 and m0["counts"][_row(S, "neighbours_" + c, 1, 0), 0] == 1
        i = _row(S, "board_suicide_" + c, 1, 0)
        assert m0["back"][i, P(S // 2, S // 2)] == 1 and m1["back"][i, P(S // 2, S // 2)] == 1
        i = _row(S, "full_" + c, 1, 0)
        assert not m0["sets"][i, :2].any() and (m0["back"][i] == -1).all() and m0["counts"][i].tolist() == [0, 0, 0, -1, 1, 2, 0, 0]
    names = SC.case_set(S)[2]
    for i, name in enumerate(names):
        if name.startswith("zero_"):
            assert not m0["sets"][i].any() and (m0["back"][i] == -1).all() and not m0["counts"][i].any()


def test_long_history_and_golden_sample_cost():
    """the 19x19 history of SGO_SUPERKO_MAX_HISTORY(19) records and one more: matches at both ends of the window, nothing from the
    record that fell out of it; and the model's time on the golden sample the device test compares: a few seconds"""
    H = SM.max_history(19)
    recs, rows, names, (a0, a1, a2) = SC.long_history()
    assert H == 1445 and len(recs) == H + 3
    m0, m1 = SC.long_model(0), SC.long_model(1)
    long_, exact, short1, short2 = (names.index(n) for n in ("one_too_long", "exactly_max", "short_by_one", "short_by_two"))
    for m in (m0, m1):
        assert m["counts"][long_, 5:].tolist() == [H, 0, 1] and m["counts"][exact, 5:].tolist() == [H, 0, 0]
        assert m["counts"][short1, 5:].tolist() == [H - 1, 0, 0]
        assert np.array_equal(m["back"][long_], m["back"][exact]) and np.array_equal(m["sets"][long_], m["sets"][exact])
        assert m["back"][long_, a0] == -1 and m["back"][long_, a2] == 1 and m["counts"][long_, 4] == H - 3
    assert m0["back"][exact, a1] == H - 2 and m1["back"][exact, a1] == H - 1          # the oldest record of the window, under rule 1
    assert m0["back"][short1, a1] == H - 2 and m1["back"][short1, a1] == -1 and m0["back"][short2, a1] == -1
    for fault in ("history_before_f", "smallest_h"):
        assert _differs(SM.superko(19, recs, rows[:2], 0, fault), {k: v[:2] for k, v in m0.items()}), fault
    grecs, grows = SC.golden_sample()
    assert 60 <= len(grows) <= 120
    t = time.time()
    g0, g1 = SM.superko(19, grecs, grows, 0), SM.superko(19, grecs, grows, 1)
    assert time.time() - t < 20.0
    assert g0["counts"][:, 5].max() > 300 and (g0["counts"][:, 7] == 0).all() and (g1["counts"][:, 0] <= g0["counts"][:, 0]).all()
