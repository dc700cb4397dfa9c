"""CPU: the model of the securing-move table (tests/secure_model.py) plays the project's rules -- its positions after a ply are
oracle.make_play and its ALLOWED bits oracle.legal_moves on every case -- its table is life_model.point_life applied to those
positions (the second formulation: the board tensor the oracle leaves, read back, through the two-colour entry of the life model),
the constructed cases (tests/secure_cases.py) hold what they were built for, and every fault switch of the model changes a compared
word of a named case: so a green run of tests/test_gpu_secure.py means something.

ARGUED, not shown -- `suicide_kept`.  No position can show it.  Let C be the mover's chain on a after the captures, without a
liberty.  Executed: the points of C are empty in P'.  No surviving chain of the mover touches them (a stone of the mover next to C
would belong to C), so the region that holds them has an empty point that touches no surviving chain: it is vital to none of them.
Kept: C stays, a chain without a liberty; a vital region needs an empty point next to the chain, so C has no vital region and goes
in the first pass, and with it every region next to C -- which are exactly the pieces the executed region falls into when C is
taken out of it (each piece was joined to the rest through C).  Either way no surviving chain counts that region, none of its
points is territory, and every other chain and region is the same in both positions: the fixed point, and with it alive, terr and
dead, agree.  SUICIDE itself is read from the rules' ply in both.  test_suicide_kept_is_inert checks this on every suicide point the
case set holds."""
import numpy as np
import pytest

from oracle import oracle
from tests import life_model as LM
from tests import secure_cases as SC
from tests import secure_model as M

# fault -> (board size, case name, side): the case whose compared words the switch changes
NOTICED_BY = {
    "captures_kept": (5, "capture_makes_eye_sb", 0),
    "stone_not_placed": (5, "corner3_sb", 0),
    "base_for_every_point": (5, "two_eyes_sb", 0),
    "opponent_benson": (5, "two_eyes_sw", 0),
    "dead_from_before": (5, "capture_makes_eye_sw", 1),
    "summary_over_all_empty": (5, "two_eyes_sb", 0),
    "ko_on_side1": (5, "ko_secure_sw", 1),
    "best_highest_on_tie": (5, "corner3_sb", 0),
    "best_sets_of_base": (5, "straight_three_sb", 0),
    "gain_alive_only": (5, "corner3_sb", 0),
    "flag_as_stone": (5, "edge_eyes_sw", 0),
}
ARGUED = ("suicide_kept",)


def _board(S, rec, side):
    """the board tensor oracle.legal_moves / make_play take, for the mover of (record, side): plane 0 own, 1 opp, 2 prev"""
    own, opp, prev, _ = M.read_record(S, rec, side)
    flat = np.zeros((S * S, 17), np.int32)
    flat[sorted(own), 0] = 1
    flat[sorted(opp), 1] = 1
    flat[sorted(prev if prev is not None else own), 2] = 1
    mover_white = bool(int(rec[(S * S + 31) // 32 - 1]) >> 31) != (side == 1)
    flat[:, 16] = -1 if mover_white else 1
    return np.ascontiguousarray(flat.reshape(1, S, S, 17))


def _check_case(S, rec, side, table, points=None):
    """ALLOWED == oracle.legal_moves on every point; on the listed empty points (None: all) P' == oracle.make_play, and the table
    row is life_model.point_life of the board the ORACLE left (the mover's colour picked out of its two-colour answer)"""
    N = S * S
    b = _board(S, rec, side)
    assert np.array_equal(1 - oracle.legal_moves(b)[:N], table[:, 0] & M.ALLOWED), "ALLOWED is not sgo_legal_moves"
    for a in (range(N) if points is None else points):
        if table[a, 0] & M.OCCUPIED:
            assert not table[a, 1:].any()
            continue
        child = b.copy()
        oracle.make_play(a % S, a // S, child)
        flat = child.reshape(N, 17)                                  # after the ply the mover's stones are plane 1
        own, opp = np.flatnonzero(flat[:, 1]).tolist(), np.flatnonzero(flat[:, 0]).tolist()
        assert (own, opp) == M.after_ply(S, rec, a, side), a
        life = LM.point_life(S, own, opp)                            # "black" = the mover
        assert table[a, 1:].tolist() == [life["counts"][0], life["counts"][2], life["counts"][4]], a
        assert bool(table[a, 0] & M.SUICIDE) == (a not in own)


@pytest.mark.parametrize("S", M.SIZES)
def test_model_plays_the_oracles_rules_on_every_case(S):
    """Every case record, both sides: ALLOWED on every point.  P' and the second formulation of the table on every empty point up to
    9x9; at 13x13 and 19x19 (where the oracle's ply and a second Benson per point are the slow part) on every seventh (13x13) or thirteenth
    (19x19) point, the offset moving with the record, and on best_move."""
    names, recs = SC.case_records(S)
    for side in (0, 1):
        m = SC.case_model(S, side)
        for i in range(len(recs)):
            points = None
            if S > 9:
                step = 7 if S == 13 else 13
                points = sorted(set(range(i % step, S * S, step)) | ({int(m["counts"][i, 6])} if m["counts"][i, 6] >= 0 else set()))
            _check_case(S, recs[i], side, m["table"][i], points)


def test_model_plays_the_oracles_rules_on_the_golden_sample():
    """the 26 golden positions: ALLOWED on every point, P' and the second formulation on every 23rd point and on best_move"""
    recs = SC.golden_sample()
    for side in (0, 1):
        m = SC.golden_model(side)
        for i in range(len(recs)):
            points = sorted(set(range(i % 23, 361, 23)) | ({int(m["counts"][i, 6])} if m["counts"][i, 6] >= 0 else set()))
            _check_case(19, recs[i], side, m["table"][i], points)


def test_counts_and_sets_follow_from_the_table():
    """counts 0..2 and sets 0 / 1 are life_model.point_life of the position itself; counts 3..7 and sets 2 / 3 follow from the table
    by the header's words"""
    for S in (5, 9):
        names, recs = SC.case_records(S)
        for side in (0, 1):
            m = SC.case_model(S, side)
            for i in range(len(recs)):
                own, opp, _, _ = M.read_record(S, recs[i], side)
                life = LM.point_life(S, sorted(own), sorted(opp))
                c, t = m["counts"][i], m["table"][i].astype(np.int64)
                assert c[:3].tolist() == [life["counts"][0], life["counts"][2], life["counts"][4]]
                assert LM.points_of(m["sets"][i, 0], S * S) == sorted(life["alive"][0]) and LM.points_of(m["sets"][i, 1], S * S) == sorted(life["terr"][0])
                ok = (t[:, 0] & M.ALLOWED) != 0
                gain = t[:, 1] + t[:, 2] - c[0] - c[1]
                assert c[3] == ok.sum() and c[4] == (ok & (gain > 0)).sum() and c[7] == (ok & (gain < 0)).sum()
                if ok.any():
                    assert c[5] == gain[ok].max() and c[6] == np.flatnonzero(ok & (gain == c[5]))[0]
                    own2, opp2 = M.after_ply(S, recs[i], int(c[6]), side)
                    star = LM.point_life(S, own2, opp2)
                    assert LM.points_of(m["sets"][i, 2], S * S) == sorted(star["alive"][0])
                    assert LM.points_of(m["sets"][i, 3], S * S) == sorted(star["terr"][0])
                else:
                    assert c[5] == 0 and c[6] == -1 and np.array_equal(m["sets"][i, 2:], m["sets"][i, :2])


def _row(S, name, side, fault=None):
    names, recs = SC.case_records(S)
    i = names.index(name)
    if fault is None:
        m = SC.case_model(S, side)
        return m["table"][i], m["sets"][i], m["counts"][i]
    return M.record_secure(S, recs[i], side, fault)


@pytest.mark.parametrize("fault", sorted(NOTICED_BY))
def test_fault_switch_changes_a_named_case(fault):
    S, name, side = NOTICED_BY[fault]
    good, bad = _row(S, name, side), _row(S, name, side, fault)
    assert not all(np.array_equal(g, b) for g, b in zip(good, bad)), (fault, name)


def test_every_switch_is_shown_or_argued():
    assert set(M.FAULTS) == set(NOTICED_BY) | set(ARGUED) and not set(NOTICED_BY) & set(ARGUED) and len(M.FAULTS) >= 10


def test_suicide_kept_is_inert():
    """the argument of the module docstring, checked on every record of the case set up to 9x9 that has a suicide point"""
    seen = 0
    for S in (5, 7, 9):
        names, recs = SC.case_records(S)
        for side in (0, 1):
            m = SC.case_model(S, side)
            for i in np.flatnonzero(((m["table"][:, :, 0] & M.SUICIDE) != 0).any(axis=1)):
                bad = M.record_secure(S, recs[i], side, "suicide_kept")
                assert all(np.array_equal(m[k][i], b) for k, b in zip(("table", "sets", "counts"), bad)), (S, names[i], side)
                seen += 1
    assert seen >= 20


def _gain(S, name, side, a):
    table, _, counts = _row(S, name, side)
    return int(table[a, 1]) + int(table[a, 2]) - int(counts[0]) - int(counts[1])


@pytest.mark.parametrize("S", M.SIZES)
def test_cases_hold_what_they_were_built_for(S):
    A, O, K, X = M.ALLOWED, M.OCCUPIED, M.KO, M.SUICIDE
    N = S * S
    flags = lambda name, side, a: int(_row(S, name, side)[0][a, 0])                      # noqa: E731
    counts = lambda name, side: _row(S, name, side)[2].tolist()                          # noqa: E731
    # the empty board: a lone stone proves nothing, anywhere
    table, sets, c = _row(S, "empty_sw", 0)
    assert (table[:, 0] == A).all() and not table[:, 1:].any() and not sets.any() and c.tolist() == [0, 0, 0, N, 0, 0, 0, 0]
    # corner3: the corner point touches no stone; a stone on any of the three points makes the rest of the region vital
    assert [_gain(S, "corner3_sb", 0, a) for a in (0, 1, S)] == [15, 15, 15] and counts("corner3_sb", 0)[4:7] == [3, 15, 0]
    assert counts("corner3_sb", 0)[:3] == [0, 0, 0] and counts("corner3_cw", 0) == counts("corner3_sb", 0) == counts("corner3_sw", 1)
    # two_eyes: filling either eye loses all nine, and neither is ALLOWED -- so nothing harmful is counted
    assert [_gain(S, "two_eyes_sb", 0, a) for a in (0, S + 1)] == [-9, -9] and flags("two_eyes_sb", 0, 0) == flags("two_eyes_sb", 0, S + 1) == 0
    assert counts("two_eyes_sb", 0)[:3] == [7, 2, 0] and counts("two_eyes_sb", 0)[7] == 0
    # straight_three: the middle point makes two eyes (8 = six stones and two points)
    assert _gain(S, "straight_three_sb", 0, 1) == 8 and _gain(S, "straight_three_sb", 0, 0) == _gain(S, "straight_three_sb", 0, 2) == 0
    if S > 5:                                                        # at 5x5 the board's right edge closes a second eye space
        assert counts("straight_three_sb", 0)[4:7] == [1, 8, 1]
    # capture_makes_eye: the capturing stone splits the region in two; dead counts nothing, the stones are gone
    table, sets, c = _row(S, "capture_makes_eye_sb", 0)
    assert table[1].tolist() == [A, 7, 3, 0] and c[4:7].tolist() == [1, 10, 1] and LM.points_of(sets[3], N) == [0, 2, 3]
    assert _row(S, "capture_makes_eye_sb", 0, "captures_kept")[0][1].tolist() == [A, 0, 0, 0]
    # capture_opens_eye: ALLOWED, captures five, and the group's life is gone; the one harmful point of the case set's design
    table, sets, c = _row(S, "capture_opens_eye_sb", 0)
    assert c[:3].tolist() == [14, 7, 5] and table[1].tolist() == [A, 0, 0, 0] and c[7] == 1 and _gain(S, "capture_opens_eye_sb", 0, 1) == -21
    assert table[3 * S].tolist() == [0, 0, 0, 0]                     # the other eye: as harmful, but not ALLOWED
    # connect: neither chain lives alone; either joining point makes one chain with two eyes
    c = counts("connect_sb", 0)
    assert c[:3] == [0, 0, 0] and c[4] == (3 if S == 7 else 2) and c[5] == (10 if S == 5 else 12)       # 7x7: the edge closes a third and _gain(S, "connect_sb", 0, 2) == c[5] - 1
    # the ko point that would secure: KO and not ALLOWED for the side to move; ALLOWED for the same colour through side 1
    assert flags("ko_secure_sb", 0, 1) == K and _gain(S, "ko_secure_sb", 0, 1) == 8 and flags("ko_secure_sw", 1, 1) == A
    assert counts("ko_secure_sw", 1)[5:7] == ([10, 9] if S == 5 else [8, 1])
    if S > 5:
        assert counts("ko_secure_sb", 0)[4:7] == [0, 0, 0]
    assert flags("ko_secure_cw", 0, 1) == K and flags("ko_secure_cb", 0, 1) == A         # swapped: the ko is white's alone
    assert flags("ko_secure_sb", 0, 2) == O
    # a suicide point: SUICIDE, not ALLOWED, and the life of the board without the two stones
    assert _row(S, "suicide_sb", 0)[0][1].tolist() == [X, 0, 0, 0] and flags("suicide_sw", 0, 1) == A
    if S == 5:
        assert counts("settled_sb", 0) == [13, 2, 0, 0, 0, 0, -1, 0] and counts("settled_cb", 0) == [8, 2, 0, 0, 0, 0, -1, 0]
    if S >= 7:
        # cascade: the move that closes the open head saves the whole snake
        c = counts("cascade_sb", 0)
        assert c[:3] == [0, 0, 0] and c[4] == 2 and c[6] == 2 and _gain(S, "cascade_sb", 0, 2) == _gain(S, "cascade_sb", 0, 2 * S) == c[5]
        assert c[5] == {7: 20, 9: 26, 13: 38, 19: 56}[S]


def test_word_boundaries_at_19():
    """`word_bounds`: eyes on 31 and 33 around a stone on 32, 63 / 65 around 64, 338 / 340 under a wall that ends on 360 -- the table rows and the set
    words on both sides of the boundaries"""
    table, sets, c = _row(19, "word_bounds_sb", 0)
    assert c[0] > 0 and c[1] >= 4 and {31, 33, 338, 340} <= set(LM.points_of(sets[1], 361)) and {32, 360} <= set(LM.points_of(sets[0], 361))
    assert table[31, 0] == 0 and table[32, 0] == M.OCCUPIED and _gain(19, "word_bounds_sb", 0, 31) < 0
    table, sets, c = _row(19, "word_bounds_sw", 0)
    assert {63, 65} <= set(LM.points_of(sets[1], 361)) and 64 in LM.points_of(sets[0], 361)


def test_what_the_case_set_reaches():
    """The counts the case set reaches, pinned: records with a securing move, records with a harmful ALLOWED move, the largest gain;
    on the golden sample the share with securing > 0 beside the share with base > 0 -- the one-ply lookahead speaks no later than
    life does."""
    reach = {}
    for S in M.SIZES:
        sec = harm = 0
        best = -1000
        for side in (0, 1):
            c = SC.case_model(S, side)["counts"]
            sec, harm, best = sec + int((c[:, 4] > 0).sum()), harm + int((c[:, 7] > 0).sum()), max(best, int(c[:, 5].max()))
        reach[S] = (sec, harm, best)
    assert reach == REACH, reach
    golden = {}
    for side in (0, 1):
        c = SC.golden_model(side)["counts"]
        golden[side] = (len(c), int((c[:, 4] > 0).sum()), int(((c[:, 0] + c[:, 1]) > 0).sum()), int(c[:, 5].max()), int((c[:, 7] > 0).sum()))
    assert golden == GOLDEN, golden


# S -> (records x sides with securing > 0, with harmful > 0, the largest best_gain)
REACH = {5: (48, 4, 15), 7: (50, 4, 20), 9: (50, 4, 26), 13: (50, 4, 38), 19: (62, 4, 56)}
# side -> (positions, with securing > 0, with base > 0, the largest best_gain, with harmful > 0)
GOLDEN = {0: (26, 4, 4, 41, 1), 1: (26, 4, 2, 24, 1)}
