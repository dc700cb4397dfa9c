"""CPU: the model of the move-outcome table (tests/moves_model.py) plays the project's rules -- its ALLOWED bits are
oracle.legal_moves and its positions after a ply are oracle.make_play, on every constructed case and on the replayed golden rule
games, whose legal masks the reference itself pinned -- the constructed cases (tests/moves_cases.py) hold what they were built for,
and every fault switch of the model changes a compared value of a named case: so a green run of tests/test_gpu_moves.py means
something."""
import numpy as np
import pytest

from oracle import oracle
from tests import moves_cases as MC
from tests import moves_model as M
from tests.helpers import load, unpack_mask
from tests.rollout_model import pack_boards

# fault -> (board size, case name, side): the case whose compared values the switch changes
NOTICED_BY = {
    "capture_after_suicide": (5, "ko_two_gone_w", 0),
    "libs_before_lift": (5, "snapback_w", 0),
    "weakest_without_a": (5, "join4_b", 0),
    "joined_stones": (5, "twice_b", 0),
    "ataris_anywhere": (5, "two_chains_b", 0),
    "allowed_not_suicide": (5, "forbidden_sound_b", 0),
    "ko_wrong_plane": (5, "ko_w", 0),
    "ko_at_side1": (5, "ko_b", 1),
    "flag_as_stone": (5, "empty_w", 0),
    "padding_read": (5, "empty_b", 0),
    "max_move_highest": (5, "two_chains_b", 0),
    "quiet_no_edge": (7, "empty_b", 0),
}
FIELDS = ("flags", "captured", "size", "libs", "joined", "weakest", "ataris", "atari_stones")


def _board(S, rec, side):
    """the board tensor oracle.legal_moves / make_play take, for the mover of (record, side): plane 0 own, 1 opp, 2 prev"""
    board, prev, area, mover_white = M.read_record(S, rec, side)
    flat = np.zeros((S * S, 17), np.int32)
    flat[[a for a in range(area) if board[a] == M.OWN], 0] = 1
    flat[[a for a in range(area) if board[a] == M.OPP], 1] = 1
    flat[sorted(prev) if prev is not None else [a for a in range(area) if board[a] == M.OWN], 2] = 1
    flat[:, 16] = -1 if mover_white else 1
    return np.ascontiguousarray(flat.reshape(1, S, S, 17))


def _check_against_oracle(S, rec, side, rows, points=None):
    N = S * S
    b = _board(S, rec, side)
    allowed = 1 - oracle.legal_moves(b)[:N]
    assert np.array_equal(allowed, rows[:, 0] & M.ALLOWED), "ALLOWED is not sgo_legal_moves"
    for a in (range(N) if points is None else points):
        if rows[a, 0] & M.OCCUPIED:
            continue
        child = b.copy()
        oracle.make_play(a % S, a // S, child)
        own, opp = M.after_ply(S, rec, a, side)
        flat = child.reshape(N, 17)                                  # after the ply the mover's stones are plane 1
        assert np.flatnonzero(flat[:, 1]).tolist() == own and np.flatnonzero(flat[:, 0]).tolist() == opp, a
        assert int(rows[a, 1]) == int(b[..., 1].sum()) - len(opp)
        assert bool(rows[a, 0] & M.SUICIDE) == (a not in own)


@pytest.mark.parametrize("S", M.SIZES)
def test_model_plays_the_oracles_rules_on_every_case(S):
    """ALLOWED on every point of every case record, both sides.  P' == oracle.make_play on every empty point of every constructed
    case at all five sizes (the straddling chain at 19x19 among them) and of the rule shapes up to 9x9; on the rule shapes at 13x13
    and 19x19 on every third point, the offset moving with the record (the oracle's ply is the slow part)."""
    names, recs = MC.case_records(S)
    for side in (0, 1):
        rows = MC.case_model(S, side)["rows"]
        for i in range(len(recs)):
            thin = S > 9 and names[i].startswith("shape_")
            _check_against_oracle(S, recs[i], side, rows[i], range(i % 3, S * S, 3) if thin else None)


@pytest.mark.parametrize("S", [5, 9, 13])
def test_model_agrees_with_the_pinned_rule_games(S):
    """rules_S*.npz: games the reference played, with the legal mask it gave after every ply.  Replayed by the oracle; the model
    reads the packed record of every position: its ALLOWED bits are the reference's mask, the played move's P' is the next board."""
    z = load("rules_S%d.npz" % S)
    N, seen = S * S, 0
    for gi in range(int(z["n_games"])):
        p = "g%02d_" % gi
        board, _ = oracle.game_init(S)
        masks = z[p + "masks"]
        for ply, (x, y, colour) in enumerate(z[p + "moves"]):
            if ply % 3 == 0:                                         # every third position of every game
                rec = pack_boards(board)[0]
                rows, counts = M.record_moves(S, rec, 0)
                assert np.array_equal(rows[:, 0] & M.ALLOWED, 1 - unpack_mask(masks[ply], N + 1)[:N]), (gi, ply)
                assert counts[0] == int((rows[:, 0] & M.ALLOWED).sum())
                if y < S and colour == 0:                            # a move in turn: the mover is the record's side to move
                    _check_against_oracle(S, rec, 0, rows, [int(y) * S + int(x)])
                seen += 1
            oracle.make_play(int(x), int(y), board, None if colour == 0 else int(colour))
    assert seen >= 20                                                # the fixture is there


def _row(S, name, side, fault=None):
    names, recs = MC.case_records(S)
    i = names.index(name)
    if fault is None:
        m = MC.case_model(S, side)
        return m["rows"][i], m["counts"][i]
    return M.record_moves(S, recs[i], side, fault)


def _move(S, name, side, x, y):
    return dict(zip(FIELDS, (int(v) for v in _row(S, name, side)[0][y * S + x])))


@pytest.mark.parametrize("fault", M.FAULTS)
def test_fault_switch_changes_a_named_case(fault):
    S, name, side = NOTICED_BY[fault]
    good, bad = _row(S, name, side), _row(S, name, side, fault)
    assert not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])), (fault, name)


def test_every_switch_is_shown():
    """No switch of the model is inert: each has its named case, none needs an argument why no position can show it."""
    assert set(M.FAULTS) == set(NOTICED_BY) and len(M.FAULTS) >= 12


@pytest.mark.parametrize("S", [5, 7, 9])
def test_cases_hold_what_they_were_built_for(S):
    A, O, K, X = M.ALLOWED, M.OCCUPIED, M.KO, M.SUICIDE
    N = S * S
    mv = lambda name, side, x, y: _move(S, name, side, x, y)                            # noqa: E731
    # the empty board: every point allowed, 2 / 3 / 4 liberties, nothing else; the same for either colour and side
    rows, counts = _row(S, "empty_w", 0)
    libs = rows[:, 3].reshape(S, S)
    assert libs[0, 0] == libs[0, S - 1] == libs[S - 1, 0] == libs[S - 1, S - 1] == 2 and libs[0, 1] == libs[S - 1, S - 2] == libs[1, 0] == 3
    assert (libs[1:-1, 1:-1] == 4).all() and (rows[:, 0] == A).all() and (rows[:, 2] == 1).all() and not rows[:, [1, 4, 5, 6, 7]].any()
    assert counts.tolist() == [N, 0, 0, -1, 0, 0, 0, 0] and np.array_equal(rows, _row(S, "empty_b", 1)[0])
    # the ko: white's retake at (1,1) would capture one stone and is KO, not ALLOWED; with two stones gone, or for side 1 of the
    # record with black to move (white again, without prev), it is allowed
    assert mv("ko_w", 0, 1, 1) == dict(flags=K, captured=1, size=1, libs=1, joined=0, weakest=0, ataris=1, atari_stones=1)
    assert mv("ko_two_gone_w", 0, 1, 1)["flags"] == A and mv("ko_b", 1, 1, 1)["flags"] == A
    assert _row(S, "ko_w", 0)[1][1] == 0 and _row(S, "ko_two_gone_w", 0)[1][1:4].tolist() == [1, 1, S + 1]
    assert mv("ko_b", 0, 1, 1)["flags"] == 0 and _row(S, "ko_b", 0)[1][7] == 2       # black filling an eye, (1,1) or (0,0): forbidden, but sound
    # snapback: white takes one and stands on one liberty (no self-atari: it captured); black takes four
    assert mv("snapback_w", 0, 1, 0) == dict(flags=A, captured=1, size=5, libs=1, joined=1, weakest=1, ataris=0, atari_stones=0)
    assert _row(S, "snapback_w", 0)[1][4] == (1 if S == 5 else 0) and mv("snapback_b", 0, 1, 0)["captured"] == 4
    # a two-stone suicide: nothing else is set, and it is no forbidden-sound point
    assert mv("suicide2_b", 0, 1, 0) == dict(flags=X, captured=0, size=0, libs=0, joined=1, weakest=1, ataris=0, atari_stones=0)
    assert _row(S, "suicide2_b", 0)[1][7] == 0
    # two chains with one stone: no empty neighbour, allowed because it captures; the far corner captures two as well, later
    m = mv("two_chains_b", 0, 1, 0)
    assert m["flags"] == A and m["captured"] == 2 and mv("two_chains_b", 0, S - 1, S - 2)["captured"] == 2
    assert _row(S, "two_chains_b", 0)[1][1:4].tolist() == [2, 2, 1] and _row(S, "two_chains_b", 0, "max_move_highest")[1][3] == N - S - 1
    assert mv("two_chains_w", 1, 1, 0) == m                                              # side 1 of the other record: the same mover
    # four chains joined, the weakest with one liberty -- and no empty neighbour, so the inherited rule forbids the connection
    assert mv("join4_b", 0, 2, 2) == dict(flags=0, captured=0, size=6, libs=6, joined=4, weakest=1, ataris=0, atari_stones=0)
    assert mv("forbidden_sound_b", 0, 0, 0) == dict(flags=0, captured=0, size=4, libs=4, joined=1, weakest=5, ataris=0, atari_stones=0)
    assert _row(S, "forbidden_sound_b", 0)[1][7] == 1 and mv("forbidden_sound_w", 0, 0, 0)["flags"] == X
    # a chain that touches the point twice counts once, as a joined chain and as a chain in atari
    assert mv("twice_b", 0, 2, 2)["joined"] == 1 and mv("twice_b", 0, 2, 2)["weakest"] == 2
    m = mv("twice_w", 0, 2, 2)
    assert (m["ataris"], m["atari_stones"]) == (1, 3) and mv("twice_b", 0, 2, 2, ) != m
    # the full board: black's last point is a suicide of N stones, white's captures N - 1
    c = S // 2
    assert mv("full_minus_one_b", 0, c, c)["flags"] == X and _row(S, "full_minus_one_b", 0)[1].tolist() == [0, 0, 0, -1, 0, 0, 0, 0]
    assert mv("full_minus_one_w", 0, c, c) == dict(flags=A, captured=N - 1, size=1, libs=4, joined=0, weakest=0, ataris=0, atari_stones=0)
    assert (_row(S, "full_minus_one_w", 0)[0][:, 0] == O).sum() == N - 1


def test_the_straddling_chain():
    """19x19: the black chain of `straddle` runs over the word boundaries 31 | 32 and 127 | 128 of the packed plane; the points
    beside it see all 15 stones"""
    S = 19
    names, recs = MC.case_records(S)
    black = {a for a in range(S * S) if recs[names.index("straddle_b")][a >> 5] >> (a & 31) & 1}
    assert {31, 32, 127, 146} <= black and len(black) == 15
    m = _move(S, "straddle_b", 0, 12, 0)
    assert m["size"] == 16 and m["joined"] == 1 and _move(S, "straddle_w", 0, 12, 0)["size"] == 1
    assert _row(S, "straddle_b", 0)[1][0] == S * S - 22


def test_golden_sample_is_large_enough():
    recs, m0, m1 = MC.golden_sample()
    assert len(recs) >= 40 and len(m0["rows"]) == len(m1["rows"]) == len(recs)
    assert m0["counts"][0].tolist() == [361, 0, 0, -1, 0, 0, 0, 0]                       # a game's first record: the empty board
    assert (m0["counts"][:, 1] > 0).any() and (m0["counts"][:, 7] > 0).any()             # real captures, real forbidden-sound points
