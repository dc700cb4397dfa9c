"""No GPU: the policy rollouts' pinned arithmetic (include/sgo.h "policy rollouts") on the CPU model tests/rollout_model.py, the
rule-determined fixtures through that model, the thresholds and the final_score text of sejonggo_amd/rollout.py on hand-made
counts, and the GTP commands final_score / final_status_list / sgo-ownership on a scripted engine."""
import numpy as np
import pytest

from oracle import oracle
from sejonggo_amd import gtp, rollout, stub_nets
from tests import rollout_model as M
from tests.test_session_review_host import ScriptedEngine, _empty_board


# ---------------------------------------------------------------------------------------------- pinned arithmetic
def test_draws():
    assert M.draw(3, 0, 0) == 0x6785fa52 and M.draw(3, 1, 0) == 0x23064794 and M.draw(3, 0, 1) == 0x9c16bc0b
    assert M.draw(0xDEADBEEF, 4095, 721) == 0x602b1d15 and M.draw(0, 0, 0) == 0


def test_weights():
    p = np.array([0, -0.0, 1e-45, 2.0 ** -20, 1.5 * 2.0 ** -20, 0.5, 1, 2, np.nan, -1, np.inf], dtype=np.float32)
    assert M.weights(p) == [1, 1, 1, 2, 2, 524289, 1048577, 1048577, 1, 1, 1048577]


def test_picks():
    w = [0, 5, 0, 3, 8]
    assert [M.pick(w, r) for r in (0, 0x4FFFFFFF, 0x50000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)] == [1, 1, 3, 3, 4, 4]


@pytest.mark.parametrize("kind, plies, areas, capped", [
    ("table", [41, 24, 28, 20, 33, 26, 25, 37], [(25, 0), (9, 12), (14, 7), (12, 10), (22, 1), (12, 11), (14, 7), (21, 1)], []),
    ("hash", [23, 30, 27, 50, 33, 29, 28, 19], None, [3])])
def test_guard_vector(kind, plies, areas, capped):
    """S = 5, the empty board, seed 3, sym_k 0, max_plies 50, g = 0..7."""
    board, _ = oracle.game_init(5)
    r = M.run(stub_nets.make_stub(kind, 5), board, 8, 3, 0, 50)
    assert [row[0] for row in r["rows"]] == plies
    assert [g for g, row in enumerate(r["rows"]) if row[3]] == capped
    if areas is not None:
        assert [row[1:3] for row in r["rows"]] == areas
    s = r["sums"][0]
    assert s[0] + s[1] + s[2] == s[7] == 8 and s[5] == sum(plies) and s[6] == len(capped)
    assert s[3] == sum(b - w for _, b, w, _ in r["rows"]) and s[4] == sum((b - w) ** 2 for _, b, w, _ in r["rows"])


def test_pack_boards_is_the_inverse_of_unpack_positions():
    from sejonggo_amd.engine import unpack_positions
    board, _ = oracle.game_init(5)
    for a in (12, 7, 25, 3, 8):
        oracle.make_play(a % 5 if a < 25 else 0, a // 5 if a < 25 else 5, board)
    boards = np.concatenate([board, M.board_of(5, *M.fixture_f2(), to_play=-1)])
    assert np.array_equal(unpack_positions(M.pack_boards(boards), 5), boards)


# ---------------------------------------------------------------------------------------------- rule-determined fixtures
def test_fixture_f1_through_the_model():
    """Neither side has a legal board move: every rollout is two passes, every point keeps its owner."""
    black, white = M.fixture_f1()
    assert len(black) == 13 and len(white) == 8
    for to_play in (1, -1):
        board = M.board_of(5, black, white, to_play)
        assert oracle.legal_moves(board)[:25].all()                   # the reference's mask flags the ILLEGAL points
        r = M.run(stub_nets.TableNet(5), board, 4, 11)
        assert [row[0] for row in r["rows"]] == [2] * 4
        cols = np.arange(25) % 5
        assert np.array_equal(r["black_own"][0], np.where(cols < 3, 4, 0)) and np.array_equal(r["white_own"][0], np.where(cols >= 3, 4, 0))
        row = {"black_own": r["black_own"][0], "white_own": r["white_own"][0], "rollouts": 4}
        assert rollout.final_score(row, 0) == "B+5.0"


@pytest.mark.parametrize("to_play, plies", [(1, 3), (-1, 4)])
def test_fixture_f2_through_the_model(to_play, plies):
    """The white stone on (0,0) is captured in every rollout, whoever moves first."""
    black, white = M.fixture_f2()
    board = M.board_of(5, black, white, to_play)
    r = M.run(stub_nets.HashNet(5), board, 4, 5)
    assert [row[0] for row in r["rows"]] == [plies] * 4 and r["black_own"][0][0] == 4
    row = {"black_own": r["black_own"][0], "white_own": r["white_own"][0], "rollouts": 4}
    st = rollout.stone_status(row, oracle.get_real_board(board))
    assert st["dead"] == {0} and st["seki"] == set() and st["alive"] == set(black) | (set(white) - {0})
    assert rollout.final_score(row, 0) == "B+5.0"


# ---------------------------------------------------------------------------------------------- thresholds and text
def _row(black_own, white_own, R):
    return {"black_own": np.array(black_own, np.int32), "white_own": np.array(white_own, np.int32), "rollouts": R}


def test_thresholds_at_the_exact_boundary():
    # R = 9: 3 * 6 == 2 * 9 settles a point, 5 does not; R = 10: 7 settles (21 >= 20), 6 does not (18 < 20)
    assert list(rollout.point_owner(_row([6, 5, 0, 3], [3, 4, 6, 5], 9))) == [1, 0, -1, 0]
    assert list(rollout.point_owner(_row([7, 6, 3, 0], [3, 4, 7, 6], 10))) == [1, 0, -1, 0]
    assert list(rollout.point_owner(_row([0, 0], [0, 0], 0))) == [0, 0]
    st = rollout.stone_status(_row([6, 5, 0, 3], [3, 4, 6, 5], 9), [1, -1, 1, 0])
    assert st == {"alive": {0}, "seki": {1}, "dead": {2}}


def test_final_score_text():
    row = _row([9, 9, 9, 0, 0, 4], [0, 0, 0, 9, 9, 4], 9)             # black 3 points, white 2, one unsettled
    assert rollout.final_score(row, 0) == "B+1.0" and rollout.final_score(row, 1) == "0" and rollout.final_score(row, 1.0) == "0"
    assert rollout.final_score(row, 0.5) == "B+0.5" and rollout.final_score(row, 6.5) == "W+5.5" and rollout.final_score(row, "7.5") == "W+6.5"
    assert rollout.score_lead(row, 0.5) == 0.5
    row = _row([9, 0], [0, 9], 9)
    assert rollout.final_score(row, 0) == "0"                          # a draw on the board


def test_result_row_and_real_board():
    res = {"black_own": np.arange(8).reshape(2, 4), "white_own": np.arange(8).reshape(2, 4)[::-1]}
    for j, name in enumerate(rollout.SUMS):
        res[name] = np.array([j, 10 + j], np.int64)
    row = rollout.result_row(res, 1)
    assert list(row["black_own"]) == [4, 5, 6, 7] and list(row["white_own"]) == [0, 1, 2, 3] and row["rollouts"] == 17 and row["capped"] == 16
    board = M.board_of(5, [3], [7], to_play=-1)
    assert np.array_equal(rollout.real_board(board), oracle.get_real_board(board))


# ---------------------------------------------------------------------------------------------- GTP on a scripted engine
class RolloutScripted(ScriptedEngine):
    """ScriptedEngine plus the `rollouts` of gtp.DeviceSejongGoEngine: F2's counts from the model."""

    def rollouts(self, per_src=None, seed=0):
        self.trace.append(("rollouts", per_src, seed))
        black, white = M.fixture_f2()
        board = M.board_of(5, black, white, 1)
        r = M.run(stub_nets.HashNet(5), board, 4, 5)
        row = {"black_own": r["black_own"][0], "white_own": r["white_own"][0]}
        for j, name in enumerate(rollout.SUMS):
            row[name] = int(r["sums"][0][j])
        return row, oracle.get_real_board(board)


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    keep = dict(conf)
    conf.update({'SIZE': 5, 'MCTS_SIMULATIONS': 16, 'ENERGY': 4})
    monkeypatch.setattr(gtp, "game_init", _empty_board)
    yield conf
    conf.clear()
    conf.update(keep)


def test_gtp_final_commands(conf5):
    assert conf5['ROLLOUTS'] == 64
    e = gtp.GTPEngine(engine=RolloutScripted(5))
    for name in ("final_score", "final_status_list", "sgo-ownership"):
        assert name in e.parse_command("list_commands").split() and e.parse_command("known_command " + name) == "= true\n\n"
    assert e.parse_command("final_score") == "= B+5.0\n\n"
    assert e.parse_command("komi 5.5") == "=\n\n" and e.parse_command("final_score") == "= W+0.5\n\n"     # komi arrives as text
    assert e.parse_command("final_status_list dead") == "= A5\n\n"
    assert e.parse_command("final_status_list seki") == "=\n\n"
    alive = e.parse_command("final_status_list alive")[2:].split()
    assert len(alive) == 12 + 8 and "A5" not in alive and "B5" in alive and "D5" in alive
    assert e.parse_command("final_status_list") == "? syntax error\n\n" and e.parse_command("final_status_list lost") == "? syntax error\n\n"
    own = e.parse_command("sgo-ownership")
    assert own == e.parse_command("sgo_ownership")
    lines = own[2:].rstrip("\n").split("\n")
    assert len(lines) == 5 and all(l.split() == ["1000", "1000", "1000", "-1000", "-1000"] for l in lines)


def test_gtp_final_commands_need_the_device_engine(conf5):
    class Host(object):
        """the host engine's surface: no load, no rollouts"""
        model = type("N", (), {"name": "x"})()

    e = gtp.GTPEngine(engine=Host())
    for cmd in ("final_score", "final_status_list dead", "sgo-ownership"):
        assert e.parse_command(cmd) == "? not supported\n\n"
