"""No GPU: the SGF reader (sgfload), the GTP commands undo / loadsgf / known_command / sgo-analyze on a scripted engine, and the
review tool's table and JSON document from a scripted SessionEngine."""
import json
import os

import numpy as np
import pytest

from sejonggo_amd import gtp, review, sgfload

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = os.path.join(GOLDEN, "review_S19.sgf")


# ---------------------------------------------------------------------------------------------- sgfload
def test_passes_both_ways_and_the_engine_style_pass():
    g = sgfload.loads("(;FF[4]SZ[9]KM[5.5];B[ee];W[];B[tt];W[aj])")
    assert (g.size, g.komi) == (9, 5.5)
    assert g.moves == [(4 * 9 + 4, 1), (81, -1), (81, 1), (81, -1)] and g.setup == [False] * 4 and g.n_moves == 4
    # on a board larger than 19x19 "tt" is a point
    assert sgfload.loads("(;SZ[21];B[tt])").moves == [(19 * 21 + 19, 1)]


def test_setup_stones_and_compressed_points():
    g = sgfload.loads("(;SZ[5]AB[aa][cc:dd]AW[ee];W[bb])")
    assert g.moves == [(0, 1), (12, 1), (13, 1), (17, 1), (18, 1), (24, -1), (6, -1)]
    assert g.setup == [True] * 6 + [False] and g.komi is None
    assert g.prefix(0) == g.moves[:6] and g.prefix(1) == g.moves and g.prefix(9) == g.moves


def test_variations_are_ignored():
    text = "(;SZ[5];B[aa](;W[bb](;B[cc])(;B[dd];W[ee]))(;W[ab];B[ba]))(;SZ[5];B[ee])"
    assert sgfload.loads(text).moves == [(0, 1), (6, -1), (12, 1)]


def test_escaped_bracket_and_line_break_in_a_comment():
    g = sgfload.loads("(;SZ[5]C[a \\] ;B[zz\\] ( \\\\]GN[x\\\ny];B[ab]C[(;W[aa\\])])")
    assert g.moves == [(5, 1)]


@pytest.mark.parametrize("text", ["(;SZ[9:13];B[aa])", "(;SZ[x];B[aa])", "(;SZ[40];B[aa])", "(;SZ[5];B[ff])", "(;SZ[5];B[a])",
                                  "(;SZ[5]KM[half];B[aa])", "(;SZ[5];B[aa", "no game here", "(;SZ[5];B)"])
def test_malformed_records_are_refused(text):
    with pytest.raises(ValueError):
        sgfload.loads(text)


def test_the_committed_record():
    g = sgfload.load_file(RECORD)
    assert (g.size, g.komi, g.n_moves) == (19, 6.5, 310) and not any(g.setup)
    assert [c for _, c in g.moves[:4]] == [1, -1, 1, -1]
    assert g.moves[-1][0] == 361 and all(0 <= a <= 361 for a, _ in g.moves)
    # the record is game 3 of the reference's five, whose plies tests/golden/sgf_S19.npz holds
    from tests.helpers import load
    mv = load("sgf_S19.npz")["g03_moves"]
    assert [a for a, _ in g.moves[:len(mv)]] == [361 if y >= 19 else int(y) * 19 + int(x) for x, y, _ in mv]


# ---------------------------------------------------------------------------------------------- GTP on a scripted engine
class _Net(object):
    name = "scripted"


class ScriptedEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: it keeps the move list and a trace."""

    def __init__(self, size):
        self.size, self.moves, self.trace, self.model = size, [], [], _Net()
        self.board, self.player, self.move, self.mcts_tree = _empty_board(size)[0], 1, 1, None

    def play(self, color, x, y, update_tree=True):
        self.moves.append((y * self.size + x if y < self.size else self.size * self.size, color))
        self.trace.append(("play", color, x, y))
        return self.board, color

    def load(self, moves, colors=None, n_setup=0):
        self.n_setup = n_setup
        if any(a == 7 for a in moves):
            raise ValueError("move list refused at index %d: -101" % list(moves).index(7))
        self.moves = list(zip(moves, colors))
        self.trace.append(("load", list(moves), list(colors)))
        return self.board, -1

    def undo(self):
        if not self.moves:
            raise ValueError("cannot undo")
        self.moves.pop()
        self.trace.append(("undo",))
        return self.board, 1

    def analyze(self, sims=None):
        self.trace.append(("analyze", sims))
        return None, 0.0

    def report(self, top=5, depth=8):
        A = self.size * self.size + 1
        N, Q, P = np.full((1, A), -1, np.int32), np.zeros((1, A), np.float32), np.zeros((1, A), np.float32)
        N[0, [12, 7, A - 1]], Q[0, [12, 7, A - 1]], P[0, [12, 7, A - 1]] = [9, 3, 0], [0.25, -0.5, 0], [0.5, 0.25, 0.125]
        ta, pv = np.full((1, top), -1, np.int32), np.full((1, top, depth), -1, np.int32)
        ta[0, :3] = [12, 7, A - 1]
        pv[0, 0, :3], pv[0, 1, :1], pv[0, 2, :1] = [12, 6, A - 1], [7], [A - 1]
        return {"N": N, "Q": Q, "P": P, "top_action": ta, "pv": pv}


def _empty_board(size):
    """play.game_init's result; the real one runs the rules library on the device"""
    board = np.zeros((1, size, size, 17), dtype=np.int32)
    board[..., -1] = 1
    return board, 1


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    keep = dict(conf)
    conf.update({'SIZE': 5, 'MCTS_SIMULATIONS': 16, 'ENERGY': 4})
    monkeypatch.setattr(gtp, "game_init", _empty_board)          # GTPEngine.__init__ starts from game_init's board
    yield conf
    conf.clear()
    conf.update(keep)


def test_gtp_undo_known_command_and_analysis_text(conf5):
    eng = ScriptedEngine(5)
    e = gtp.GTPEngine(engine=eng)
    assert e.parse_command("known_command undo") == "= true\n\n" and e.parse_command("known_command sgo-analyze") == "= true\n\n"
    assert e.parse_command("known_command sgo_analyze") == "= true\n\n"     # parse_command accepts the method name, too
    assert e.parse_command("known_command frobnicate") == "= false\n\n" and e.parse_command("known_command") == "= false\n\n"
    for name in ("undo", "loadsgf", "known_command", "sgo-analyze", "genmove", "quit"):
        assert name in e.parse_command("list_commands").split()
    assert e.parse_command("undo") == "? cannot undo\n\n"
    assert e.parse_command("play B C3") == "=\n\n" and e.parse_command("undo") == "=\n\n" and eng.moves == []
    assert e.parse_command("sgo-analyze 32") == ("= C3 visits 9 mean 0.2500 prior 0.5000 pv C3 B4 pass\n"
                                                  "C4 visits 3 mean -0.5000 prior 0.2500 pv C4\n"
                                                  "pass visits 0 mean 0.0000 prior 0.1250 pv pass\n\n")
    assert e.parse_command("sgo-analyze") == e.parse_command("sgo_analyze")
    assert eng.trace[-3:] == [("analyze", 32), ("analyze", None), ("analyze", None)]
    assert e.parse_command("sgo-analyze many") == "? syntax error\n\n"
    assert e.parse_command("_vertex 3") == "? unknown command\n\n"


def test_gtp_loadsgf(conf5, tmp_path):
    eng = ScriptedEngine(5)
    e = gtp.GTPEngine(engine=eng)
    f = tmp_path / "g.sgf"
    f.write_text("(;SZ[5]KM[2.5]AB[aa];W[bb];B[cc];W[];B[dd])")
    assert e.parse_command("loadsgf %s" % f) == "=\n\n"
    assert eng.trace[-1] == ("load", [0, 6, 12, 25, 18], [1, -1, 1, -1, 1]) and e._komi == 2.5
    assert e.parse_command("loadsgf %s 3" % f) == "=\n\n"                  # the position before move 3: set-up + two moves
    assert eng.trace[-1] == ("load", [0, 6, 12], [1, -1, 1])
    assert e.parse_command("loadsgf %s 1" % f) == "=\n\n" and eng.trace[-1] == ("load", [0], [1])
    assert eng.n_setup == 1                                                # the AB stone is no move: undo stops in front of it
    n = len(eng.trace)
    assert e.parse_command("loadsgf %s" % (tmp_path / "missing.sgf")).startswith("? cannot load file")
    f.write_text("(;SZ[9];B[aa])")
    assert e.parse_command("loadsgf %s" % f).startswith("? cannot load file: the record is 9x9")
    f.write_text("(;SZ[5];B[cb];W[aa])")                                   # action 7 is what the scripted engine refuses
    assert e.parse_command("loadsgf %s" % f).startswith("? cannot load file: move list refused at index 0")
    f.write_text("(;SZ[5];B[zz])")
    assert e.parse_command("loadsgf %s" % f).startswith("? cannot load file: SGF")
    assert len(eng.trace) == n


def test_gtp_on_the_host_engine_answers_not_supported(conf5):
    class Host(object):                      # gtp.SejongGoEngine's surface: it has analyze, but neither load nor report
        model = _Net()

        def analyze(self, sims=None):
            raise AssertionError("not reached")
    e = gtp.GTPEngine(engine=Host())
    for cmd in ("undo", "loadsgf x.sgf", "sgo-analyze", "sgo-analyze 8"):
        assert e.parse_command(cmd) == "? not supported\n\n", cmd
    assert e.parse_command("known_command undo") == "= true\n\n"


# ---------------------------------------------------------------------------------------------- review from a scripted engine
class ScriptedSessions(object):
    """engine.SessionEngine's surface as review() drives it: G slots; the 'search' of a position is a fixed function of its
    move list, so the expected table can be written down."""

    def __init__(self, size, G):
        self.S, self.G, self.A = size, G, size * size + 1
        self.calls, self.lists = [], {}
        self.raise_on_error, self.fail_slot = True, None

    def open(self, slots, resign=None):
        self.calls.append(("open", len(slots)))

    def setup(self, slots, move_lists, color_lists=None):
        self.calls.append(("setup", len(slots)))
        status = np.zeros(len(slots), np.int32)
        for s, m, c in zip(slots, move_lists, color_lists):
            self.lists[int(s)] = (list(m), list(c))
            status[list(slots).index(s)] = -101 if len(m) == 4 else 0
        return status, np.where(status != 0, 3, -1).astype(np.int32)

    def analyze(self, slots, sims=None):
        self.calls.append(("analyze", len(slots), sims))
        self.raise_seen = self.raise_on_error
        if self.fail_slot in [int(s) for s in slots]:
            from sejonggo_amd._lib import SgoError
            raise SgoError("genmove: slots [%d] recorded no move" % self.fail_slot)

    def results(self, slots):
        return np.array([(-201,)] * len(slots), dtype=[("done", "<i4")])

    def report(self, slots, top=5, depth=8):
        self.calls.append(("report", len(slots)))
        n, A = len(slots), self.A
        r = {"status": np.zeros(n, np.int32), "to_play": np.zeros(n, np.int32), "root_count": np.full(n, 10, np.int32),
             "root_value": np.full(n, 0.5, np.float32), "root_mean": np.zeros(n, np.float32), "n_children": np.zeros(n, np.int32),
             "N": np.full((n, A), -1, np.int32), "Q": np.zeros((n, A), np.float32), "P": np.zeros((n, A), np.float32),
             "top_action": np.full((n, top), -1, np.int32), "pv": np.full((n, top, depth), -1, np.int32)}
        for i, s in enumerate(slots):
            k = len(self.lists[int(s)][0])
            r["to_play"][i] = 1 if k % 2 == 0 else -1
            if int(s) == self.fail_slot:
                r["status"][i] = -203
            best, other = (k + 1) % (A - 1), (k + 7) % (A - 1)
            r["N"][i, :] = 0
            r["N"][i, [best, other]], r["Q"][i, [best, other]], r["P"][i, [best, other]] = [6, 4], [0.5, -0.25], [0.75, 0.25]
            r["top_action"][i, :2] = [best, other][:top]
            r["pv"][i, 0, :2] = [best, A - 1]
            if top > 1:
                r["pv"][i, 1, :1] = [other]
        return r


def test_review_table_and_json(tmp_path):
    # moves 1..6 of a 5x5 record: move m is played at point m - 1... except where the scripted best move is met
    text = "(;SZ[5]KM[0.5];B[ba];W[ab];B[da];W[ea];B[bb];W[ca])"
    game = sgfload.loads(text)
    eng = ScriptedSessions(5, 4)
    rows = review.review(eng, game, sims=12, every=1, top=2, depth=4)
    assert eng.calls == [("open", 4), ("setup", 4), ("analyze", 4, 12), ("report", 4), ("setup", 2), ("analyze", 1, 12), ("report", 2)]
    assert [r["move_number"] for r in rows] == [1, 2, 3, 4, 5, 6] and [r["colour"] for r in rows] == list("BWBWBW")
    first = rows[0]                 # the empty board: best = point 1 = B5 = the move played, other = point 7
    assert first["played"] == "B5" and first["best"] == "B5" and first["played_visits"] == 6 and first["visits"] == 10
    assert first["played_share"] == 0.6 and first["played_mean"] == 0.5 and first["root_value"] == 0.5
    assert first["top"] == [{"move": "B5", "visits": 6, "mean": 0.5, "prior": 0.75, "pv": ["B5", "pass"]},
                            {"move": "C4", "visits": 4, "mean": -0.25, "prior": 0.25, "pv": ["C4"]}]
    assert rows[1]["played"] == "A4" and rows[1]["played_visits"] == 0 and rows[1]["best"] == "C5"
    assert rows[4] == {"move_number": 5, "colour": "B", "played": "B4", "error": -101, "fail_at": 3}
    lines = [review.format_row(r) for r in rows]
    assert lines[0] == "   1 B B5   share  60.0% mean +0.5000  best B5   mean +0.5000  pv B5 pass"
    assert lines[4] == "   5 B B4    set-up refused (-101 at entry 3)"
    doc = json.loads(json.dumps(review.document(game, rows, 12, 4, "scripted")))
    assert doc["positions"] == rows and (doc["size"], doc["komi"], doc["moves"], doc["sims"]) == (5, 0.5, 6, 12)
    # every = 4: the positions before moves 1 and 5
    eng = ScriptedSessions(5, 4)
    assert [r["move_number"] for r in review.review(eng, game, every=4, top=1, depth=2)] == [1, 5]
    assert review.vertex(8 * 19 + 8, 19) == "J11" and review.vertex(361, 19) == "pass"


def test_review_reports_a_failed_search_as_a_row():
    game = sgfload.loads("(;SZ[5];B[ba];W[ab];B[da])")
    eng = ScriptedSessions(5, 4)
    eng.fail_slot = 1
    rows = review.review(eng, game, sims=12, top=2, depth=4)
    assert eng.raise_seen is False and eng.raise_on_error is True         # the engine's steps did not raise meanwhile
    assert rows[1] == {"move_number": 2, "colour": "W", "played": "A4", "error": -201, "fail_at": -1}
    assert "error" not in rows[0] and "error" not in rows[2]
    assert review.format_row(rows[1]) == "   2 W A4    search failed (-201)"
    assert eng.calls[-1] == ("open", 1)                                  # the failed slot is a session again


def test_review_refuses_another_board_size():
    with pytest.raises(ValueError):
        review.review(ScriptedSessions(9, 2), sgfload.loads("(;SZ[5];B[aa])"))
