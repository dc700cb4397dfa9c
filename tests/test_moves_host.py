"""CPU: the host side of the move outcomes -- the predicates of moves.Move, the `sgo-moves` lines, the flags of `review --moves`,
the bucket table of `records --moves`, records.RecordSet.moves and GTP's `sgo-moves` -- on hand-written rows, on the fake replay
object with the model behind it (tests/fake_moves_records.py) and on a scripted engine; no GPU.  And the three new symbols: declared,
listed, exported."""
import io
import os
import re

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import moves as mv
from sejonggo_amd.sgfload import SgfGame
from tests import moves_cases as MC
from tests import moves_model as M
from tests.fake_moves_records import MovesRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 5
P = lambda x, y: y * S + x                                                               # noqa: E731
A, O, K, X = mv.ALLOWED, mv.OCCUPIED, mv.KO, mv.SUICIDE
#            flags captured size libs joined weakest ataris atari_stones
QUIET = (A, 0, 1, 4, 0, 0, 0, 0)
CAPTURE = (A, 3, 2, 1, 1, 1, 0, 0)           # takes three and stands on one liberty: a capture, not a self-atari, no escape
SELF_ATARI = (A, 0, 2, 1, 1, 2, 0, 0)
THROW_IN = (A, 0, 1, 1, 0, 0, 1, 4)          # one stone on one liberty that gives atari
ESCAPE = (A, 0, 3, 3, 1, 1, 1, 2)
KO_ROW = (K, 1, 1, 1, 0, 0, 1, 1)            # would capture, but is not allowed: none of the predicates of the counts holds
SUICIDE = (X, 0, 0, 0, 1, 1, 0, 0)
SOUND = (0, 0, 4, 4, 1, 5, 0, 0)
STONE = (O, 0, 0, 0, 0, 0, 0, 0)
ALL = (QUIET, CAPTURE, SELF_ATARI, THROW_IN, ESCAPE, KO_ROW, SUICIDE, SOUND, STONE)


def test_the_same_constants_as_the_header():
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for name, value in (("ALLOWED", A), ("OCCUPIED", O), ("KO", K), ("SUICIDE", X)):
        assert re.search(r"#define SGO_MOVES_%s %d\b" % (name, value), hdr), name
    assert (M.ALLOWED, M.OCCUPIED, M.KO, M.SUICIDE) == (A, O, K, X) == (1, 2, 4, 8)


def test_move_predicates():
    props = ("allowed", "occupied", "ko", "suicide", "captures", "self_atari", "gives_atari", "escapes", "forbidden_sound")
    want = {QUIET: {"allowed"}, CAPTURE: {"allowed", "captures"}, SELF_ATARI: {"allowed", "self_atari"},
            THROW_IN: {"allowed", "self_atari", "gives_atari"}, ESCAPE: {"allowed", "gives_atari", "escapes"}, KO_ROW: {"ko"},
            SUICIDE: {"suicide"}, SOUND: {"forbidden_sound"}, STONE: {"occupied"}}
    for row in ALL:
        m = mv.Move(*row)
        assert {p for p in props if getattr(m, p)} == want[row], row
    # the predicates are those of the counts: the model's counts of a table are the sums of the properties
    rows = np.array(ALL, np.int16)
    v = mv.Moves(3, rows[None], M.counts_of(rows)[None])
    ms = [v.move(0, a) for a in range(9)]
    c = v.counts[0]
    assert [c[0], c[1], c[4], c[5], c[6], c[7]] == [sum(getattr(m, p) for m in ms) for p in
                                                   ("allowed", "captures", "self_atari", "gives_atari", "escapes", "forbidden_sound")]
    assert v.count(0, "max_captured") == 3 and v.count(0, "max_capture_move") == 1 and len(v) == 1
    assert [a for a, _ in v.points(0, "capture")] == [1] and [a for a, _ in v.points(0, "atari")] == [3, 4]
    assert [a for a, _ in v.points(0, "selfatari")] == [2, 3] and [a for a, _ in v.points(0, "escape")] == [4]
    assert [a for a, _ in v.points(0, "forbidden")] == [7] and [a for a, _ in v.points(0, "all")] == list(range(8))


def test_format_move():
    assert mv.format_move(mv.Move(A, 3, 1, 2, 0, 0, 1, 5), "D4") == "D4 captures 3 size 1 liberties 2 joins 0 ataris 1"
    assert mv.format_move(mv.Move(*KO_ROW), "B4") == "B4 captures 1 size 1 liberties 1 joins 0 ataris 1 ko"
    assert mv.format_move(mv.Move(*SUICIDE), "A5") == "A5 captures 0 size 0 liberties 0 joins 1 ataris 0 suicide"
    assert mv.format_move(mv.Move(*SOUND), "A5") == "A5 captures 0 size 4 liberties 4 joins 1 ataris 0 forbidden"


def test_review_flags_on_hand_written_rows():
    name = lambda a: "v%d" % a                                                           # noqa: E731
    quiet_counts, big = [20, 0, 0, -1, 0, 0, 0, 0], [20, 2, 4, 7, 0, 0, 0, 0]
    f = lambda row, counts=quiet_counts, action=3: mv.review_flags(S, action, row, counts, name)   # noqa: E731
    assert f(QUIET) == [] and f(CAPTURE, big) == ["captures 3"] and f(ESCAPE) == ["atari", "escape"]
    assert f(SELF_ATARI) == ["self-atari"]
    assert f(THROW_IN) == ["atari"]                                  # one stone on one liberty: a throw-in is not flagged
    assert f(QUIET, big) == ["missed-capture 4 at v7"] and f(QUIET, [20, 1, 2, 7, 0, 0, 0, 0]) == []      # only from three stones
    assert f(SELF_ATARI, big) == ["self-atari", "missed-capture 4 at v7"]
    assert f(CAPTURE, big, S * S) == [] and f(QUIET, big, S * S) == [] and f(QUIET, big, -1) == []       # a pass gets no flag


def test_bucket_table_arithmetic():
    # five plies in bucket 0 (one a pass), two in bucket 2
    ply = [0, 1, 2, 3, 19, 40, 41]
    actions = [3, 4, S * S, 6, 7, 8, 9]
    played = np.array([CAPTURE, SELF_ATARI, STONE, ESCAPE, QUIET, THROW_IN, QUIET], np.int16)
    counts = np.array([[10, 2, 3, 1, 1, 5, 0, 0], [20, 2, 3, 1, 2, 5, 10, 1], [9, 9, 9, 9, 9, 9, 9, 4], [0, 0, 0, -1, 0, 0, 0, 0],
                       [5, 0, 0, -1, 5, 0, 0, 0], [4, 1, 1, 0, 0, 0, 2, 3], [8, 1, 1, 0, 0, 8, 2, 0]], np.int32)
    t = mv.bucket_table(ply, actions, played, counts, S, 20)
    assert [(r["from"], r["to"], r["plies"], r["passes"]) for r in t] == [(1, 20, 5, 1), (41, 60, 2, 0)]
    a, b = t
    assert a["played"] == {"capture": 0.25, "atari": 0.25, "escape": 0.25, "self_atari": 0.25}
    # the allowed shares: the mean over the three non-pass positions that have an allowed point (the fourth has none)
    assert a["allowed"]["capture"] == pytest.approx((0.2 + 0.1 + 0.0) / 3) and a["allowed"]["self_atari"] == pytest.approx((0.1 + 0.1 + 1.0) / 3)
    assert a["allowed"]["atari"] == pytest.approx((0.5 + 0.25 + 0.0) / 3) and a["allowed"]["escape"] == pytest.approx((0.0 + 0.5 + 0.0) / 3)
    assert (a["forbidden_sound"], a["positions_forbidden"]) == (5, 2)                    # the pass's position counts here too
    assert b["played"] == {"capture": 0.0, "atari": 0.5, "escape": 0.0, "self_atari": 0.5}
    assert b["allowed"]["capture"] == pytest.approx((0.25 + 0.125) / 2) and (b["forbidden_sound"], b["positions_forbidden"]) == (3, 1)
    text = mv.format_bucket_table(t).split("\n")
    assert len(text) == 3 and text[1].split()[:2] == ["1-20", "5"] and text[2].split()[-2:] == ["3", "1"]
    assert mv.bucket_table([], [], np.zeros((0, 8)), np.zeros((0, 8)), S) == []


def test_symbols_declared_listed_and_exported():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.build import build_lib
    build_lib()
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for s in ("sgo_moves_dev", "sgo_moves", "sgo_session_moves"):
        assert re.search(r"\bint %s\s*\(" % s, hdr) and s in L.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None
    assert len(lib.sgo_moves_dev.argtypes) == 9 and len(lib.sgo_moves.argtypes) == 6 and len(lib.sgo_session_moves.argtypes) == 8
    assert "sgo_moves.hip" in __import__("sejonggo_amd.build", fromlist=["SOURCES"]).SOURCES
    assert re.search(r"#define SGO_ABI_VERSION 4\b", hdr)


# ---- the fake replay object: RecordSet.moves, review --moves, records --moves -------------------------------------------------
# the snapback corner of tests/moves_cases.py as set-up stones, then: black plays (4,4) elsewhere, white takes the stone on (0,0)
# with (1,0) (captures 1, five stones on one liberty), black retakes the five with (0,0), white passes, black plays (4,3)
_B, _W = MC.diagram(S, ["X.OX", "OOOX", "XXXX"])
SETUP = [(a, 1) for a in _B] + [(a, -1) for a in _W]
PLAY = [(P(4, 4), 1), (P(1, 0), -1), (P(0, 0), 1), (S * S, -1), (P(4, 3), 1)]


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=MovesRecords(S, 4, 64))


def test_record_set_moves_rows():
    game = _game(SETUP + PLAY, n_setup=len(SETUP))
    rs = _set(game)
    chunks = list(rs.moves())
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "moves"]
    ch = chunks[0]
    n, e = len(game.moves), len(SETUP)
    assert ch.played.shape == (n, 8) and ch.move_counts.shape == (n, 8) and ch.in_turn.shape == (n,)
    # every row is the model's row of the entry's action in the record before it
    recs = rs.backend.last["records"]
    for i in range(n):
        rows, counts = M.record_moves(S, recs[int(ch.index[i])], 0)
        a = int(ch.action[i])
        assert ch.played[i].tolist() == (rows[a].tolist() if a < S * S else [0] * 8) and ch.move_counts[i].tolist() == counts.tolist()
    assert ch.in_turn[e:].all() and not ch.in_turn[1:len(_B)].any()                      # black's set-up stones after the first: out of turn
    # white's capture; black's retake of the five stones is on the point its one stone vanished from: the one-stone ko
    # approximation of the inherited rule names it, snapback or not
    assert ch.played[e + 1].tolist() == [A, 1, 5, 1, 1, 1, 0, 0] and ch.played[e + 2].tolist() == [K, 5, 1, 2, 0, 0, 0, 0]
    assert not ch.played[e + 3].any()                                                    # the pass


def test_review_moves_flags():
    game = _game(SETUP + PLAY, n_setup=len(SETUP))
    found = review.moves_rows(game, _set(game))
    # black's first move leaves four white stones en prise at B5; white's capture is no self-atari; black retakes five
    assert found == {1: ["missed-capture 4 at B5"], 2: ["captures 1"], 3: ["captures 5"], 4: [], 5: []}
    rows = [{"move_number": m, "colour": "B", "played": "A1", "played_share": 0.5, "played_mean": 0.1, "best": "B2", "best_mean": 0.2,
             "top": [{"pv": ["B2", "C3"]}]} for m in (1, 2, 4, 9)]
    plain = [review.format_row(dict(r)) for r in rows]
    review.add_moves(rows, game, record_set=_set(game))
    assert [r["moves_flags"] for r in rows] == [["missed-capture 4 at B5"], ["captures 1"], [], []]
    assert [review.format_row(r) for r in rows] == [plain[0] + "  | missed-capture 4 at B5", plain[1] + "  | captures 1", plain[2], plain[3]]
    rows[1]["tactics"] = ["missed"]
    assert review.format_row(rows[1]) == plain[1] + "  | missed captures 1"             # behind the other units' flags


def test_records_moves_table(tmp_path, monkeypatch):
    L = "abcde"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    text = "(;FF[4]SZ[5]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a in _B), "".join(pt(a) for a in _W)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a) if a < S * S else "[]") for a, c in PLAY) + ")"
    (tmp_path / "snap.sgf").write_text(text)
    monkeypatch.setattr(R, "DeviceRecords", MovesRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "5", "--moves", "--bucket", "2"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert lines[1].startswith("moves ") and [l.split()[:2] for l in lines[2:5]] == [["1-2", "2"], ["3-4", "2"], ["5-6", "1"]]
    assert lines[-1].startswith("moves: forbidden-sound points ")
    rec, _ = R.read_path(str(tmp_path), S)
    t = R.moves_table(R.RecordSet(rec, S, backend=MovesRecords(S, 4, 64)), 2)
    assert [(r["plies"], r["passes"]) for r in t] == [(2, 0), (2, 1), (1, 0)]
    assert t[0]["played"]["capture"] == 0.5 and t[1]["played"]["capture"] == 1.0 and t[2]["played"]["capture"] == 0.0


class MovesEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `move_outcomes` serves the model's row of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, size, case):
        names, recs = MC.case_records(size)
        self.rec, self.size = recs[names.index(case)][None], size

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def move_outcomes(self, side=0):
        m = M.moves(self.size, self.rec, side=side)
        return mv.Moves(self.size, m["rows"], m["counts"])


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_moves(conf5):
    e = gtp.GTPEngine(engine=MovesEngine(S, "two_chains_b"))
    assert e.parse_command("known_command sgo-moves") == "= true\n\n" and "sgo-moves" in e.parse_command("list_commands").split()
    assert e.parse_command("sgo-moves capture") == "= B5 captures 2 size 4 liberties 6 joins 1 ataris 0\nE2 captures 2 size 2 liberties 5 joins 1 ataris 0\n\n"
    assert e.parse_command("sgo_moves capture") == e.parse_command("sgo-moves capture")
    # the opponent's captures: nothing of black's is en prise
    assert e.parse_command("sgo-moves opponent capture") == "=\n\n" == e.parse_command("sgo-moves capture opponent")
    assert len(e.parse_command("sgo-moves").strip("= \n").split("\n")) == len(e.parse_command("sgo-moves all").strip("= \n").split("\n")) == 15
    assert e.parse_command("sgo-moves nonsense") == "? syntax error\n\n" and e.parse_command("sgo-moves capture atari") == "? syntax error\n\n"
    e = gtp.GTPEngine(engine=MovesEngine(S, "forbidden_sound_b"))
    assert e.parse_command("sgo-moves forbidden") == "= A5 captures 0 size 4 liberties 4 joins 1 ataris 0 forbidden\n\n"
    assert e.parse_command("sgo-moves opponent all").split("\n")[0] == "= A5 captures 0 size 0 liberties 0 joins 0 ataris 0 suicide"

    class Host(object):
        """the host engine's surface: no load, no move_outcomes"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-moves") == "? not supported\n\n"
