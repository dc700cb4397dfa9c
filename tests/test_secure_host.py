"""CPU: the host side of the securing moves -- the readers of secure.Secure, the `sgo-secure` text, the flags of `review --secure`,
the bucket table of `records --secure`, records.RecordSet.secure and GTP's `sgo-secure` -- on the model's rows, on the fake replay
object with the model behind it (tests/fake_secure_records.py) and on a scripted engine; no GPU.  And the new symbols: declared,
listed, exported."""
import io
import os
import re

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import secure as sc
from sejonggo_amd.sgfload import SgfGame
from tests import secure_cases as SC
from tests import secure_model as M
from tests.fake_secure_records import SecureRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 5
P = lambda x, y: y * S + x                                                               # noqa: E731
V = lambda a: review.vertex(a, S)                                                        # noqa: E731


def _case(name, side=0):
    """(Secure with one row, stones int8 [N]) of a named 5x5 case, from the model"""
    names, recs = SC.case_records(S)
    rec = recs[names.index(name)]
    m = M.secure(S, rec[None], side=side)
    black, white, _, _ = M.read_record(S, rec, 1 if rec[0] >> 31 else 0)                 # black's stones first, whoever moves
    stones = np.zeros(S * S, np.int8)
    stones[sorted(black)], stones[sorted(white)] = 1, -1
    return sc.Secure(S, m["table"], m["sets"], m["counts"]), stones


def test_the_same_constants_and_counts_as_the_header():
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    assert (M.ALLOWED, M.OCCUPIED, M.KO, M.SUICIDE) == (sc.ALLOWED, sc.OCCUPIED, 4, 8) == (1, 2, 4, 8)
    section = hdr[hdr.index("---- securing moves"):hdr.index("---- influence")]
    for k, name in enumerate(sc.COUNTS):
        assert re.search(r"\* +%d %s\b" % (k, name), section), name
    assert sc.COUNTS == M.COUNTS and sc.MIN_GAIN == 2


def test_secure_readers():
    v, _ = _case("capture_makes_eye_sb")
    assert len(v) == 1 and v.base(0) == 0 and v.best(0) == (1, 10) and v.securing(0) == [(1, 10)] and v.harmful(0) == []
    assert v.gain(0, 1) == 10 and v.gain(0, 0) == 0 and v.gain(0, 2) is None and v.count(0, "allowed") == 17
    assert v.secured(0) == list(range(10)) and v.safe(0) == [] and v.safe(0, after=True) == list(range(10))
    v, _ = _case("capture_opens_eye_sb")
    assert v.base(0) == 21 and v.harmful(0) == [(1, -21)] and v.best(0) == (19, 4) and v.securing(0, 2) == [(19, 4), (23, 4)]
    assert [a for a, _ in v.securing(0)] == [19, 22, 23] and v.gain(0, 15) == -21         # the own eye: harmful, but not ALLOWED
    v, _ = _case("two_eyes_sb")
    assert v.securing(0, 2) == [] and v.harmful(0) == [] and v.gain(0, 0) == -9
    empty = sc.Secure(S, np.zeros((1, S * S, 4), np.int16), np.zeros((1, 4, 1), np.uint32), np.zeros((1, 8), np.int32))
    assert empty.best(0) is None and empty.secured(0) == []


def test_format_board():
    v, stones = _case("capture_opens_eye_sb")
    text = sc.format_board(v, 0, stones, V).split("\n")
    assert text[0].split() == ["X", "-", "O", "X", "X"] and text[3].split() == [".", "X", "X", "X", "4"] and text[4].split() == ["X", "X", ".", "4", "."]
    assert text[5:] == ["base 21 allowed 5 securing 2 harmful 1", "best E2 gain 4 secures E2 C1 D1 E1"]
    loose = sc.format_board(v, 0, stones, V, 1).split("\n")
    assert loose[4].split() == ["X", "X", "1", "4", "."] and loose[5] == "base 21 allowed 5 securing 3 harmful 1"
    v, stones = _case("two_eyes_sb")
    assert sc.format_board(v, 0, stones, V).split("\n")[-1] == "best none"                # the best gain is 1: below the default
    assert sc.format_board(v, 0, stones, V, 1).split("\n")[-1].startswith("best D5 gain 1 secures D5")


def test_review_flags_on_rows():
    counts = np.array([6, 2, 0, 12, 3, 10, 7, 1])                                        # base 8, best 10 at point 7
    flag = lambda a, row: sc.review_flags(S, a, row, counts, V)                          # noqa: E731
    assert flag(7, (1, 12, 6, 0)) == ["secures 10"]
    assert flag(3, (1, 8, 5, 0)) == ["secures 5"] and flag(3, (1, 8, 4, 0)) == ["secures 4", "missed-secure 10 at C4"]
    assert flag(3, (1, 7, 2, 0)) == ["missed-secure 10 at C4"] and flag(3, (1, 7, 0, 0)) == ["missed-secure 10 at C4", "destroys 1"]
    assert flag(S * S, (0, 0, 0, 0)) == ["missed-secure 10 at C4"] and flag(3, (2, 0, 0, 0)) == ["missed-secure 10 at C4"]
    assert flag(3, (0, 0, 0, 0)) == ["missed-secure 10 at C4", "destroys 8"]              # played although not ALLOWED: the literal row
    quiet = np.array([6, 2, 0, 12, 1, 1, 7, 0])
    assert sc.review_flags(S, 3, (1, 7, 2, 0), quiet, V) == [] and sc.review_flags(S, 7, (1, 7, 2, 0), quiet, V) == []
    assert sc.review_flags(S, 3, (1, 7, 2, 0), np.array([6, 2, 0, 0, 0, 0, -1, 0]), V) == []


def test_symbols_declared_listed_and_exported():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.build import build_lib
    build_lib()
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for s in ("sgo_secure_dev", "sgo_secure", "sgo_session_secure", "sgo_secure_mode"):
        assert re.search(r"\bint %s\s*\(" % s, hdr) and s in L.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None
    assert len(lib.sgo_secure_dev.argtypes) == 10 and len(lib.sgo_secure.argtypes) == 7 and len(lib.sgo_session_secure.argtypes) == 9
    assert "sgo_secure.hip" in __import__("sejonggo_amd.build", fromlist=["SOURCES"]).SOURCES
    assert re.search(r"#define SGO_ABI_VERSION 4\b", hdr)


# ---- the fake replay object: RecordSet.secure, review --secure, records --secure ------------------------------------------------
# capture_makes_eye as set-up stones, then: black plays elsewhere (the securing capture is missed), white passes, black captures
# (two eyes: ten points proved), white plays elsewhere, black fills his own corner eye (not ALLOWED, played as recorded), white passes
_B, _W = SC.diagram(S, ["..OOX", "XXXXX"])
SETUP = [(a, 1) for a in _B] + [(a, -1) for a in _W]
PLAY = [(P(4, 4), 1), (S * S, -1), (P(1, 0), 1), (P(0, 4), -1), (P(0, 0), 1), (S * S, -1)]


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=SecureRecords(S, 4, 64))


def test_record_set_secure_rows():
    game = _game(SETUP + PLAY, n_setup=len(SETUP))
    rs = _set(game)
    chunks = list(rs.secure())
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "secure"]
    ch = chunks[0]
    n = len(game.moves)
    assert ch.secure.table.shape == (n + 1, S * S, 4) and ch.secure.counts.shape == (n + 1, 8) and ch.to_play.shape == (n + 1,)
    recs = rs.backend.last["records"]
    for r in range(n + 1):                                           # every record of the game: the model's row
        table, sets, counts = M.record_secure(S, recs[r], 0)
        assert np.array_equal(ch.secure.table[r], table) and np.array_equal(ch.secure.sets[r], sets) and np.array_equal(ch.secure.counts[r], counts)
    e = len(SETUP)
    assert ch.to_play[e:].tolist() == [1, -1, 1, -1, 1, -1, 1] and ch.secure.best(e) == (1, 10)
    assert ch.secure.base(e + 4) == 10 and ch.secure.base(e + 3) == 0                   # black's ten points; white to move: white's none


def test_review_secure_flags():
    game = _game(SETUP + PLAY, n_setup=len(SETUP))
    found = review.secure_rows(game, _set(game))
    assert found == {1: ["missed-secure 10 at B5"], 2: [], 3: ["secures 10"], 4: [], 5: ["destroys 10"], 6: []}
    rows = [{"move_number": m, "colour": "B", "played": "A1", "played_share": 0.5, "played_mean": 0.1, "best": "B2", "best_mean": 0.2,
             "top": [{"pv": ["B2", "C3"]}]} for m in (1, 3, 4, 9)]
    plain = [review.format_row(dict(r)) for r in rows]
    review.add_secure(rows, game, record_set=_set(game))
    assert [r["secure_flags"] for r in rows] == [["missed-secure 10 at B5"], ["secures 10"], [], []]
    assert [review.format_row(r) for r in rows] == [plain[0] + "  | missed-secure 10 at B5", plain[1] + "  | secures 10", plain[2], plain[3]]
    rows[1]["moves_flags"] = ["captures 2"]
    assert review.format_row(rows[1]) == plain[1] + "  | captures 2 secures 10"           # behind the other units' flags
    # a move out of turn gets no flag: black twice in a row
    twice = _game(SETUP + [(P(4, 4), 1), (P(1, 0), 1)], n_setup=len(SETUP))
    assert review.secure_rows(twice, _set(twice)) == {1: ["missed-secure 10 at B5"], 2: []}


def test_review_secure_loads_no_net(tmp_path, monkeypatch):
    """review.main --secure alone: the rows of a review without a search, the flags behind them, and neither a net nor an engine"""
    L = "abcde"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    text = "(;FF[4]SZ[5]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a in _B), "".join(pt(a) for a in _W)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a) if a < S * S else "[]") for a, c in PLAY) + ")"
    (tmp_path / "eye.sgf").write_text(text)
    monkeypatch.setattr(R, "DeviceRecords", SecureRecords)
    monkeypatch.setattr(review, "_net", lambda *a: (_ for _ in ()).throw(AssertionError("no net is loaded")))
    out = io.StringIO()
    assert review.main([str(tmp_path / "eye.sgf"), "--secure"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == 6 and lines[0].endswith("  | missed-secure 10 at B5") and lines[2].endswith("  | secures 10")
    assert lines[4].endswith("  | destroys 10") and "|" not in lines[1] + lines[3] + lines[5]


def test_records_secure_table(tmp_path, monkeypatch):
    L = "abcde"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    text = "(;FF[4]SZ[5]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a in _B), "".join(pt(a) for a in _W)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a) if a < S * S else "[]") for a, c in PLAY) + ")"
    (tmp_path / "eye.sgf").write_text(text)
    monkeypatch.setattr(R, "DeviceRecords", SecureRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "5", "--secure", "--bucket", "2"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert lines[1].startswith("moves ") and [l.split() for l in lines[2:5]] == [["1-2", "2", "0", "1", "0", "0", "0"], ["3-4", "2", "0", "1", "1", "1", "0"],
                                                                                  ["5-6", "2", "1", "0", "0", "0", "1"]]
    assert lines[5] == "secure: 2 of 6 positions offer a securing move; the recorded move took the best 1 times, any 1 times; harmful moves played 1"
    rec, _ = R.read_path(str(tmp_path), S)
    t = R.secure_table(R.RecordSet(rec, S, backend=SecureRecords(S, 4, 64)), 20)
    assert t == [{"from": 1, "to": 20, "plies": 6, "proved": 1, "offered": 2, "took_best": 1, "took_any": 1, "harmful_played": 1}]
    assert sc.bucket_table([], [], np.zeros((0, 4)), np.zeros((0, 8)), S) == []


class SecureEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `secure` serves the model's row of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, case):
        self.case = case

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def secure(self, side=0):
        return _case(self.case, side)


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_secure(conf5):
    e = gtp.GTPEngine(engine=SecureEngine("capture_opens_eye_sb"))
    assert e.parse_command("known_command sgo-secure") == "= true\n\n" and "sgo-secure" in e.parse_command("list_commands").split()
    v, stones = _case("capture_opens_eye_sb")
    assert e.parse_command("sgo-secure") == "= " + sc.format_board(v, 0, stones, V) + "\n\n" == e.parse_command("sgo_secure")
    assert e.parse_command("sgo-secure").endswith("base 21 allowed 5 securing 2 harmful 1\nbest E2 gain 4 secures E2 C1 D1 E1\n\n")
    assert e.parse_command("sgo-secure min 1") == "= " + sc.format_board(v, 0, stones, V, 1) + "\n\n"
    w, _ = _case("capture_opens_eye_sb", 1)
    assert e.parse_command("sgo-secure opponent") == "= " + sc.format_board(w, 0, stones, V) + "\n\n" == e.parse_command("sgo-secure min 2 opponent")
    assert w.base(0) == 0 and e.parse_command("sgo-secure opponent").endswith("best none\n\n")
    for bad in ("sgo-secure nonsense", "sgo-secure min", "sgo-secure min x", "sgo-secure opponent opponent", "sgo-secure min 1 min 2"):
        assert e.parse_command(bad) == "? syntax error\n\n", bad

    class Host(object):
        """the host engine's surface: no load, no secure"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-secure") == "? not supported\n\n"
