"""CPU: the host side of the capturing-race reader -- the argument checks, the racer words and the pair's outcome of race.py, the
`sgo-race` text, the flags of `review --race`, the bucket table of `records --race`, records.RecordSet.race and GTP's `sgo-race` -- on
the model's rows, on the fake replay object with the model behind it (tests/fake_race_records.py) and on a scripted engine; no GPU.
And the new symbols: declared, listed, exported."""
import io
import os
import re

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import race as rc
from sejonggo_amd.sgfload import SgfGame
from tests import race_model as M
from tests.fake_race_records import RaceRecords
from tests.tactics_cases import diagram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 7
N = S * S
P = lambda x, y: y * S + x                                                               # noqa: E731
V = lambda a: review.vertex(a, S)                                                        # noqa: E731

# the plain two-against-two race at 7x7: C7 (black) against E7 (white), first to move wins at G7 (black) / B7 (white)
_B, _W = diagram(S, ["O.XXOO.", "O.XXOO.", "OOOOXXX"])
PLAIN = "C7 E7 libs 2 2 shared 0 empty 4 first to move wins black catch B7 save G7 white catch G7 save B7 nodes 6 12 17 4"


def _race(ask=None, rules=1, max_libs=4, max_nodes=1024, white_to_play=False):
    """Race with one row of the plain position, from the model"""
    rec = M.build_record(S, _B, _W, white_to_play)
    m = M.race(S, rec[None], ask=None if ask is None else [ask], rules=rules, max_libs=max_libs, max_nodes=max_nodes)
    T = max(1, len(m["rows"][0]))
    rows, regions = np.zeros((1, T, 16), np.int32), np.zeros((1, T, 2), np.uint32)
    rows[0, :len(m["rows"][0])], regions[0, :len(m["rows"][0])] = m["rows"][0], m["regions"][0]
    return rc.Race(S, m["n_pairs"], rows, regions)


def test_the_same_constants_as_the_header():
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for name, val in (("A_CAUGHT", 1), ("D_CAUGHT", 2), ("A_UNKNOWN", 4), ("D_UNKNOWN", 8), ("D_RAN", 16), ("WHITE_SHIFT", 8), ("MAX_LIBS", 8),
                      ("MAX_REGION", 32), ("MAX_NODES", 32768), ("MAX_PAIRS", 64)):
        assert re.search(r"#define SGO_RACE_%s %d\b" % (name, val), hdr), name
        assert getattr(rc, name) == val == getattr(M, name), name
    assert re.search(r"#define SGO_RACE_OPEN \(1 << 16\)", hdr) and re.search(r"#define SGO_RACE_NO_PAIR \(1 << 17\)", hdr)
    assert rc.OPEN == M.OPEN == 1 << 16 and rc.NO_PAIR == M.NO_PAIR == 1 << 17
    assert re.search(r"#define SGO_RACE_MAX_DEPTH 80\b", hdr) and M.MAX_DEPTH == 80


def _pair(status, **kw):
    f = dict(anchor_b=2, anchor_w=4, libs_b=2, libs_w=2, shared=0, region_empty=4, status=status, reserved=0, catch_b=1, save_b=6, catch_w=6,
             save_w=1, nodes_ab=6, nodes_db=12, nodes_aw=17, nodes_dw=4)
    f.update(kw)
    return rc.Pair(**f)


def test_racer_words_and_outcomes():
    v = rc.verdict_of
    assert v(0) == "safe" and v(17) == "unsettled" and v(19) == "caught" and v(4) == "unknown" and v(25) == "unknown"
    assert rc.VERDICTS == ("safe", "unsettled", "caught", "unknown")
    for st in (0, 17, 19, 4, 17 | 19 << 8, 4 << 8, 19 | 17 << 8):
        p = _pair(st)
        assert (p.black, p.white) == M.verdicts([0] * 6 + [st]) and not p.open and not p.no_pair
    assert _pair(19 << 8).outcome == "black wins" and _pair(19).outcome == "white wins" and _pair(17 | 17 << 8).outcome == "first to move wins"
    assert _pair(0).outcome == "standoff" and _pair(17).outcome == "black unsettled, white safe" and _pair(4 | 19 << 8).outcome == "black unknown, white caught"
    o, n = _pair(rc.OPEN), _pair(rc.NO_PAIR)
    assert (o.open, o.black, o.white, o.outcome) == (True, None, None, "open") and (n.no_pair, n.black, n.outcome) == (True, None, "no pair")


def test_argument_checks():
    for bad in (dict(rules=2), dict(rules=-1), dict(max_libs=0), dict(max_libs=9), dict(max_region=0), dict(max_region=33), dict(max_nodes=0),
                dict(max_nodes=32769), dict(max_pairs=0), dict(max_pairs=65)):
        kw = dict(rules=1, max_libs=4, max_region=8, max_nodes=1024, max_pairs=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            rc.check_args(**kw)
    rc.check_args(0, 1, 1, 1, 1)
    rc.check_args(1, 8, 32, 32768, 64)
    with pytest.raises(ValueError):
        rc.host_inputs(S, 2, [(1, 2)], None)
    with pytest.raises(ValueError):
        rc.host_inputs(S, 1, None, np.zeros((1, 2), np.uint32))
    with pytest.raises(ValueError):
        rc.host_inputs(S, 2, [(1, 2), (3, 4)], np.zeros((1, 2), np.uint32))
    a, g = rc.host_inputs(S, 2, [(3, 4), (-1, -1)], np.ones((2, 2), np.uint32))
    assert a.dtype == np.int32 and a.shape == (2, 2) and g.shape == (2, 2)


def test_race_readers_and_text():
    v = _race()
    (p,) = v.pairs_of(0)
    assert len(v) == 1 and v.listed(0) == 1 and (p.anchor_b, p.anchor_w) == (2, 4) and v.find(0, 2, 4) == p and v.find(0, 4, 2) is None
    assert v.region(0, 0) == [1, 6, 8, 13] and rc.format_pair(p, V, N) == PLAIN
    assert _race(ask=(P(5, 1), P(3, 1))).pairs_of(0) == [p]          # either colour order, any stone of the chains
    assert rc.format_pair(_pair(17, catch_b=N, save_b=N), V, N).endswith("black unsettled, white safe black catch wait save pass white catch G7 save B7 nodes 6 12 17 4")
    assert " black catch none save none " in rc.format_pair(_pair(0, catch_b=-1, save_b=-1), V, N)
    assert _race(ask=(P(1, 0), P(2, 0))).pairs_of(0)[0].no_pair


def test_symbols_declared_listed_and_exported():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.build import build_lib
    build_lib()
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for s in ("sgo_race_dev", "sgo_race", "sgo_session_race"):
        assert re.search(r"\bint %s\s*\(" % s, hdr) and s in L.SYMBOLS and hasattr(lib, s), s
    assert len(lib.sgo_race_dev.argtypes) == 16 and len(lib.sgo_race.argtypes) == 13 and len(lib.sgo_session_race.argtypes) == 15
    assert "sgo_race.hip" in __import__("sejonggo_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "---- capturing races" in hdr and "a snapback under the captured stones is not read" in hdr and hdr.count("WHAT IS LEFT OUT") >= 2


# ---- the fake replay object: RecordSet.race, review --race, records --race ---------------------------------------------------------
SETUP = [(a, 1) for a in _B] + [(a, -1) for a in _W]
MISSED = [(P(0, 6), 1), (P(1, 0), -1)]                               # black plays elsewhere, white fills the black racer's liberty and wins
WON = [(P(6, 0), 1)]                                                 # black fills the white racer's liberty at once


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=RaceRecords(S, 4, 64))


def test_record_set_race_rows():
    game = _game(SETUP + MISSED, n_setup=len(SETUP))
    rs = _set(game)
    chunks = list(rs.race())
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "race"]
    ch, e = chunks[0], len(SETUP)
    assert ch.race.rows.shape == (len(game.moves) + 1, 64, 16)
    assert [p.outcome for p in ch.race.pairs_of(e)] == ["first to move wins"] and rc.format_pair(ch.race.pairs_of(e)[0], V, N) == PLAIN
    assert [(p.black, p.white) for p in ch.race.pairs_of(e + 2)] == [("caught", "safe")]      # after B7 black is in atari with white to answer


def test_review_race_flags():
    game = _game(SETUP + MISSED, n_setup=len(SETUP))
    assert review.race_rows(game, _set(game)) == {1: ["missed-race C7 at G7"], 2: ["wins-race E7"]}
    game = _game(SETUP + WON, n_setup=len(SETUP))
    assert review.race_rows(game, _set(game)) == {1: ["wins-race C7"]}
    rows = [{"move_number": m, "colour": "B", "played": "A1"} for m in (1, 9)]
    review.add_race(rows, game, record_set=_set(game))
    assert [r["race_flags"] for r in rows] == [["wins-race C7"], []]
    rows[0]["solve_flags"] = ["kills E7"]
    assert review.format_row(rows[0]).endswith("  | kills E7 wins-race C7") and "|" not in review.format_row(rows[1])
    two = [_pair(17 | 17 << 8), _pair(17, anchor_b=30, anchor_w=31, save_b=40, catch_b=41)]
    assert rc.review_flags(S, 0, 1, two, V) == ["missed-race C7 at G7", "missed-race %s at %s" % (V(30), V(40))]
    assert rc.review_flags(S, 40, 1, two, V) == ["wins-race %s" % V(30)] and rc.review_flags(S, 41, -1, two, V) == ["wins-race %s" % V(30)]
    assert rc.review_flags(S, 0, 1, [_pair(4 | 4 << 8), _pair(rc.OPEN), _pair(17, save_b=N)], V) == []


def _sgf(tmp_path, play):
    L = "abcdefg"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    text = "(;FF[4]SZ[7]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a in _B), "".join(pt(a) for a in _W)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a) if a < N else "[]") for a, c in play) + ")"
    (tmp_path / "race.sgf").write_text(text)
    return str(tmp_path / "race.sgf")


def test_review_race_loads_no_net(tmp_path, monkeypatch):
    """review.main --race alone: the rows of a review without a search, the flags behind them, and neither a net nor an engine"""
    path = _sgf(tmp_path, MISSED)
    monkeypatch.setattr(R, "DeviceRecords", RaceRecords)
    monkeypatch.setattr(review, "_net", lambda *a: (_ for _ in ()).throw(AssertionError("no net is loaded")))
    out = io.StringIO()
    assert review.main([path, "--race"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == 2 and lines[0].endswith("  | missed-race C7 at G7") and lines[1].endswith("  | wins-race E7")


def test_records_race_table(tmp_path, monkeypatch):
    _sgf(tmp_path, MISSED)
    monkeypatch.setattr(R, "DeviceRecords", RaceRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "7", "--race", "--bucket", "1"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert lines[1].startswith("moves ")
    assert [l.split() for l in lines[2:4]] == [["1-1", "1", "1.00", "0%", "100%", "0%", "0%", "1", "0"], ["2-2", "1", "1.00", "0%", "100%", "0%", "0%", "1", "1"]]
    assert lines[4] == ("race: 2 pairs in 2 positions; 2 positions offered the mover a catching or saving move; the recorded move was one 1 times; "
                        "unknown racers 0 of 4")
    rows = np.zeros((3, 2, 16), np.int64)
    rows[0, 0] = list(_pair(17 | 17 << 8))
    rows[1, 0] = list(_pair(4 | 19 << 8))
    rows[1, 1] = list(_pair(rc.OPEN))
    rows[2, 0] = list(_pair(rc.OPEN))
    rows[2, 1] = list(_pair(17 | 17 << 8))                           # behind n_pairs: not counted
    t = rc.bucket_table([0, 1, 25], [6, 6, 6], [1, -1, 1], rows, [1, 2, 1], N, 20)
    assert t == [{"from": 1, "to": 20, "plies": 2, "pairs": 3, "racers": 4, "chances": 1, "took": 1, "safe": 0, "unsettled": 2, "caught": 1, "unknown": 1},
                 {"from": 21, "to": 40, "plies": 1, "pairs": 1, "racers": 0, "chances": 0, "took": 0, "safe": 0, "unsettled": 0, "caught": 0, "unknown": 0}]
    assert " 25%" in rc.format_bucket_table(t).split("\n")[1]


class RaceEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `race` serves the model's rows of the position"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self):
        self.calls = []

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def race(self, ask=None, rules=1, max_libs=4, max_nodes=1024, max_region=8):
        self.calls.append((ask, rules, max_libs, max_nodes))
        return _race(ask, rules, max_libs, max_nodes)


@pytest.fixture()
def conf7(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_race(conf7):
    eng = RaceEngine()
    e = gtp.GTPEngine(engine=eng)
    assert e.parse_command("known_command sgo-race") == "= true\n\n" and "sgo-race" in e.parse_command("list_commands").split()
    assert e.parse_command("sgo-race") == "= " + PLAIN + "\n\n" == e.parse_command("sgo_race")
    assert e.parse_command("sgo-race F6 D6") == "= " + PLAIN + "\n\n" and eng.calls[-1] == ((P(5, 1), P(3, 1)), 1, 4, 1024)
    assert e.parse_command("sgo-race libs 1") == "=\n\n" and eng.calls[-1] == (None, 1, 1, 1024)
    assert " black unknown, white unknown " in e.parse_command("sgo-race C7 E7 nodes 3 inherited libs 2") and eng.calls[-1] == ((2, 4), 0, 2, 3)
    assert e.parse_command("sgo-race B7 C7") == "? no pair on B7 C7\n\n" and e.parse_command("sgo-race C7 D7") == "? no pair on C7 D7\n\n"
    for bad in ("sgo-race nonsense", "sgo-race C7", "sgo-race C7 E7 A1", "sgo-race nodes", "sgo-race nodes 0", "sgo-race nodes 32769", "sgo-race libs 0",
                "sgo-race libs 9", "sgo-race H7 C7", "sgo-race C8 C7", "sgo-race inherited inherited", "sgo-race libs 2 libs 3", "sgo-race pass C7"):
        assert e.parse_command(bad) == "? syntax error\n\n", bad

    class Host(object):
        """the host engine's surface: no load, no race"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-race") == "? not supported\n\n"
