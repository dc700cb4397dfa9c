"""CPU: the host side of the connection reader -- the argument checks, the verdict words of connect.py, the `sgo-connect` and
`sgo-groups` texts, the flags of `review --connect`, the bucket table of `records --connect`, records.RecordSet.connect and GTP's two
commands -- on the model's rows, on the fake replay object with the model behind it (tests/fake_connect_records.py) and on a scripted
engine; no GPU.  And the new symbols: declared, listed, exported."""
import io
import os
import re

import numpy as np
import pytest

from sejonggo_amd import connect as cn
from sejonggo_amd import gtp, records as R, review
from sejonggo_amd.sgfload import SgfGame
from tests import connect_model as M
from tests.fake_connect_records import ConnectRecords
from tests.tactics_cases import diagram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 7
N = S * S
P = lambda x, y: y * S + x                                                               # noqa: E731
V = lambda a: review.vertex(a, S)                                                        # noqa: E731

# the one-point jump at 7x7: B5 and D5 (black), cut at C5, the first join found at C6; a white stone far away
_B, _W = diagram(S, ["", "", ".X.X", "", "", "", ".....O"])
JUMP = "B5 D5 black shared 1 links 1 empty 3 cutting 0 unsettled cut C5 join C6 nodes 8 10"


def _connect(ask=None, rules=1, cut_libs=1, max_nodes=1024, white_to_play=False, black=_B, white=_W):
    """(Connect with one row of the position, its stones), from the model"""
    rec = M.build_record(S, black, white, white_to_play)
    m = M.connect(S, rec[None], ask=None if ask is None else [ask], rules=rules, cut_libs=cut_libs, max_nodes=max_nodes)
    T = max(1, len(m["rows"][0]))
    rows, regions = np.zeros((1, T, 12), np.int32), np.zeros((1, T, 2), np.uint32)
    rows[0, :len(m["rows"][0])], regions[0, :len(m["rows"][0])] = m["rows"][0], m["regions"][0]
    stones = np.zeros(N, np.int8)
    stones[black], stones[white] = 1, -1
    return cn.Connect(S, m["n_pairs"], rows, regions, m["groups"][0][None], m["counts"][0][None]), stones


def test_the_same_constants_as_the_header():
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for name, val in (("A_CUT", 1), ("D_CUT", 2), ("A_UNKNOWN", 4), ("D_UNKNOWN", 8), ("D_RAN", 16), ("MAX_CUT_LIBS", 4), ("MAX_REGION", 32),
                      ("MAX_NODES", 32768), ("MAX_PAIRS", 64)):
        assert re.search(r"#define SGO_CONNECT_%s %d\b" % (name, val), hdr), name
        assert getattr(cn, name) == val == getattr(M, name), name
    assert re.search(r"#define SGO_CONNECT_OPEN \(1 << 16\)", hdr) and re.search(r"#define SGO_CONNECT_NO_PAIR \(1 << 17\)", hdr)
    assert cn.OPEN == M.OPEN == 1 << 16 and cn.NO_PAIR == M.NO_PAIR == 1 << 17 and cn.WORDS == M.W == 12
    assert re.search(r"#define SGO_CONNECT_MAX_DEPTH 80\b", hdr) and M.MAX_DEPTH == 80
    assert (cn.FLAG_CUT_TABLE, cn.FLAG_UNDECIDED) == (M.FLAG_CUT_TABLE, M.FLAG_UNDECIDED) == (1, 2)


def _pair(status, **kw):
    f = dict(anchor_x=15, anchor_y=17, colour=1, shared=1, links=1, region_empty=3, status=status, cutting=0, cut_move=16, join_move=9,
             nodes_a=8, nodes_d=10)
    f.update(kw)
    return cn.Pair(**f)


def test_verdict_words():
    v = cn.verdict_of
    assert [v(s) for s in (0, 17, 19, 4, 25, cn.OPEN, cn.NO_PAIR)] == ["connected", "unsettled", "cut", "unknown", "unknown", "open", "no pair"]
    assert cn.VERDICTS == ("connected", "unsettled", "cut", "unknown", "open")
    for st in (0, 17, 19, 4, 25, cn.OPEN, cn.NO_PAIR):
        assert _pair(st).verdict.replace(" ", "_") == M.verdict([0] * 6 + [st])
    assert _pair(cn.OPEN).open and _pair(cn.NO_PAIR).no_pair and not _pair(17).open


def test_argument_checks():
    for bad in (dict(rules=2), dict(rules=-1), dict(cut_libs=-1), dict(cut_libs=5), dict(max_region=0), dict(max_region=33), dict(max_nodes=0),
                dict(max_nodes=32769), dict(max_pairs=0), dict(max_pairs=65)):
        kw = dict(rules=1, cut_libs=1, max_region=8, max_nodes=1024, max_pairs=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            cn.check_args(**kw)
    cn.check_args(0, 0, 1, 1, 1)
    cn.check_args(1, 4, 32, 32768, 64)
    with pytest.raises(ValueError):
        cn.host_inputs(S, 2, [(1, 2)], None)
    with pytest.raises(ValueError):
        cn.host_inputs(S, 1, None, np.zeros((1, 2), np.uint32))
    a, g = cn.host_inputs(S, 2, [(3, 4), (-1, -1)], np.ones((2, 2), np.uint32))
    assert a.dtype == np.int32 and a.shape == (2, 2) and g.shape == (2, 2)


def test_connect_readers_and_text():
    v, stones = _connect()
    (p,) = v.pairs_of(0)
    assert len(v) == 1 and v.listed(0) == 1 and (p.anchor_x, p.anchor_y) == (15, 17) and v.find(0, 15, 17) == p and v.find(0, 17, 15) is None
    assert v.region(0, 0) == [9, 16, 23] and v.verdicts(0) == ["unsettled"] and cn.format_pair(p, V, N) == JUMP
    assert _connect(ask=(17, 15))[0].pairs_of(0) == [p]              # either order
    assert v.groups_of(0) == {15: [15], 17: [17], 47: [47]} and v.group_counts[0].tolist() == [3, 3, 0, 0]
    assert cn.format_pair(_pair(19, cut_move=N, join_move=-1), V, N).endswith(" cut cut pass join none nodes 8 10")
    assert cn.format_pair(_pair(cn.NO_PAIR), V, N) == "no pair" and _connect(ask=(15, 47))[0].pairs_of(0)[0].no_pair
    text = cn.format_groups(S, v.groups[0], set(_B))
    assert text.split("\n") == [" 7 . . . . . . .", " 6 . . . . . . .", " 5 . A . B . . .", " 4 . . . . . . .", " 3 . . . . . . .",
                                " 2 . . . . . . .", " 1 . . . . . a .", "   A B C D E F G"]
    b, w = diagram(S, ["", ".X", "..X", "...X"])
    v3, _ = _connect(black=b, white=[])
    assert v3.group_counts[0].tolist() == [3, 1, 2, 0] and cn.format_groups(S, v3.groups[0], set(b)).split("\n")[1:4] == [
        " 6 . A . . . . .", " 5 . . A . . . .", " 4 . . . A . . ."]


def test_symbols_declared_listed_and_exported():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.build import build_lib
    build_lib()
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for s in ("sgo_connect_dev", "sgo_connect", "sgo_session_connect"):
        assert re.search(r"\bint %s\s*\(" % s, hdr) and s in L.SYMBOLS and hasattr(lib, s), s
    assert len(lib.sgo_connect_dev.argtypes) == 18 and len(lib.sgo_connect.argtypes) == 15 and len(lib.sgo_session_connect.argtypes) == 17
    assert "sgo_connect.hip" in __import__("sejonggo_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "---- connections" in hdr and "is not about whether the joined chain lives" in hdr and hdr.count("WHAT IS LEFT OUT") >= 3


# ---- the fake replay object: RecordSet.connect, review --connect, records --connect ------------------------------------------------
SETUP = [(a, 1) for a in _B] + [(a, -1) for a in _W]
MISSED = [(P(0, 6), -1), (P(2, 1), 1)]                               # white plays elsewhere, black joins
CUT = [(P(2, 2), -1)]                                                # white cuts at once


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=ConnectRecords(S, 4, 64))


def test_record_set_connect_rows():
    game = _game(SETUP + MISSED, n_setup=len(SETUP))
    rs = _set(game)
    chunks = list(rs.connect())
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "connect"]
    ch, e = chunks[0], len(SETUP)
    assert ch.connect.rows.shape == (len(game.moves) + 1, 64, 12) and ch.connect.groups.shape == (len(game.moves) + 1, N)
    assert ch.connect.verdicts(e) == ["unsettled"] and cn.format_pair(ch.connect.pairs_of(e)[0], V, N) == JUMP
    assert ch.connect.group_counts[e].tolist() == [3, 3, 0, 0]
    after = ch.connect.pairs_of(e + 2)                                # after C6 the three stones are tied: C6 with each neighbour
    assert after and all(p.verdict == "connected" for p in after if p.colour == 1) and ch.connect.group_counts[e + 2][1] < ch.connect.group_counts[e + 2][0]


def test_review_connect_flags():
    game = _game(SETUP + MISSED, n_setup=len(SETUP))
    assert review.connect_rows(game, _set(game)) == {1: ["missed-cut B5 at C5"], 2: ["joins B5"]}
    game = _game(SETUP + CUT, n_setup=len(SETUP))
    assert review.connect_rows(game, _set(game)) == {1: ["cuts B5"]}
    rows = [{"move_number": m, "colour": "W", "played": "A1"} for m in (1, 9)]
    review.add_connect(rows, game, record_set=_set(game))
    assert [r["connect_flags"] for r in rows] == [["cuts B5"], []]
    rows[0]["race_flags"] = ["wins-race E7"]
    assert review.format_row(rows[0]).endswith("  | wins-race E7 cuts B5") and "|" not in review.format_row(rows[1])
    two = [_pair(17), _pair(17, anchor_x=30, anchor_y=32, colour=-1, cut_move=31, join_move=24)]
    assert cn.review_flags(S, 0, 1, two, V) == ["missed-cut %s at %s" % (V(30), V(31)), "missed-join B5 at C6"]
    assert cn.review_flags(S, 31, 1, two, V) == ["cuts %s" % V(30), "missed-join B5 at C6"]
    assert cn.review_flags(S, 24, -1, two, V) == ["missed-cut B5 at C5", "joins %s" % V(30)]
    assert cn.review_flags(S, 0, 1, [_pair(4), _pair(cn.OPEN), _pair(19), _pair(0), _pair(17, join_move=-1, colour=1), _pair(17, colour=-1, cut_move=N)], V) == []


def _sgf(tmp_path, play):
    L = "abcdefg"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    text = "(;FF[4]SZ[7]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a in _B), "".join(pt(a) for a in _W)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a) if a < N else "[]") for a, c in play) + ")"
    (tmp_path / "connect.sgf").write_text(text)
    return str(tmp_path / "connect.sgf")


def test_review_connect_loads_no_net(tmp_path, monkeypatch):
    """review.main --connect alone: the rows of a review without a search, the flags behind them, and neither a net nor an engine"""
    path = _sgf(tmp_path, MISSED)
    monkeypatch.setattr(R, "DeviceRecords", ConnectRecords)
    monkeypatch.setattr(review, "_net", lambda *a: (_ for _ in ()).throw(AssertionError("no net is loaded")))
    out = io.StringIO()
    assert review.main([path, "--connect"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == 2 and lines[0].endswith("  | missed-cut B5 at C5") and lines[1].endswith("  | joins B5")


def test_records_connect_table(tmp_path, monkeypatch):
    _sgf(tmp_path, MISSED)
    monkeypatch.setattr(R, "DeviceRecords", ConnectRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "7", "--connect", "--bucket", "1"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert lines[1].startswith("moves ") and lines[1].split()[-2:] == ["chains/ply", "groups/ply"]
    assert [l.split() for l in lines[2:4]] == [["1-1", "1", "1.00", "0%", "100%", "0%", "0%", "0%", "3.00", "3.00"],
                                               ["2-2", "1", "1.00", "0%", "100%", "0%", "0%", "0%", "4.00", "4.00"]]
    assert lines[4] == "connect: 2 pairs in 2 positions (2 found, 0 tables cut); connected 0 unsettled 2 cut 0 unknown 0 open 0; 7 chains in 7 groups"
    rows = np.zeros((3, 2, 12), np.int64)
    rows[0, 0] = list(_pair(0))
    rows[1, 0] = list(_pair(4))
    rows[1, 1] = list(_pair(cn.OPEN))
    rows[2, 0] = list(_pair(19))
    rows[2, 1] = list(_pair(17))                                     # behind n_pairs: not counted
    t = cn.bucket_table([0, 1, 25], rows, [1, 2, 1], [[5, 4, 1, 0], [6, 6, 0, 2], [9, 9, 0, 1]], 20)
    assert t == [{"from": 1, "to": 20, "plies": 2, "pairs": 3, "found": 3, "chains": 11, "groups": 10, "cut_tables": 0, "connected": 1,
                  "unsettled": 0, "cut": 0, "unknown": 1, "open": 1},
                 {"from": 21, "to": 40, "plies": 1, "pairs": 1, "found": 1, "chains": 9, "groups": 9, "cut_tables": 1, "connected": 0,
                  "unsettled": 0, "cut": 1, "unknown": 0, "open": 0}]
    assert " 33%" in cn.format_bucket_table(t).split("\n")[1] and cn.format_bucket_table(t).split("\n")[1].split()[-2:] == ["5.50", "5.00"]


class ConnectEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `connect` serves the model's rows of the position"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self):
        self.calls = []

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def connect(self, ask=None, rules=1, cut_libs=1, max_nodes=1024, max_region=8):
        self.calls.append((ask, rules, cut_libs, max_nodes))
        return _connect(ask, rules, cut_libs, max_nodes)


@pytest.fixture()
def conf7(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_connect_and_groups(conf7):
    eng = ConnectEngine()
    e = gtp.GTPEngine(engine=eng)
    for name in ("sgo-connect", "sgo-groups"):
        assert e.parse_command("known_command " + name) == "= true\n\n" and name in e.parse_command("list_commands").split()
    assert e.parse_command("sgo-connect") == "= " + JUMP + "\n\n" == e.parse_command("sgo_connect")
    assert e.parse_command("sgo-connect D5 B5") == "= " + JUMP + "\n\n" and eng.calls[-1] == ((17, 15), 1, 1, 1024)
    assert e.parse_command("sgo-connect cutlibs 0") == "= " + JUMP + "\n\n" and eng.calls[-1] == (None, 1, 0, 1024)
    assert " unknown cut none join none nodes 4 0" in e.parse_command("sgo-connect B5 D5 nodes 3 inherited cutlibs 2") and eng.calls[-1] == ((15, 17), 0, 2, 3)
    assert e.parse_command("sgo-connect B5 F1") == "? no pair on B5 F1\n\n" and e.parse_command("sgo-connect B5 C5") == "? no pair on B5 C5\n\n"
    for bad in ("sgo-connect nonsense", "sgo-connect B5", "sgo-connect B5 D5 A1", "sgo-connect nodes", "sgo-connect nodes 0", "sgo-connect nodes 32769",
                "sgo-connect cutlibs 5", "sgo-connect H7 C7", "sgo-connect C8 C7", "sgo-connect inherited inherited", "sgo-connect cutlibs 2 cutlibs 3",
                "sgo-connect pass C7", "sgo-groups B5 D5", "sgo-groups nodes 0"):
        assert e.parse_command(bad) == "? syntax error\n\n", bad
    text = e.parse_command("sgo-groups nodes 64")
    assert eng.calls[-1] == (None, 1, 1, 64) and text.startswith("=  7 . . . . . . .\n") and " 5 . A . B . . .\n" in text
    assert text.endswith("   A B C D E F G\nchains 3 groups 3 connected 0\n\n")
    assert e.parse_command("sgo-groups nodes 3").endswith("chains 3 groups 3 connected 0 undecided\n\n")

    class Host(object):
        """the host engine's surface: no load, no connect"""
        model = type("N", (), {"name": "x"})()

    host = gtp.GTPEngine(engine=Host())
    assert host.parse_command("sgo-connect") == "? not supported\n\n" == host.parse_command("sgo-groups")
