"""CPU: the host side of the life-and-death reader -- the argument checks and the verdict mapping of solve.py, the `sgo-solve` text,
the flags of `review --solve`, the bucket table of `records --solve`, records.RecordSet.solve and GTP's `sgo-solve` -- on the model's
rows, on the fake replay object with the model behind it (tests/fake_solve_records.py) and on a scripted engine; no GPU.  And the
new symbols: declared, listed, exported."""
import io
import os
import re

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import solve as sv
from sejonggo_amd.sgfload import SgfGame
from tests import solve_cases as SC
from tests import solve_model as M
from tests.fake_solve_records import SolveRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 7
N = S * S
P = lambda x, y: y * S + x                                                               # noqa: E731
V = lambda a: review.vertex(a, S)                                                        # noqa: E731


def _case(name, ask=True, region=None, rules=1, max_nodes=4096):
    """(Solve with one row, stones int8 [N]) of a named 7x7 case, from the model"""
    names, recs, asks, _, _ = SC.case_records(S)
    k = names.index(name)
    m = M.solve(S, recs[k:k + 1], ask=asks[k:k + 1] if ask else None, region=None if region is None else M._words(region, 2)[None], rules=rules,
                max_nodes=max_nodes)
    black, white = M.T.record_sets(S, recs[k])[:2]
    stones = np.zeros(N, np.int8)
    stones[black], stones[white] = 1, -1
    T = max(1, len(m["rows"][0]))
    rows, regions = np.zeros((1, T, 8), np.int32), np.zeros((1, T, 2), np.uint32)
    rows[0, :len(m["rows"][0])], regions[0, :len(m["rows"][0])] = m["rows"][0], m["regions"][0]
    return sv.Solve(S, m["n_targets"], rows, regions), stones


def test_the_same_constants_as_the_header():
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for name, val in (("A_DEAD", 1), ("D_DEAD", 2), ("A_UNKNOWN", 4), ("D_UNKNOWN", 8), ("D_RAN", 16), ("OPEN", 32), ("NO_STONE", 64),
                      ("MAX_REGION", 32), ("MAX_NODES", 65536), ("MAX_TARGETS", 64)):
        assert re.search(r"#define SGO_SOLVE_%s %d\b" % (name, val), hdr), name
        assert getattr(sv, name) == val == getattr(M, name), name
    assert re.search(r"#define SGO_SOLVE_MAX_DEPTH 80\b", hdr) and M.MAX_DEPTH == 80


def test_verdict_mapping():
    v = sv.verdict_of
    assert v(0) == "alive" and v(sv.A_DEAD | sv.D_RAN) == "unsettled" and v(sv.A_DEAD | sv.D_RAN | sv.D_DEAD) == "dead"
    assert v(sv.A_UNKNOWN) == "unknown" and v(sv.A_DEAD | sv.D_RAN | sv.D_UNKNOWN) == "unknown" and v(sv.OPEN) == "open" and v(sv.NO_STONE) is None
    assert all(v(s) == SC.verdict([0, 0, 0, s]) for s in (0, 17, 19, 4, 25, 32)) and sv.VERDICTS == ("alive", "unsettled", "dead", "unknown", "open")
    t = sv.Target(5, 1, 3, 17, 4, 4, 1, 4)
    assert t.verdict == "unsettled" and (t.kill_move, t.live_move, t.nodes_a, t.nodes_d) == (4, 4, 1, 4)


def test_argument_checks():
    for bad in (dict(rules=2), dict(rules=-1), dict(max_region=0), dict(max_region=33), dict(max_nodes=0), dict(max_nodes=65537),
                dict(max_targets=0), dict(max_targets=65)):
        kw = dict(rules=1, max_region=12, max_nodes=4096, max_targets=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            sv.check_args(**kw)
    sv.check_args(0, 1, 1, 1)
    sv.check_args(1, 32, 65536, 64)
    with pytest.raises(ValueError):
        sv.host_inputs(S, 2, [1], None)
    with pytest.raises(ValueError):
        sv.host_inputs(S, 1, None, np.zeros((1, 2), np.uint32))
    with pytest.raises(ValueError):
        sv.host_inputs(S, 2, [1, 2], np.zeros((1, 2), np.uint32))
    a, g = sv.host_inputs(S, 2, [3, -1], np.ones((2, 2), np.uint32))
    assert a.dtype == np.int32 and g.shape == (2, 2) and sv.region_words(S, [0, 33]).tolist() == [1, 2]


def test_solve_readers_and_text():
    v, stones = _case("connect_b")
    (t,) = v.targets_of(0)
    assert len(v) == 1 and v.listed(0) == 1 and t.anchor == 5 and v.find(0, 5) == t and v.find(0, 6) is None
    assert v.region(0, 0) == [0, 1, 2, 3, 4, 5, 7, 8, 9, 10]
    assert sv.format_target(t, V, N) == "F7 black empty 3 unsettled kill E7 live E7 nodes 1 4"
    board = sv.format_board(S, stones, v.region(0, 0), t).split("\n")
    assert board[0].split() == ["*", "X", "*", "X", "!", "X", "O"] and board[1].split() == ["X", "X", "X", "X", "O", "O", "O"] and len(board) == S
    dead = _case("connect_b", rules=0)[0].targets_of(0)[0]
    assert sv.format_target(dead, V, N) == "F7 black empty 3 dead kill E7 live none nodes 1 2"
    assert sv.format_board(S, stones, v.region(0, 0), dead).split("\n")[0].split()[4] == "K"
    seki = _case("seki_b")[0].targets_of(0)[0]
    assert seki.verdict == "alive" and sv.format_target(seki, V, N).endswith("alive kill none live none nodes 285 0")
    assert sv.format_target(sv.Target(5, -1, 3, 17, 4, N, 1, 4), V, N) == "F7 white empty 3 unsettled kill E7 live pass nodes 1 4"
    both = _case("seki_b", ask=False)[0]
    assert [(t.anchor, t.colour, t.verdict) for t in both.targets_of(0)] == [(0, -1, "dead"), (4, 1, "alive")]


def test_symbols_declared_listed_and_exported():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.build import build_lib
    build_lib()
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "sgo.h")).read()
    for s in ("sgo_solve_dev", "sgo_solve", "sgo_session_solve"):
        assert re.search(r"\bint %s\s*\(" % s, hdr) and s in L.SYMBOLS and hasattr(lib, s), s
    assert len(lib.sgo_solve_dev.argtypes) == 15 and len(lib.sgo_solve.argtypes) == 12 and len(lib.sgo_session_solve.argtypes) == 14
    assert "sgo_solve.hip" in __import__("sejonggo_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "---- life and death" in hdr and "EVERY VERDICT HOLDS\n * FOR THE CHOSEN RULE SET" in hdr and "WHAT IS LEFT OUT" in hdr


# ---- the fake replay object: RecordSet.solve, review --solve, records --solve -----------------------------------------------------
# `connect` as set-up stones (the stone on F7 is unsettled, E7 both kills and saves it), then: black passes (the save is missed),
# white plays elsewhere (the kill is missed), black connects (saved)
_B, _W = SC.diagram(S, [".X.X.XO", "XXXXOOO", "OOOOO"])
SETUP = [(a, 1) for a in _B] + [(a, -1) for a in _W]
SAVED = [(N, 1), (P(6, 6), -1), (P(4, 0), 1)]
KILLED = [(P(0, 6), 1), (P(4, 0), -1)]


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=SolveRecords(S, 4, 64))


def test_record_set_solve_rows():
    game = _game(SETUP + SAVED, n_setup=len(SETUP))
    rs = _set(game)
    chunks = list(rs.solve(stones=True))
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "solve"]
    ch, e = chunks[0], len(SETUP)
    assert ch.solve.rows.shape == (len(game.moves) + 1, 16, 8) and ch.stones.shape == (len(game.moves) + 1, N)
    assert [t.verdict for t in ch.solve.targets_of(e)] == ["unsettled"] and ch.solve.targets_of(e)[0].anchor == 5
    assert ch.solve.targets_of(e + 3) == [] and ch.stones[e + 3, P(4, 0)] == 1          # connected: pass-alive, nothing listed


def test_review_solve_flags():
    game = _game(SETUP + SAVED, n_setup=len(SETUP))
    assert review.solve_rows(game, _set(game)) == {1: ["missed-save F7 at E7"], 2: ["missed-kill F7 at E7"], 3: ["saves F7"]}
    game = _game(SETUP + KILLED, n_setup=len(SETUP))
    assert review.solve_rows(game, _set(game)) == {1: ["missed-save F7 at E7"], 2: ["kills F7"]}
    rows = [{"move_number": m, "colour": "B", "played": "A1"} for m in (1, 2, 9)]
    review.add_solve(rows, game, record_set=_set(game))
    assert [r["solve_flags"] for r in rows] == [["missed-save F7 at E7"], ["kills F7"], []]
    rows[1]["secure_flags"] = ["secures 3"]
    assert review.format_row(rows[1]).endswith("  | secures 3 kills F7") and "|" not in review.format_row(rows[2])


def _sgf(tmp_path, play):
    L = "abcdefg"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    text = "(;FF[4]SZ[7]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a in _B), "".join(pt(a) for a in _W)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a) if a < N else "[]") for a, c in play) + ")"
    (tmp_path / "eye.sgf").write_text(text)
    return str(tmp_path / "eye.sgf")


def test_review_solve_loads_no_net(tmp_path, monkeypatch):
    """review.main --solve alone: the rows of a review without a search, the flags behind them, and neither a net nor an engine"""
    path = _sgf(tmp_path, SAVED)
    monkeypatch.setattr(R, "DeviceRecords", SolveRecords)
    monkeypatch.setattr(review, "_net", lambda *a: (_ for _ in ()).throw(AssertionError("no net is loaded")))
    out = io.StringIO()
    assert review.main([path, "--solve"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == 3 and lines[0].endswith("  | missed-save F7 at E7") and lines[1].endswith("  | missed-kill F7 at E7")
    assert lines[2].endswith("  | saves F7")


def test_records_solve_table(tmp_path, monkeypatch):
    _sgf(tmp_path, SAVED)
    monkeypatch.setattr(R, "DeviceRecords", SolveRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "7", "--solve", "--bucket", "2"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert lines[1].startswith("moves ") and [l.split() for l in lines[2:4]] == [["1-2", "2", "2", "2", "0", "0.0%"], ["3-4", "1", "1", "1", "1", "0.0%"]]
    assert lines[4] == "solve: 3 of 3 positions hold an unsettled enclosed chain; the recorded move was its kill or live move 1 times; unknown rows 0 of 3"
    rows = np.zeros((3, 2, 8), np.int64)
    rows[0, 0] = [5, 1, 3, 17, 4, 4, 1, 4]
    rows[1, 0] = [5, 1, 3, 4, -1, -1, 9, 0]
    rows[2, 1] = [5, 1, 3, 17, 7, 7, 1, 4]                           # behind n_targets: not counted
    t = sv.bucket_table([0, 1, 25], [4, 4, 7], rows, [1, 1, 1], 20)
    assert t == [{"from": 1, "to": 20, "plies": 2, "rows": 2, "unsettled": 1, "took": 1, "unknown": 1},
                 {"from": 21, "to": 40, "plies": 1, "rows": 1, "unsettled": 0, "took": 0, "unknown": 0}]
    assert "50.0%" in sv.format_bucket_table(t).split("\n")[1]


class SolveEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `solve` serves the model's row of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, case):
        self.case, self.calls = case, []

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def solve(self, ask=None, region=None, rules=1, max_nodes=4096, max_region=12):
        self.calls.append((ask, region, rules, max_nodes))
        if ask is not None and ask != P(5, 0):
            return sv.Solve(S, [1], [[[-1, 0, 0, sv.NO_STONE, -1, -1, 0, 0]]], np.zeros((1, 1, 2), np.uint32)), np.zeros(N, np.int8)
        return _case(self.case, ask is not None, region, rules, max_nodes)


@pytest.fixture()
def conf7(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_solve(conf7):
    eng = SolveEngine("connect_b")
    e = gtp.GTPEngine(engine=eng)
    assert e.parse_command("known_command sgo-solve") == "= true\n\n" and "sgo-solve" in e.parse_command("list_commands").split()
    v, stones = _case("connect_b")
    t = v.targets_of(0)[0]
    want = sv.format_target(t, V, N) + "\n" + sv.format_board(S, stones, v.region(0, 0), t)
    assert e.parse_command("sgo-solve F7") == "= " + want + "\n\n" == e.parse_command("sgo_solve F7")
    assert e.parse_command("sgo-solve F7").startswith("= F7 black empty 3 unsettled kill E7 live E7 nodes 1 4\n* X * X ! X O\n")
    assert " dead kill E7 live none " in e.parse_command("sgo-solve F7 inherited")
    assert " empty 2 alive kill none live none nodes 1 0" in e.parse_command("sgo-solve F7 A7 C7 nodes 50")
    assert eng.calls[-1] == (P(5, 0), [P(0, 0), P(2, 0)], 1, 50) and eng.calls[-2] == (P(5, 0), None, 0, 4096)
    assert e.parse_command("sgo-solve") == "= F7 black empty 3 unsettled kill E7 live E7 nodes 1 4\n\n"
    assert e.parse_command("sgo-solve E7") == "? no stone on E7\n\n"
    for bad in ("sgo-solve nonsense", "sgo-solve F7 nodes", "sgo-solve F7 nodes 0", "sgo-solve F7 nodes 65537", "sgo-solve H7", "sgo-solve F8",
                "sgo-solve inherited inherited", "sgo-solve F7 nodes 5 nodes 6", "sgo-solve pass"):
        assert e.parse_command(bad) == "? syntax error\n\n", bad

    class Host(object):
        """the host engine's surface: no load, no solve"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-solve") == "? not supported\n\n"
