"""CPU: the Python layers above the superko kernels (superko.py, records.py, review.py, gtp.py) on a fake backend that serves the
model's rows (tests/fake_superko_records.py): which history each record is given, the texts of the two command-line tools on a small
game with a known cycle, and GTP's refusal, fallback and listing on a scripted engine."""
import io
import json

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import superko as sk
from tests import superko_cases as SC
from tests import superko_model as SM
from tests.fake_superko_records import SuperkoRecords

S = 5
P = lambda x, y: y * S + x                                                               # noqa: E731
# black builds the corner, white answers elsewhere, then sending two (B A5), returning one (W C5 takes two, B B5 takes one back): the stones
# after move 9 are those after move 6
CYCLE = [(P(1, 0), 1), (P(0, 1), -1), (P(3, 0), 1), (P(1, 1), -1), (P(2, 1), 1), (P(4, 3), -1), (P(0, 0), 1), (P(2, 0), -1), (P(1, 0), 1),
         (P(4, 4), -1)]


def cycle_sgf():
    L = "abcde"
    return "(;FF[4]SZ[5]KM[5.5]" + "".join(";%s[%s]" % ("B" if c > 0 else "W", "" if a == S * S else L[a % S] + L[a // S]) for a, c in CYCLE) + ")"


def _record(name, entries):
    return R.Record(name, S, list(entries), [False] * len(entries), list(range(1, len(entries) + 1)), None)


def test_symbols_are_bound():
    from sejonggo_amd import _lib
    assert {"sgo_superko_dev", "sgo_superko", "sgo_superko_mode"} <= set(_lib.SYMBOLS)
    assert sk.rule_of("positional") == 0 and sk.rule_of("situational") == 1 and sk.rule_of(1) == 1
    with pytest.raises(ValueError):
        sk.rule_of("natural")


def test_record_set_gives_every_record_its_own_game():
    """first = base_g for the records of game g, -1 (with index -1) behind a refused entry; the rows are the model's"""
    cut = [(P(2, 2), 1), (P(2, 2), -1), (P(0, 0), 1)]                # the second entry lands on a stone
    rs = R.RecordSet([_record("cycle", CYCLE), _record("cut", cut), _record("one", [(P(1, 1), 1)])], S, backend=SuperkoRecords(S, 8, 64))
    chunks = list(rs.superko(rule=1))
    assert len(chunks) == 1 and rs.refused == [("cut", -101, 1)]
    index, first, rule, used = rs.backend.asked[0]
    n0, n1 = len(CYCLE) + 1, len(cut) + 1
    assert index == list(range(n0)) + [n0, n0 + 1, -1, -1] + [n0 + n1, n0 + n1 + 1]
    assert first == [0] * n0 + [n0, n0, -1, -1] + [n0 + n1] * 2 and rule == 1 and used == len(index)
    v = chunks[0].superko
    assert len(v) == len(index) and not v.counts[n0 + 2].any() and (v.back[n0 + 2] == -1).all()
    assert v.counts[:n0, 5].tolist() == list(range(1, n0 + 1)) and v.counts[n0, 5] == 1 and v.counts[n0 + n1 + 1, 5] == 2
    # the cycle: B5 from record 8 gives the stones of record 6 -- with the other side to move, so only the positional rule sees it
    assert v.extra(8) == [] and v.count(9, "seen") == 0
    v0 = next(R.RecordSet([_record("cycle", CYCLE)], S, backend=SuperkoRecords(S, 8, 64)).superko()).superko
    assert v0.extra(8) == [(P(1, 0), 2)] and v0.repeat(8) == [(P(1, 0), 2)] and v0.count(9, "seen") == 3 and v0.played(8, P(1, 0)) == (True, True, 2)
    assert v0.count(8, "max_back") == 2 and v0.count(8, "max_back_point") == P(1, 0) and not v0.legal(8)[P(1, 0)] and v0.legal(8)[S * S]
    assert v0.count(6, "seen") == 0 and v0.count(6, "history") == 7


def test_records_superko_text(tmp_path, monkeypatch):
    (tmp_path / "cycle.sgf").write_text(cycle_sgf())
    (tmp_path / "open.sgf").write_text("(;FF[4]SZ[5]KM[5.5];B[cc];W[bb];B[])")
    monkeypatch.setattr(R, "DeviceRecords", SuperkoRecords)
    out, doc = io.StringIO(), tmp_path / "doc.json"
    assert R.main([str(tmp_path), "--size", "5", "--superko", "--json", str(doc)], out=out) == 0
    text = out.getvalue().split("\n")
    at = text.index("superko (positional)")
    assert text[at + 1:at + 3] == ["cycle: cycled at move 9 (3 plies back)", "cycle: move 9 B5 repeats a position, back 2"]
    assert text[at + 3] == "games 2  cycled 1  repetitions played through 1  ko recaptures played through 0"
    assert text[at + 5].split() == ["1-20", "15", "1", "0.067"]
    d = json.loads(doc.read_text())["superko"]
    assert d["rule"] == "positional" and d["positions_with_extra"] == 1 and d["max_back"] == 2
    assert [g["cycled_at"] for g in d["games"]] == [9, None] and d["games"][0]["through"] == [{"ply": 9, "action": P(1, 0), "back": 2}]
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "5", "--superko", "situational"], out=out) == 0
    text = out.getvalue().split("\n")
    at = text.index("superko (situational)")
    assert text[at + 1] == "games 2  cycled 0  repetitions played through 0  ko recaptures played through 0"


def test_review_superko_text_without_a_net(tmp_path, monkeypatch):
    path = tmp_path / "cycle.sgf"
    path.write_text(cycle_sgf())
    monkeypatch.setattr(R, "DeviceRecords", SuperkoRecords)
    monkeypatch.setattr(review, "_net", lambda *a: pytest.fail("a net was asked for"))
    out = io.StringIO()
    assert review.main([str(path), "--superko"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == len(CYCLE) and lines[8] == "   9 B B5    | repeats 2 superko-forbidden B5"
    assert all("|" not in l for i, l in enumerate(lines) if i != 8)
    out = io.StringIO()
    assert review.main([str(path), "--superko", "situational"], out=out) == 0 and "|" not in out.getvalue()


# ---- GTP -------------------------------------------------------------------------------------------------------------------------
class ScriptedEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `superko` serves the model's row for the move list
    played so far (replayed by the records model), `report` a canned table"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, entries, counts=None, means=None):
        self.size, self.moves, self.calls = S, list(entries), []
        self.counts, self.means = counts, means

    @property
    def board(self):
        b = np.zeros((1, S, S, 17), np.int32)
        b[..., 16] = 1 if self._to_move() > 0 else -1
        return b

    def _to_move(self):
        return -self.moves[-1][1] if self.moves else 1

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def superko(self, rule=0):
        from tests import records_model
        self.calls.append(("superko", sk.rule_of(rule)))
        rep = records_model.replay(S, [([a for a, _ in self.moves], [c for _, c in self.moves])])
        n = len(self.moves)
        m = SM.superko(S, rep["records"][:n + 1], [(n, 0)], sk.rule_of(rule))
        return sk.Superko(S, m["sets"], m["back"], m["counts"])

    def play(self, color, x, y, update_tree=True):
        self.calls.append(("play", color, x, y))
        self.moves.append((S * S if y >= S else y * S + x, color))
        return self.board, color

    def genmove(self, color):
        self.calls.append(("genmove", color))
        self.moves.append((P(4, 4), color))
        return 4, 4, None, 0.0, self.board, color

    def analyze(self, sims=None):
        self.calls.append(("analyze", sims))
        return None, 0.0

    def report(self, top=5, depth=8):
        self.calls.append(("report",))
        return {"N": np.asarray([self.counts], np.int32), "Q": np.asarray([self.means], np.float32)}


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_superko_needs_the_device(conf5, capsys):
    assert gtp.main(inp=io.StringIO(""), out=io.StringIO(), device=False, superko="positional") == 2
    assert "--superko needs the device engine" in capsys.readouterr().err
    assert gtp._cli(["--superko", "situational"]) == 2

    class Host(object):
        model = type("N", (), {"name": "x"})()

    with pytest.raises(ValueError):
        gtp.GTPEngine(engine=Host(), superko="positional")
    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-superko") == "? not supported\n\n"


def test_gtp_sgo_superko_play_and_genmove(conf5):
    before = CYCLE[:8]                                               # black to move; B5 would repeat
    eng = ScriptedEngine(before)
    e = gtp.GTPEngine(engine=eng)                                    # without the option: the listing only
    assert "sgo-superko" in e.parse_command("list_commands").split() and e.parse_command("known_command sgo-superko") == "= true\n\n"
    assert e.parse_command("sgo-superko") == "= B5 2 forbidden\n\n" and e.parse_command("sgo_superko positional") == "= B5 2 forbidden\n\n"
    assert e.parse_command("sgo-superko situational") == "=\n\n"
    assert e.parse_command("sgo-superko natural") == "? syntax error\n\n" and e.parse_command("sgo-superko positional x") == "? syntax error\n\n"
    assert e.parse_command("play B B5") == "=\n\n" and eng.moves[-1] == (P(1, 0), 1)   # nothing is refused without the option
    # with it: the repeat is refused and the game is as it was; another move, a pass and a stone out of turn go through
    eng = ScriptedEngine(before)
    e = gtp.GTPEngine(engine=eng, superko="positional")
    assert e.parse_command("play B B5") == "? illegal move\n\n" and eng.moves == before and ("play", 1, 1, 0) not in eng.calls
    assert e.parse_command("play W B5") == "=\n\n" and eng.moves[-1] == (P(1, 0), -1)
    eng = ScriptedEngine(before)
    e = gtp.GTPEngine(engine=eng, superko="situational")
    assert e.parse_command("play B B5") == "=\n\n"                  # the other side is to move in the earlier position
    # genmove while extra is not empty: analyze, report, the best child by (N, Q, higher index) outside extra, through play
    N, Q = np.full(S * S + 1, -1, np.int32), np.zeros(S * S + 1, np.float32)
    N[[P(1, 0), P(0, 0), P(4, 4), P(3, 3), S * S]] = [90, 7, 7, 7, 2]
    Q[[P(0, 0), P(4, 4), P(3, 3)]] = [0.25, 0.5, 0.5]
    eng = ScriptedEngine(before, N, Q)
    e = gtp.GTPEngine(engine=eng, superko="positional")
    assert e.parse_command("genmove b") == "= E1\n\n" and eng.moves[-1] == (P(4, 4), 1)
    assert [c[0] for c in eng.calls] == ["superko", "analyze", "report", "play"]
    N2 = np.full(S * S + 1, -1, np.int32)
    N2[P(1, 0)] = 5                                                  # the forbidden move is the only child: a pass
    eng = ScriptedEngine(before, N2, Q)
    assert gtp.GTPEngine(engine=eng, superko="positional").parse_command("genmove b") == "= pass\n\n" and eng.moves[-1] == (S * S, 1)
    # extra empty: genmove is the engine's own
    eng = ScriptedEngine(CYCLE[:5], N, Q)
    e = gtp.GTPEngine(engine=eng, superko="positional")
    assert e.parse_command("genmove w") == "= E1\n\n" and [c[0] for c in eng.calls] == ["superko", "genmove"]
