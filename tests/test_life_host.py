"""CPU: the host side of unconditional life -- the accessors of life.Life, records.RecordSet.life, the flags of `review --life`,
the lines of `records --life` and GTP's `sgo-life` -- on the fake replay object with the model behind it
(tests/fake_life_records.py) and on a scripted engine; no GPU, no library."""
import io

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import life as life_mod
from sejonggo_amd.sgfload import SgfGame
from tests import life_cases as LC
from tests import life_model as M
from tests.fake_life_records import LifeRecords

S = 5
P = lambda x, y: y * S + x                                                               # noqa: E731

# the settled 5x5 board of tests/life_cases.py stone by stone, black's (2,4) last; then white fills its own eye (4,0) -- a move
# inside settled territory on a decided board -- and black takes the nine white stones at (4,2)
_B, _W = LC.diagram(S, LC.SETTLED)
SETUP = [(a, 1) for a in _B if a != P(2, 4)] + [(a, -1) for a in _W]
PLAY = [(P(2, 4), 1), (P(4, 0), -1), (P(4, 2), 1)]
SETTLED_GAME = SETUP + PLAY
SETTLED_TEXT = "bBBWw\nBBBWW\nbBBWw\nBBBWW\nBBBWW\nsettled 25/25 black 15 white 10"


def review_sgf():
    L = "abcde"
    pt = lambda a: "[%s]" % (L[a % S] + L[a // S])                                       # noqa: E731
    return "(;FF[4]SZ[5]KM[5.5]AB%sAW%s" % ("".join(pt(a) for a, c in SETUP if c > 0), "".join(pt(a) for a, c in SETUP if c < 0)) + \
        "".join(";%s%s" % ("B" if c > 0 else "W", pt(a)) for a, c in PLAY) + ")"


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=LifeRecords(S, 4, 64))


def test_life_accessors():
    names, recs = LC.case_records(S)
    m = LC.case_model(S)
    k, d = names.index("settled_sw"), names.index("dead_stone_cb")
    v = life_mod.Life(S, m["sets"], m["counts"])
    assert len(v) == len(names)
    assert v.alive(k, 1) == sorted(_B) and v.alive(k, -1) == sorted(_W)
    assert v.territory(k, 1) == [P(0, 0), P(0, 2)] and v.territory(k, -1) == [P(4, 0), P(4, 2)]
    assert v.safe(k, -1) == sorted(_W + [P(4, 0), P(4, 2)])
    assert v.unsettled(k) == 0 and v.settled(k) and v.margin(k) == 5 and v.n_dead(k, 1) == 0
    # colours swapped: white is alive around a black stone on the corner point
    black, white, _ = M.record_stones(S, recs[d])
    stones = np.zeros(S * S, np.int8)
    stones[black], stones[white] = 1, -1
    assert v.dead(d, 1, stones) == [0] and v.n_dead(d, 1) == 1 and v.dead(d, -1, stones) == [] and v.n_dead(d, -1) == 0
    assert v.territory(d, -1) == [0, 1, 5, P(3, 1)] and not v.settled(d) and v.margin(d) == -15 and v.unsettled(d) == 10
    assert life_mod.format_board(v, k) == SETTLED_TEXT
    assert life_mod.format_board(v, d).split("\n") == ["wwWWW", "wWWwW", "WWWWW", ".....", ".....", "settled 15/25 black 0 white 15"]
    e = names.index("empty_sb")
    assert life_mod.format_board(v, e).split("\n") == ["....."] * 5 + ["settled 0/25 black 0 white 0"]


def test_record_set_life_rows():
    game = _game(SETTLED_GAME)
    rs = _set(game)
    chunks = list(rs.life(stones=True))
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "life", "stones"]
    ch = chunks[0]
    v, n = ch.life, len(game.moves)
    assert v.sets.shape == (n + 1, 4, 1) and v.counts.shape == (n + 1, 8) and ch.stones.shape == (n + 1, S * S)
    assert v.counts[0].tolist() == [0, 0, 0, 0, 0, 0, 25, 0]
    # row ch.index[e] is the position before entry e, row + 1 the one after it
    e = len(SETUP)
    r = int(ch.index[e])
    assert v.unsettled(r) == 1 and v.settled(r + 1) and v.margin(r + 1) == 5
    assert v.counts[r + 2].tolist() == [13, 0, 2, 0, 0, 0, 10, 15]                    # white filled its eye: not alive any more
    # black took the white stones; the emptied side is open board beside the wall, and the lone capturing stone is not alive
    assert v.counts[r + 3].tolist() == [13, 0, 2, 0, 0, 0, 10, 15] and not (ch.stones[r + 3] == -1).any()
    # a refused entry: the records behind it give the zero row
    rs2 = _set(_game(SETUP + [(P(1, 1), -1), (P(4, 0), 1)]))
    ch2 = next(rs2.life())
    assert ch2.status[0] != 0 and ch2.life.unsettled(len(SETUP)) == 1 and not ch2.life.counts[len(SETUP) + 1:].any()
    assert not ch2.life.sets[len(SETUP) + 1:].any()


def test_review_life_flags():
    game = _game(SETTLED_GAME, n_setup=len(SETUP))
    found = review.life_rows(game, _set(game))
    assert found == {1: {"settled": 24, "black": 14, "white": 10, "flags": []},
                     2: {"settled": 25, "black": 15, "white": 10, "flags": ["inside", "decided"]},
                     3: {"settled": 15, "black": 15, "white": 0, "flags": []}}
    rows = [{"move_number": m, "colour": "B", "played": "A1", "played_share": 0.5, "played_mean": 0.1, "best": "B2", "best_mean": 0.2,
             "top": [{"pv": ["B2", "C3"]}]} for m in (1, 2, 3, 9)]
    plain = [review.format_row(dict(r)) for r in rows]
    review.add_life(rows, game, record_set=_set(game))
    assert [r.get("life_flags") for r in rows] == [[], ["inside", "decided"], [], None]
    assert rows[1]["life"] == {"settled": 25, "black": 15, "white": 10} and "life" not in rows[3]
    text = [review.format_row(r) for r in rows]
    assert text == [plain[0], plain[1] + "  | inside decided", plain[2], plain[3]]
    rows[1]["tactics"] = ["missed"]
    assert review.format_row(rows[1]) == plain[1] + "  | missed inside decided"        # beside the tactics flags
    # `decided` is given once: a second settled position is not flagged again, and a pass is never `inside`
    again = _game(SETUP + [PLAY[0], (S * S, -1), (S * S, 1), (P(0, 0), -1)], n_setup=len(SETUP))
    flags = {m: d["flags"] for m, d in review.life_rows(again, _set(again)).items()}
    assert flags == {1: [], 2: ["decided"], 3: [], 4: ["inside"]}


def test_review_flags_logic():
    names, recs = LC.case_records(S)
    m = LC.case_model(S)
    v = life_mod.Life(S, m["sets"], m["counts"])
    k, w = names.index("settled_sb"), names.index("wall_sb")
    f = lambda action, row, decided=False: life_mod.review_flags(S, action, v, row, decided)   # noqa: E731
    assert f(P(0, 0), k) == ["inside", "decided"] and f(P(4, 2), k, True) == ["inside"]
    assert f(P(1, 1), k, True) == [] and f(S * S, k) == ["decided"]                    # on a stone's point (refused anyway); a pass
    assert f(P(0, 3), w) == ["inside"] and f(P(0, 0), w) == []                         # the wall's eye; the open board beside it


def test_records_life_lines(tmp_path, monkeypatch):
    (tmp_path / "settled.sgf").write_text(review_sgf())
    (tmp_path / "open.sgf").write_text("(;FF[4]SZ[5]KM[5.5];B[cc];W[bb];B[])")
    monkeypatch.setattr(R, "DeviceRecords", LifeRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "5", "--life"], out=out) == 0
    lines = [l for l in out.getvalue().split("\n") if l.startswith("life ")]
    # black's ninth set-up stone closes its second eye; after the last move black has taken white off and ten points lie open
    assert sorted(lines) == ["life open plies 3 first_alive - unsettled 25",
                             "life settled plies %d first_alive 9 unsettled 10" % len(SETTLED_GAME)]
    # the same figures from the generator, for a record the replay cuts short
    rs = _set(_game(SETUP + [(P(1, 1), -1), (P(4, 0), 1)]), "cut")
    assert R.life_lines(rs) == [{"name": "cut", "plies": len(SETUP), "first_alive": 9, "unsettled": 1}]


class LifeEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `life` serves the model's row of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, size, case):
        names, recs = LC.case_records(size)
        m = M.life(size, recs[names.index(case)][None])
        self.view = life_mod.Life(size, m["sets"], m["counts"])

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def life(self):
        return self.view


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_life(conf5):
    e = gtp.GTPEngine(engine=LifeEngine(S, "settled_sb"))
    assert e.parse_command("known_command sgo-life") == "= true\n\n" and "sgo-life" in e.parse_command("list_commands").split()
    assert e.parse_command("sgo-life") == "= " + SETTLED_TEXT + "\n\n"
    assert e.parse_command("sgo_life") == e.parse_command("sgo-life")
    e = gtp.GTPEngine(engine=LifeEngine(S, "wall_cw"))
    assert e.parse_command("sgo-life") == "= .....\n.....\nWWWWW\nwWwWW\nWWWWW\nsettled 15/25 black 0 white 15\n\n"
    for name in ("final_score", "final_status_list", "sgo-ownership"):                  # untouched: they need the rollouts
        assert e.parse_command(name) == "? not supported\n\n"

    class Host(object):
        """the host engine's surface: no load, no life"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-life") == "? not supported\n\n"
