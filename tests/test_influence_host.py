"""CPU: the host side of the influence estimate -- the accessors of influence.Influence, the text of format_board,
records.RecordSet.influence, the fields and the summary of `review --influence`, the buckets of `records --influence`, GTP's
`sgo-influence` / `sgo-estimate`, and the argument refusals of influence() -- on the fake replay object with the model behind it
(tests/fake_influence_records.py) and on a scripted engine; no GPU, no library."""
import io

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import influence as inf
from sejonggo_amd.sgfload import SgfGame
from tests import influence_cases as IC
from tests import influence_model as M
from tests import life_cases as LC
from tests.fake_influence_records import InfluenceRecords
from tests.test_life_host import PLAY, SETTLED_GAME, SETUP, review_sgf

S = 5
P = lambda x, y: y * S + x                                                               # noqa: E731


def _view(triple=M.TERRITORY):
    m = IC.case_model(S, triple)
    return IC.case_records(S)[0], inf.Influence(S, m["values"], m["sets"], m["counts"])


def _stones(name):
    names, recs, _ = IC.case_records(S)
    black, white, _ = M.record_stones(S, recs[names.index(name)])
    st = np.zeros(S * S, np.int8)
    st[black], st[white] = 1, -1
    return st


def _game(entries, n_setup=0, komi=5.5):
    return SgfGame(S, komi, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game, name="game"):
    rec = R.Record(name, S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=InfluenceRecords(S, 4, 64))


def test_presets_are_the_classical_triples():
    assert inf.PRESETS == {"territory": {"dilate": 5, "erode_moyo": 10, "erode_terr": 21},
                           "area": {"dilate": 4, "erode_moyo": 0, "erode_terr": 0}}
    assert (inf.MAX_DILATE, inf.MAX_ERODE) == (M.MAX_DILATE, M.MAX_ERODE) == (8, 31)


def test_influence_accessors():
    names, v = _view()
    assert len(v) == len(names) and v.values.shape == (len(names), 25) and v.values.dtype == np.int16
    k = names.index("corners_cw")                            # white on (1, 1), black on (3, 3)
    assert v.territory(k, -1) == [0] and v.territory(k, 1) == [24]
    assert v.moyo(k, -1) == [0, 1, 5] and v.moyo(k, 1) == [P(4, 3), P(3, 4), 24]
    assert v.live(k, 1) == 1 and v.live(k, -1) == 1 and v.neutral(k) == 21 and v.margin(k) == 0
    assert v.estimate(k, 0.5) == -0.5 and v.estimate(k) == 0
    c = names.index("lone_centre_sb")
    assert v.territory(c, 1) == [a for a in range(25) if a != 12] and v.margin(c) == 25 and v.neutral(c) == 0
    # the lifted white stone at (1, 0) is black's territory; black's at (3, 4) white's
    d = names.index("dead_inside_sb")
    assert P(1, 0) in v.territory(d, 1) and P(3, 4) in v.territory(d, -1) and v.live(d, 1) == 5 and v.live(d, -1) == 5


def test_format_board_text():
    names, v = _view()
    f = lambda name, komi=0.5: inf.format_board(v, _stones(name), names.index(name), komi).split("\n")   # noqa: E731
    assert f("corners_cw") == ["w-...", "-O...", ".....", "...X+", "...+b", "estimate W+0.5 black 2 white 2 neutral 21 komi 0.5"]
    assert f("corners_cw", 0.0)[-1] == "estimate 0 black 2 white 2 neutral 21 komi 0.0"
    assert f("walls_sb") == ["bbbbb", "XXXXX", ".....", "OOOOO", "wwwww", "estimate W+0.5 black 10 white 10 neutral 5 komi 0.5"]
    # lifted stones are drawn as the territory they lie in
    assert f("dead_inside_sb") == ["bbbbb", "bbbbb", "XXXXX", "OOOOO", "wwwww", "estimate B+4.5 black 15 white 10 neutral 0 komi 0.5"]
    assert f("empty_sb", 7.5) == ["....."] * 5 + ["estimate W+7.5 black 0 white 0 neutral 25 komi 7.5"]
    names, area = _view(M.AREA)
    text = inf.format_board(area, _stones("corners_cw"), names.index("corners_cw"), 0.5).split("\n")
    assert text == ["wwww.", "wOw.b", "ww.bb", "w.bXb", ".bbbb", "estimate W+0.5 black 10 white 10 neutral 5 komi 0.5"]
    assert inf.score_text(3) == "B+3.0" and inf.score_text(-0.5) == "W+0.5" and inf.score_text(0) == "0"


def test_record_set_influence_rows():
    game = _game(SETTLED_GAME)
    rs = _set(game)
    chunks = list(rs.influence(stones=True))
    assert [c[0] for c in rs.backend.calls] == ["replay", "influence", "stones"]
    assert rs.backend.calls[1][2:] == ("life", (5, 10, 21))
    ch = chunks[0]
    v, n = ch.influence, len(game.moves)
    assert v.values.shape == (n + 1, 25) and v.sets.shape == (n + 1, 4, 1) and v.counts.shape == (n + 1, 8)
    assert v.counts[0].tolist() == [0, 0, 0, 0, 0, 0, 25, 0]
    r = int(ch.index[len(SETUP)])                           # the position before black's last stone
    assert inf.format_board(v, ch.stones[r], r, 5.5).split("\n") == [
        "bXXOw", "XXXOO", "bXXOw", "XXXOO", "XX.OO", "estimate W+1.5 black 14 white 10 neutral 1 komi 5.5"]
    assert v.counts[r + 1].tolist() == [2, 2, 2, 2, 13, 8, 0, 5]
    # black took the nine white stones: the whole board is black's
    assert v.counts[r + 3].tolist() == [11, 0, 11, 0, 14, 0, 0, 25]
    # the other presets and dead=None reach the backend as given
    rs = _set(game)
    next(rs.influence(dead=None, **inf.PRESETS["area"]))
    assert rs.backend.calls[1][2:] == (None, (4, 0, 0))
    # a refused entry: the records behind it give the zero row
    rs2 = _set(_game(SETUP + [(P(1, 1), -1), (P(4, 0), 1)]))
    ch2 = next(rs2.influence())
    assert ch2.status[0] != 0 and ch2.influence.counts[len(SETUP)].any() and not ch2.influence.counts[len(SETUP) + 1:].any()
    assert not ch2.influence.values[len(SETUP) + 1:].any() and not ch2.influence.sets[len(SETUP) + 1:].any()


def test_dead_life_lifts_the_proved_dead_stones():
    """a white stone on black's corner point, inside a living black group: lifted with dead="life", standing without"""
    b, w = LC.diagram(S, ["O.XXX", ".XX.X", "XXXXX"])
    game = _game([(a, 1) for a in b] + [(a, -1) for a in w])
    last = len(game.moves)
    with_life = next(_set(game).influence(dead="life")).influence
    without = next(_set(game).influence(dead=None)).influence
    assert with_life.live(last, -1) == 0 and without.live(last, -1) == 1
    assert 0 in with_life.territory(last, 1) and 0 not in without.territory(last, 1)
    # lifted, the corner is black's to the last point; standing, the stone keeps its point and the two beside it stay neutral
    assert with_life.margin(last) == 25 and without.margin(last) == 21 and without.neutral(last) == 2


def test_review_influence_fields_and_summary():
    game = _game(SETTLED_GAME, n_setup=len(SETUP))
    found = review.influence_rows(game, _set(game), 5.5)
    assert found == {1: {"estimate": -1.5, "gain": 1}, 2: {"estimate": -0.5, "gain": 0}, 3: {"estimate": -0.5, "gain": 20}}
    rows = review.bare_rows(game)
    assert rows == [{"move_number": 1, "colour": "B", "played": "C1"}, {"move_number": 2, "colour": "W", "played": "E5"},
                    {"move_number": 3, "colour": "B", "played": "E3"}]
    rows.append({"move_number": 9, "colour": "B", "played": "A1"})
    review.add_influence(rows, game, record_set=_set(game))                              # komi None: the record's 5.5
    assert [(r.get("estimate"), r.get("gain")) for r in rows] == [(-1.5, 1), (-0.5, 0), (-0.5, 20), (None, None)]
    assert [review.format_row(r) for r in rows] == ["   1 B C1    | estimate W+1.5 gain +1", "   2 W E5    | estimate W+0.5 gain +0",
                                                    "   3 B E3    | estimate W+0.5 gain +20", "   9 B A1  "]
    assert review.influence_summary(rows) == "influence: highest gain 3 (+20) 1 (+1) 2 (+0); lowest gain 2 (+0) 1 (+1) 3 (+20)"
    # beside the fields of a searched row and its flags
    full = {"move_number": 2, "colour": "W", "played": "E5", "played_share": 0.5, "played_mean": 0.1, "best": "B2", "best_mean": 0.2,
            "top": [{"pv": ["B2", "C3"]}]}
    plain = review.format_row(dict(full))
    full.update(estimate=-0.5, gain=0, life_flags=["inside"])
    assert review.format_row(full) == plain + "  | estimate W+0.5 gain +0  | inside"
    # the gain is the mover's: white's move that loses black two points gains white two
    v = inf.Influence(S, np.zeros((2, 25)), np.zeros((2, 4, 1)), [[0, 0, 0, 0, 0, 0, 25, 3], [0, 0, 0, 0, 0, 0, 25, 1]])
    assert inf.review_fields(v, 0, 1, -1, 0.5) == {"estimate": 2.5, "gain": 2}
    assert inf.review_fields(v, 0, None, 1, 0.0) == {"estimate": 3.0, "gain": None}
    assert inf.review_summary([(1, 5), (2, None), (3, -4), (4, 5), (5, 0), (6, 1)]) == ([1, 4, 6], [3, 5, 6])


def test_review_main_without_a_net(tmp_path, monkeypatch):
    """`review game.sgf --influence` alone searches nothing and loads no net"""
    path = tmp_path / "game.sgf"
    path.write_text(review_sgf())
    monkeypatch.setattr(R, "DeviceRecords", InfluenceRecords)
    monkeypatch.setattr(review, "_net", lambda *a: pytest.fail("a net was asked for"))
    out = io.StringIO()
    assert review.main([str(path), "--influence", "--json", str(tmp_path / "doc.json")], out=out) == 0
    assert out.getvalue().split("\n") == ["   1 B C1    | estimate W+1.5 gain +1", "   2 W E5    | estimate W+0.5 gain +0",
                                          "   3 B E3    | estimate W+0.5 gain +20",
                                          "influence: highest gain 3 (+20) 1 (+1) 2 (+0); lowest gain 2 (+0) 1 (+1) 3 (+20)", ""]
    import json
    doc = json.loads((tmp_path / "doc.json").read_text())
    assert doc["net"] is None and doc["sims"] == 0 and [p["gain"] for p in doc["positions"]] == [1, 0, 20]


def test_records_influence_buckets(tmp_path, monkeypatch):
    (tmp_path / "settled.sgf").write_text(review_sgf())
    (tmp_path / "open.sgf").write_text("(;FF[4]SZ[5]KM[5.5];B[cc];W[bb];B[])")
    monkeypatch.setattr(R, "DeviceRecords", InfluenceRecords)
    out = io.StringIO()
    assert R.main([str(tmp_path), "--size", "5", "--influence"], out=out) == 0
    lines = [l for l in out.getvalue().split("\n") if l.startswith("influence ")]
    assert len(lines) == 4 and lines[0].startswith("influence 0-19 positions 24 ") and lines[1].startswith("influence 20-39 positions 4 ")
    assert sorted(lines[2:]) == ["influence open plies 3 estimate %s" % inf.score_text(_open_margin()),
                                 "influence settled plies %d estimate B+25.0" % len(SETTLED_GAME)]
    game = _game(SETTLED_GAME)
    t = R.influence_table(_set(game), 20)
    assert [b["positions"] for b in t["buckets"]] == [20, 4] and t["games"] == [{"name": "game", "plies": 23, "margin": 25}]
    # every figure against the model's rows, position by position
    want = next(_set(game).influence()).influence.counts.astype(np.int64)
    for b, rows in zip(t["buckets"], (want[:20], want[20:])):
        assert b["abs_margin"] == np.abs(rows[:, 7]).mean() and b["neutral"] == rows[:, 6].mean()
        assert b["moyo_beyond_black"] == (rows[:, 2] - rows[:, 0]).mean() and b["moyo_beyond_white"] == (rows[:, 3] - rows[:, 1]).mean()
    cut = _set(_game(SETUP + [(P(1, 1), -1), (P(4, 0), 1)]), "cut")
    assert R.influence_table(cut)["games"] == [{"name": "cut", "plies": len(SETUP), "margin": 4}]


def _open_margin():
    return M.bouzy(S, [P(2, 2)], [P(1, 1)])["counts"][7]


# ---- GTP -------------------------------------------------------------------------------------------------------------------------
class InfluenceEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `influence` serves the model's row of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, size, case):
        self.size, self.case, self.asked = size, case, []

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def influence(self, dead="life", dilate=5, erode_moyo=10, erode_terr=21):
        self.asked.append((dead, dilate, erode_moyo, erode_terr))
        names, recs, lift = IC.case_records(self.size)
        i = names.index(self.case)
        m = M.influence(self.size, recs[i:i + 1], None, lift[i:i + 1] if dead == "life" else None, dilate, erode_moyo, erode_terr)
        return inf.Influence(self.size, m["values"], m["sets"], m["counts"]), _stones(self.case)


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_influence_and_estimate(conf5):
    eng = InfluenceEngine(S, "dead_inside_sb")
    e = gtp.GTPEngine(engine=eng)
    for name in ("sgo-influence", "sgo-estimate"):
        assert e.parse_command("known_command " + name) == "= true\n\n" and name in e.parse_command("list_commands").split()
    e.parse_command("komi 0.5")
    assert e.parse_command("sgo-influence") == "= bbbbb\nbbbbb\nXXXXX\nOOOOO\nwwwww\nestimate B+4.5 black 15 white 10 neutral 0 komi 0.5\n\n"
    assert e.parse_command("sgo_influence") == e.parse_command("sgo-influence")
    assert e.parse_command("sgo-estimate") == "= B+4.5\n\n"
    # nodead: the white stone behind black's wall and the black one behind white's stand, and little is left of either territory
    text = e.parse_command("sgo-influence nodead")
    assert text == "= .O...\n....+\nXXXXX\nOOOOO\n-..X.\nestimate W+0.5 black 6 white 6 neutral 13 komi 0.5\n\n"
    assert e.parse_command("sgo-estimate nodead") == "= W+0.5\n\n"
    assert e.parse_command("sgo-influence area nodead").split("\n")[:2] == ["= wOw.b", "b.bbb"]
    assert e.parse_command("sgo-influence area nodead").split("\n")[:5] == e.parse_command("sgo-influence nodead area").split("\n")[:5]
    assert eng.asked[0] == ("life", 5, 10, 21) and eng.asked[-1] == (None, 4, 0, 0) and ("life", 4, 0, 0) not in eng.asked
    assert e.parse_command("sgo-estimate area") == "= B+4.5\n\n" and eng.asked[-1] == ("life", 4, 0, 0)
    for bad in ("sgo-influence moyo", "sgo-influence area area", "sgo-influence nodead nodead", "sgo-estimate 5"):
        assert e.parse_command(bad) == "? syntax error\n\n"
    e = gtp.GTPEngine(engine=InfluenceEngine(S, "corners_cw"))
    assert e.parse_command("sgo-estimate") == "= 0\n\n"
    for name in ("final_score", "sgo-ownership", "sgo-life"):                            # untouched: this engine has none of them
        assert e.parse_command(name) == "? not supported\n\n"

    class Host(object):
        """the host engine's surface: no load, no influence"""
        model = type("N", (), {"name": "x"})()

    for name in ("sgo-influence", "sgo-estimate", "sgo-influence area"):
        assert gtp.GTPEngine(engine=Host()).parse_command(name) == "? not supported\n\n"


# ---- refusals of influence() -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", [(-1, 0, 0), (9, 0, 0), (5, -1, 21), (5, 10, 32), (5, 11, 10), (5, 32, 32), (2.5, 0, 0)])
def test_influence_refuses_bad_parameters_before_the_device(triple, monkeypatch):
    from sejonggo_amd import _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("the device was asked for"))
    recs = IC.case_records(S)[1]
    with pytest.raises(ValueError):
        inf.influence(S, recs, None, None, *triple)
    with pytest.raises(ValueError):
        inf.check_params(*triple)
    assert inf.check_params(8, 31, 31) == (8, 31, 31) and inf.check_params(0, 0, 0) == (0, 0, 0)
