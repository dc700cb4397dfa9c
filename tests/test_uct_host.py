"""CPU: the Python layers above the playout-tree-search kernel (uct.py, records.py, review.py and its `--uct`, gtp.py) on a fake backend
that serves the model's rows (tests/fake_uct_records.py): the symbols and the argument checks, the result object, the text of
`review --uct` without a net, GTP's `sgo-uct` and the `--player uct` option on a scripted engine -- genmove through the slot's play, the
superko filter, the refusals of what would call the net, and a start that never touches the model loader."""
import io

import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review, rollout, uct
from tests import playout_model as PM
from tests import uct_model as UM
from tests.fake_uct_records import UctRecords

S = 5
N = S * S
P = lambda x, y: y * S + x                                                               # noqa: E731
GAME = [(P(1, 1), 1), (P(3, 3), -1), (P(2, 2), 1), (N, -1), (P(1, 3), 1)]
OK = dict(trees=2, sims=8, rules=1, max_plies=0, komi2=0, expand_at=2, rave_equiv=64, prior=4, max_nodes=9)


def test_symbols_are_bound_and_arguments_checked():
    from sejonggo_amd import _lib
    assert {"sgo_uct_workspace", "sgo_uct_dev", "sgo_uct", "sgo_session_uct"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert len(lib.sgo_uct_dev.argtypes) == 25 and len(lib.sgo_uct.argtypes) == 22 and len(lib.sgo_session_uct.argtypes) == 21
    assert (uct.MAX_TREES, uct.MAX_SIMS, uct.MAX_DEPTH) == (UM.MAX_TREES, UM.MAX_SIMS, UM.MAX_DEPTH) and uct.RULES == 1
    check = lambda **kw: uct.check_args(S, *[dict(OK, **kw)[k] for k in ("trees", "sims", "rules", "max_plies", "komi2", "expand_at", "rave_equiv",   # noqa: E731
                                                                         "prior", "max_nodes")])
    check()
    check(trees=uct.MAX_TREES, sims=uct.MAX_SIMS, max_plies=4 * N, komi2=-4 * N, expand_at=0, rave_equiv=1 << 20, prior=1024, max_nodes=uct.MAX_SIMS + 1)
    for bad in (dict(trees=0), dict(trees=uct.MAX_TREES + 1), dict(sims=0), dict(sims=uct.MAX_SIMS + 1), dict(rules=2), dict(max_plies=4 * N + 1),
                dict(komi2=4 * N + 1), dict(expand_at=-1), dict(expand_at=9), dict(rave_equiv=-1), dict(rave_equiv=(1 << 20) + 1), dict(prior=-1),
                dict(prior=1025), dict(max_nodes=0), dict(max_nodes=10)):
        with pytest.raises(ValueError):
            check(**bad)
    assert uct.komi2_of(7.5) == 15 and uct.komi2_of(-0.5) == -1 and uct.komi2_of(0) == 0
    with pytest.raises(ValueError):
        uct.komi2_of(0.3)
    # the default settings pass their own checks, and the docstring says what they are
    check(trees=uct.TREES, sims=uct.SIMS, expand_at=uct.EXPAND_AT, rave_equiv=uct.RAVE_EQUIV, prior=uct.PRIOR, max_nodes=uct.SIMS + 1)
    assert "UNTUNED" in uct.__doc__ and "untuned" in uct.search.__doc__


def _model_result(recs, **kw):
    m = UM.search(S, recs, None, trees=2, sims=12, seed=3, komi2=1, **kw)
    return uct.Search(S, m["visits"], m["wins2"], m["rave"], m["own"], m["sums"], m["info"], m["trace"]), m


def test_result_object():
    recs = np.stack([PM.build_record(S, [P(1, 1), P(2, 1)], [P(3, 3)], False), PM.build_record(S, [P(1, 1)], [P(3, 3), P(3, 2)], True)])
    v, m = _model_result(recs)
    assert len(v) == 2
    for i in range(2):
        b = v.best(i)
        assert b == int(m["info"][i, 3]) and v.ranked(i)[0] == b
        assert abs(v.winrate(i) - m["wins2"][i, b] / (2.0 * m["visits"][i, b])) < 1e-12 and v.winrate(i, 0) == 0.5      # an occupied point: never visited
        t = v.move_table(i)
        assert [r[0] for r in t] == v.ranked(i) and sum(r[1] for r in t) == 24 and t[0][0] == b
        assert all(r[1] == m["visits"][i, r[0]] and r[3] == m["rave"][i, 0, r[0]] for r in t) and len(v.move_table(i, 3)) == 3
        assert [r[1] for r in t] == sorted((r[1] for r in t), reverse=True)
        assert v.ranked(i, lambda a: a != b)[0] != b
        row = v.row(i)
        assert set(rollout.SUMS) <= set(row) and row["rollouts"] == 24 and (row["black_own"] == m["own"][i, 0]).all()
        assert rollout.final_score(row, 0.5)[0] in "BW"
        own = v.ownership(i)
        assert own.shape == (N,) and (abs(own) <= 1).all() and abs(own.sum() - m["sums"][i, 3] / 24.0) < 1e-9
        text = uct.format_moves(v, i, 4, str).split("\n")
        assert text[0] == "best %d winrate %.3f simulations 24 nodes %d depth %d" % (b, v.winrate(i), m["info"][i, 0], m["info"][i, 1])
        assert len(text) == 5 and text[1].split()[:2] == [str(b), str(m["visits"][i, b])]
    zero = uct.Search(S, np.zeros((1, N + 1)), np.zeros((1, N + 1)), None, None, np.zeros((1, 8)), [[0, 0, 0, -1]])
    assert zero.best(0) is None and zero.winrate(0) == 0.5 and zero.move_table(0) == [] and zero.ranked(0) == []
    assert uct.format_moves(zero, 0, 3, str) == "best none winrate 0.500 simulations 0 nodes 0 depth 0"
    for call in (zero.ownership, zero.row):
        with pytest.raises(ValueError):
            call(0)


def test_review_uct_text_without_a_net(tmp_path, monkeypatch):
    L = "abcde"
    path = tmp_path / "game.sgf"
    path.write_text("(;FF[4]SZ[5]KM[5.5]" + "".join(";%s[%s]" % ("B" if c > 0 else "W", "" if a == N else L[a % S] + L[a // S]) for a, c in GAME) + ")")
    monkeypatch.setattr(R, "DeviceRecords", UctRecords)
    monkeypatch.setattr(review, "_net", lambda *a: pytest.fail("a net was asked for"))
    out = io.StringIO()
    assert review.main([str(path), "--uct", "2", "6"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == len(GAME)
    from tests import records_model
    recs = records_model.replay(S, [([a for a, _ in GAME], [c for _, c in GAME])])["records"]
    m = UM.search(S, recs, None, trees=2, sims=6, seed=0, rules=1, komi2=11, expand_at=2, rave_equiv=uct.RAVE_EQUIV, prior=uct.PRIOR)
    for j, (a, c) in enumerate(GAME):
        b = int(m["info"][j, 3])
        text = review.vertex(b, S)
        flag = "uct-agrees" if b == a else "uct-prefers " + text
        assert lines[j].endswith("| uct %s %.3f  | %s" % (text, m["wins2"][j, b] / (2.0 * m["visits"][j, b]), flag)), (j, lines[j])
    with pytest.raises(SystemExit):
        review.main([str(path), "--uct", "2"], out=io.StringIO())


class ScriptedEngine(object):
    """what GTPEngine asks of the device engine for the uct player: the model on the position the played moves give"""
    size = S

    def __init__(self):
        self.asked, self.played, self.forbidden = [], [], []
        self.model = type("M", (), {"name": "none"})()
        self.stones = ([P(1, 1), P(2, 1), P(1, 2)], [P(3, 3), P(3, 2)])
        self.to_move = -1

    @property
    def board(self):
        b = np.zeros((1, S, S, 17), np.int32)
        b[..., 16] = self.to_move
        return b

    def load(self, moves, colors=None, n_setup=0):
        raise NotImplementedError

    def uct(self, trees=None, sims=None, komi=0.0, seed=0, rules=1):
        self.asked.append((trees, sims, komi))
        rec = PM.build_record(S, self.stones[0], self.stones[1], self.to_move < 0)
        m = UM.search(S, rec[None], None, trees=trees or 2, sims=sims or 12, seed=seed, rules=rules, komi2=uct.komi2_of(komi))
        return uct.Search(S, m["visits"], m["wins2"], m["rave"], m["own"], m["sums"], m["info"], white_to_play=[self.to_move < 0])

    def play(self, color, x, y):
        self.played.append((color, x, y))
        self.to_move = -self.to_move
        return self.board, color

    def superko(self, rule):
        forbidden = self.forbidden
        return type("K", (), {"extra": lambda self, i: [(a, 1) for a in forbidden], "played": lambda self, i, a: [a in forbidden]})()

    def playouts(self, per_row=None, rules=1, seed=0):
        from sejonggo_amd import playout as po
        m = PM.playouts(S, PM.build_record(S, self.stones[0], self.stones[1], True)[None], None, 8, seed, rules, 0)
        return po.Playouts(S, m["own"], m["amaf"], m["sums"], [True]), np.zeros((S, S), np.int8)

    def analyze(self, sims=None):
        raise AssertionError("the net's search was asked for")

    def report(self, top=5, depth=8):
        raise AssertionError("the net's search was asked for")

    def genmove(self, color):
        raise AssertionError("the net's genmove was asked for")

    def rollouts(self, per_src=None, seed=0):
        raise AssertionError("policy rollouts were asked for")

    def close(self):
        pass


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_uct_text(conf5):
    dev = ScriptedEngine()
    e = gtp.GTPEngine(engine=dev)                                    # the command is there without --player uct
    e.parse_command("komi 1.5")
    v = dev.uct(3, 10, 1.5)
    dev.asked = []
    assert e.parse_command("sgo-uct trees 3 sims 10") == "= " + uct.format_moves(v, 0, 10, e._vertex) + "\n\n" and dev.asked == [(3, 10, 1.5)]
    assert e.parse_command("sgo-uct sims 4").startswith("= best ") and dev.asked[-1] == (None, 4, 1.5)
    assert e.parse_command("sgo-uct").startswith("= best ") and dev.asked[-1] == (None, None, 1.5)
    for bad in ("sgo-uct 3", "sgo-uct trees", "sgo-uct trees 0", "sgo-uct sims %d" % (uct.MAX_SIMS + 1), "sgo-uct plies 3", "sgo-uct trees x"):
        assert e.parse_command(bad) == "? syntax error\n\n", bad
    assert "sgo-uct" in e.parse_command("list_commands").split() and e.parse_command("known_command sgo-uct") == "= true\n\n"
    # the net player is as it was: genmove goes to the engine's own genmove
    with pytest.raises(AssertionError):
        e.parse_command("genmove w")


def test_gtp_player_uct(conf5):
    dev = ScriptedEngine()
    e = gtp.GTPEngine(engine=dev, player="uct", uct_trees=2, uct_sims=12)
    assert e.score == "playouts"
    v = dev.uct(2, 12, 0.0)
    best = v.best(0)
    assert e.parse_command("genmove w") == "= " + e._vertex(best) + "\n\n"
    assert dev.played == [(-1, best % S, best // S)] and dev.asked[-1] == (2, 12, 0.0)
    assert e.parse_command("genmove w").startswith("? genmove for the side that is not to move")
    # with superko the best child that is not a repeat is played
    dev = ScriptedEngine()
    e = gtp.GTPEngine(engine=dev, player="uct", uct_trees=2, uct_sims=12, superko="positional")
    order = v.ranked(0)
    dev.forbidden = order[:2]
    assert e.parse_command("genmove w") == "= " + e._vertex(order[2]) + "\n\n"
    dev.to_move, dev.forbidden = -1, order
    assert e.parse_command("genmove w") == "= pass\n\n" and dev.played[-1] == (-1, 0, S)
    # what would call the net says so; the scoring commands stand on playouts
    for cmd in ("sgo-analyze", "sgo-analyze 16"):
        r = e.parse_command(cmd)
        assert r.startswith("? ") and "--player uct" in r and "without a model" in r, r
    assert e.parse_command("final_score").startswith("= ") and len(e.parse_command("sgo-ownership").strip("= \n").split("\n")) == S
    e = gtp.GTPEngine(engine=dev, player="uct", score="rollouts")
    assert "without a model" in e.parse_command("final_score") and "without a model" in e.parse_command("final_status_list dead")
    with pytest.raises(ValueError):
        gtp.GTPEngine(engine=None, player="uct")
    with pytest.raises(ValueError):
        gtp.GTPEngine(engine=dev, player="random")


def test_gtp_player_uct_starts_without_a_model(conf5, monkeypatch, capsys):
    made = []

    def fake_device_engine(sims, **kw):
        made.append(kw)
        return ScriptedEngine()
    monkeypatch.setattr(gtp, "DeviceSejongGoEngine", fake_device_engine)
    monkeypatch.setattr(gtp, "get_model", lambda *a, **k: pytest.fail("the model loader was called"))
    monkeypatch.setattr(gtp, "init_predicting_workers", lambda *a, **k: pytest.fail("a predicting worker was started"))
    out = io.StringIO()
    gtp.main(inp=["genmove w\n", "sgo-analyze\n", "quit\n"], out=out, device=True, player="uct", uct_trees=2, uct_sims=6)
    replies = out.getvalue().split("\n\n")
    assert replies[0].startswith("= ") and replies[1].startswith("? ") and "without a model" in replies[1]
    assert made[0]["net"] is not None and made[0]["net"].name == "uniform_stub" and made[0]["size"] == S
    # without the option nothing changes: no net is handed over, the device engine loads its own
    gtp.main(inp=["quit\n"], out=io.StringIO(), device=True)
    assert made[1]["net"] is None
    assert gtp.main(inp=[], device=False, player="uct") == 2 and "--device" in capsys.readouterr().err
    assert gtp._cli(["--player", "uct"]) == 2
