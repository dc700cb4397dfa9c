"""CPU: the Python layers above the light-playout kernel (playout.py, records.py and its `--playouts`, review.py, gtp.py) on a fake backend that serves the model's
rows (tests/fake_playout_records.py): the result object, which rows RecordSet.playouts asks for, the text of `review --playouts` without a net, and GTP's two commands, the
`--score playouts` option and their refusals on a scripted engine."""
import numpy as np
import pytest

import io

from sejonggo_amd import gtp, playout as po, records as R, review, rollout
from tests import playout_model as PM
from tests.fake_playout_records import PlayoutRecords

S = 5
P = lambda x, y: y * S + x                                                               # noqa: E731
GAME = [(P(1, 1), 1), (P(3, 3), -1), (P(2, 2), 1), (S * S, -1), (P(1, 3), 1)]


def _record(name, entries):
    return R.Record(name, S, list(entries), [False] * len(entries), list(range(1, len(entries) + 1)), None)


def test_symbols_are_bound_and_arguments_checked():
    from sejonggo_amd import _lib
    from sejonggo_amd.solve import check_args as solve_check
    assert {"sgo_playout_dev", "sgo_playout", "sgo_session_playout"} <= set(_lib.SYMBOLS)
    assert po.RULES == 1 and po.MAX_PER_ROW == PM.MAX_PER_ROW and po.SUMS == PM.SUMS
    solve_check(po.RULES, 12, 4096, 16)                              # the default of solve.py is the default here
    for bad in (dict(per_row=0), dict(per_row=po.MAX_PER_ROW + 1), dict(rules=2), dict(max_plies=4 * S * S + 1)):
        kw = dict(dict(per_row=4, rules=1, max_plies=0), **bad)
        with pytest.raises(ValueError):
            po.check_args(S, kw["per_row"], kw["rules"], kw["max_plies"])
    po.check_args(S, po.MAX_PER_ROW, 0, 4 * S * S)


def _model_result(recs, per_row=8, **kw):
    m = PM.playouts(S, recs, None, per_row, 3, 1, 0, **kw)
    wtp = [bool(r.reshape(16, -1)[0, -1] >> 31) for r in recs]
    return po.Playouts(S, m["own"], m["amaf"], m["sums"], wtp), m


def test_result_object():
    recs = np.stack([PM.build_record(S, [P(1, 1), P(2, 1)], [P(3, 3)], False), PM.build_record(S, [P(1, 1)], [P(3, 3), P(3, 2)], True)])
    v, m = _model_result(recs)
    assert len(v) == 2
    for i in range(2):
        row = v.row(i)
        assert set(rollout.SUMS) <= set(row) and row["rollouts"] == 8 and (row["black_own"] == m["own"][i, 0]).all()
        assert rollout.final_score(row, 0.5)[0] in "BW" and set(rollout.stone_status(row, np.zeros(S * S, np.int8))) == {"alive", "dead", "seki"}
        assert abs(v.score_mean(i) - m["sums"][i, 3] / 8.0) < 1e-12 and v.capped_share(i) == m["sums"][i, 6] / 8.0
        assert abs(v.score_sd(i) ** 2 - (m["sums"][i, 4] / 8.0 - v.score_mean(i) ** 2)) < 1e-9
        own = v.ownership(i)
        assert own.shape == (S * S,) and (abs(own) <= 1).all() and abs(own.sum() - v.score_mean(i)) < 1e-9
        mv = v.move_values(i, 2)
        assert mv and all(c >= 2 for _, c, _ in mv) and [t[2] for t in mv] == sorted((t[2] for t in mv), reverse=True)
        assert all(m["amaf"][i, 0, a] == c and abs(m["amaf"][i, 1, a] / float(c) - mean) < 1e-12 for a, c, mean in mv)
        assert len(v.format_board(i).split("\n")) == S and "playouts 8" in po.format_summary(v, i)
        assert len(po.format_moves(v, i, 3, str).split("\n")) == min(3, len(v.move_values(i, 1)))
    zero = po.Playouts(S, np.zeros((1, 2, S * S)), None, np.zeros((1, 8)))
    assert zero.score_mean(0) == 0 and zero.score_sd(0) == 0 and zero.capped_share(0) == 0 and not zero.ownership(0).any()
    with pytest.raises(ValueError):
        zero.move_values(0)


def test_record_set_asks_for_every_record_once():
    cut = [(P(2, 2), 1), (P(2, 2), -1), (P(0, 0), 1)]                # the second entry lands on a stone
    rs = R.RecordSet([_record("game", GAME), _record("cut", cut)], S, backend=PlayoutRecords(S, 8, 64))
    chunks = list(rs.playouts(per_row=3, seed=9, rules=0, max_plies=20))
    assert len(chunks) == 1 and rs.refused == [("cut", -101, 1)]
    index, per_row, seed, rules, max_plies = rs.backend.asked[0]
    n0 = len(GAME) + 1
    assert index == list(range(n0)) + [n0, n0 + 1, -1, -1] and (per_row, seed, rules, max_plies) == (3, 9, 0, 20)
    ch = chunks[0]
    v = ch.playouts
    want = PM.playouts(S, rs.backend.last["records"], index, 3, 9, 0, 20)
    assert (v.own == want["own"]).all() and (v.amaf == want["amaf"]).all() and (v.sums == want["sums"]).all()
    assert ch.to_play.tolist() == [1, -1, 1, -1, 1, -1, 1, -1, 0, 0] and v.white_to_play.tolist() == [t < 0 for t in ch.to_play]
    assert not v.sums[n0 + 2].any() and v.count(0, "playouts") == 3
    with pytest.raises(ValueError):
        next(rs.playouts(per_row=0))


def test_review_playouts_text_without_a_net(tmp_path, monkeypatch):
    L = "abcde"
    path = tmp_path / "game.sgf"
    path.write_text("(;FF[4]SZ[5]KM[5.5]" + "".join(";%s[%s]" % ("B" if c > 0 else "W", "" if a == S * S else L[a % S] + L[a // S]) for a, c in GAME) + ")")
    monkeypatch.setattr(R, "DeviceRecords", PlayoutRecords)
    monkeypatch.setattr(review, "_net", lambda *a: pytest.fail("a net was asked for"))
    out = io.StringIO()
    assert review.main([str(path), "--playouts", "6"], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    assert len(lines) == len(GAME) + 1 and lines[-1].startswith("playouts (estimate): largest drops ")
    from tests import records_model
    recs = records_model.replay(S, [([a for a, _ in GAME], [c for _, c in GAME])])["records"]
    m = PM.playouts(S, recs, None, 6, 0, 1, 0)
    mean = m["sums"][:, 3] / 6.0
    for j, (a, c) in enumerate(GAME):
        sd = max(0.0, m["sums"][j, 4] / 6.0 - mean[j] ** 2) ** 0.5
        assert lines[j].endswith("| playouts %+.1f +- %.1f change %+.1f" % (mean[j], sd, (mean[j + 1] - mean[j]) * c)), (j, lines[j])
    drops = sorted(((mean[j + 1] - mean[j]) * c, j + 1) for j, (a, c) in enumerate(GAME) if (mean[j + 1] - mean[j]) * c < 0)[:3]
    assert [int(w) for w in lines[-1].split("drops ")[1].split() if w.isdigit()] == [mv for _, mv in drops]


def test_records_playouts_text(tmp_path, monkeypatch):
    import json
    L = "abcde"
    sgf = lambda game, re: "(;FF[4]SZ[5]KM[5.5]RE[%s]" % re + "".join(                       # noqa: E731
        ";%s[%s]" % ("B" if c > 0 else "W", "" if a == S * S else L[a % S] + L[a // S]) for a, c in game) + ")"
    (tmp_path / "a.sgf").write_text(sgf(GAME, "B+3.5"))
    (tmp_path / "b.sgf").write_text(sgf(GAME[:2], "W+R"))
    monkeypatch.setattr(R, "DeviceRecords", PlayoutRecords)
    out, doc = io.StringIO(), tmp_path / "doc.json"
    assert R.main([str(tmp_path), "--size", "5", "--playouts", "5", "--json", str(doc)], out=out) == 0
    text = out.getvalue().split("\n")
    at = text.index("playouts (5 per position; an estimate)")
    d = json.loads(doc.read_text())["playouts"]
    assert d["per_row"] == 5 and [(g["name"], g["plies"], g["result"]) for g in d["games"]] == [("a", 5, "B"), ("b", 2, "W")]
    from tests import records_model
    recs = records_model.replay(S, [([a for a, _ in g], [c for _, c in g]) for g in (GAME, GAME[:2])])["records"]
    m = PM.playouts(S, recs, None, 5, 0, 1, 0)
    mean = m["sums"][:, 3] / 5.0
    assert abs(d["games"][0]["lead"] - mean[5]) < 1e-12 and abs(d["games"][1]["lead"] - mean[8]) < 1e-12
    assert text[at + 1].startswith("a: playouts %+.1f +- " % mean[5]) and text[at + 1].endswith("recorded B")
    assert len(d["buckets"]) == 1 and d["buckets"][0]["positions"] == 9 and abs(d["buckets"][0]["abs_score"] - np.abs(mean).mean()) < 1e-9
    assert text[at + 4].split()[:2] == ["1-20", "9"]


class ScriptedEngine(object):
    """what GTPEngine asks of the device engine for the playout commands: the model on a fixed record"""
    size = S

    def __init__(self):
        self.rec = PM.build_record(S, [P(1, 1), P(2, 1), P(1, 2)], [P(3, 3), P(3, 2)], True)
        self.asked = []
        self.model = type("M", (), {"name": "none"})()

    def load(self, moves, colors=None, n_setup=0):
        raise NotImplementedError

    def playouts(self, per_row=None, rules=1, seed=0):
        self.asked.append((per_row, rules))
        n = int(per_row or po.DEFAULT_PER_ROW)
        m = PM.playouts(S, self.rec[None], None, min(n, 24), seed, rules, 0)
        stones = np.zeros((S, S), np.int8)
        stones[1, 1] = stones[1, 2] = stones[2, 1] = 1
        stones[3, 3] = stones[2, 3] = -1
        return po.Playouts(S, m["own"], m["amaf"], m["sums"], [True]), stones

    def rollouts(self, per_src=None, seed=0):
        raise AssertionError("policy rollouts were asked for")


@pytest.fixture()
def conf5(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_playout_commands(conf5):
    dev = ScriptedEngine()
    e = gtp.GTPEngine(engine=dev, score="playouts")
    v, _ = dev.playouts(12, 1)
    dev.asked = []
    assert e.parse_command("sgo-playouts 12") == "= " + po.format_summary(v, 0) + "\n" + v.format_board(0) + "\n\n"
    assert e.parse_command("sgo-playouts inherited 12") .startswith("= score ") and dev.asked == [(12, 1), (12, 0)]
    assert e.parse_command("sgo-playouts") .startswith("= score ") and dev.asked[-1] == (po.DEFAULT_PER_ROW, 1)
    for bad in ("sgo-playouts 0", "sgo-playouts 3 4", "sgo-playouts sound", "sgo-playout-moves inherited inherited"):
        assert e.parse_command(bad) == "? syntax error\n\n", bad
    assert e.parse_command("sgo-playouts %d" % (po.MAX_PER_ROW + 1)).startswith("? at most")
    vd, _ = dev.playouts(None, 1)
    text = po.format_moves(vd, 0, 3, e._vertex, min_count=max(1, vd.count(0, "playouts") // 100))
    assert e.parse_command("sgo-playout-moves 3") == "= " + text + "\n\n" and 1 <= text.count("\n") + 1 <= 3
    assert {"sgo-playouts", "sgo-playout-moves"} <= set(e.parse_command("list_commands").split())
    # --score playouts: the three scoring commands stand on the playouts (the scripted engine refuses policy rollouts)
    row = vd.row(0)
    assert e.parse_command("final_score") == "= " + rollout.final_score(row, 0.0) + "\n\n"
    assert e.parse_command("final_status_list alive").startswith("=") and e.parse_command("final_status_list gone") == "? syntax error\n\n"
    assert len(e.parse_command("sgo-ownership").strip("= \n").split("\n")) == S


def test_gtp_score_option_needs_the_device(conf5, capsys):
    with pytest.raises(ValueError):
        gtp.GTPEngine(engine=None, score="playouts")
    with pytest.raises(ValueError):
        gtp.GTPEngine(engine=ScriptedEngine(), score="net")
    assert gtp.main(inp=[], device=False, score="playouts") == 2 and "--device" in capsys.readouterr().err
    assert gtp._cli(["--score", "playouts"]) == 2
    # without the option the scoring commands ask for policy rollouts, as before
    e = gtp.GTPEngine(engine=ScriptedEngine())
    with pytest.raises(AssertionError):
        e.parse_command("final_score")
