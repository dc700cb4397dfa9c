"""CPU: the host side of the chains and ladders -- records.RecordSet.tactics, the flags of `review --tactics` and GTP's
`sgo-ladders` -- on the fake replay object (tests/fake_records.py) extended with the `tactics` / `stones` surface of
records.DeviceRecords served by the model (tests/tactics_model.py), and on a scripted engine; no GPU, no library."""
import numpy as np
import pytest

from sejonggo_amd import gtp, records as R, review
from sejonggo_amd import tactics as tactics_mod
from sejonggo_amd.sgfload import SgfGame
from tests import tactics_cases as TC
from tests import tactics_model as T
from tests.fake_records import FakeRecords

S = 9
P = lambda x, y: y * S + x                                                               # noqa: E731


def _stones(size, rec):
    black, white = T.record_sets(size, rec)[:2]
    out = np.zeros(size * size, np.int8)
    out[black], out[white] = 1, -1
    return out


class TacticsRecords(FakeRecords):
    """FakeRecords with the tactics surface of records.DeviceRecords: the model on the records of the last replay, numpy out"""

    def tactics(self, index, max_chains=128):
        self.calls.append(("tactics", len(index), max_chains))
        m = T.tactics(self.S, self.last["records"], index, max_chains)
        chains = np.zeros((len(index), max_chains, 8), np.int32)
        for i, rows in enumerate(m["rows"]):
            chains[i, :len(rows)] = rows
        return m["libs"], m["n_chains"], chains

    def stones(self, index):
        self.calls.append(("stones", len(index)))
        recs = self.last["records"]
        return np.stack([_stones(self.S, recs[i]) if 0 <= i < len(recs) else np.zeros(self.S * self.S, np.int8) for i in index])


# the 9x9 ladder in atari, stone by stone, then: black runs (4,3), white chases (5,3), black runs (4,4), white plays away, black
# plays away, black passes on an occupied point (refused: the rest of the record is not played)
SHAPE = [(P(3, 3), 1), (P(3, 2), -1), (P(2, 3), -1), (P(4, 2), -1), (P(3, 4), -1)]
PLAY = [(P(4, 3), 1), (P(5, 3), -1), (P(4, 4), 1), (P(0, 8), -1), (P(8, 0), 1)]


def _game(entries, n_setup=0):
    return SgfGame(S, 5.5, list(entries), [i < n_setup for i in range(len(entries))])


def _set(game):
    rec = R.Record("game", S, list(game.moves), list(game.setup), list(range(1, len(game.moves) + 1)), None)
    return R.RecordSet([rec], S, backend=TacticsRecords(S, 4, 64))


def test_record_set_tactics_rows():
    game = _game(SHAPE + PLAY)
    rs = _set(game)
    chunks = list(rs.tactics(max_chains=4, stones=True))
    assert len(chunks) == 1 and [c[0] for c in rs.backend.calls] == ["replay", "tactics", "stones"]
    ch = chunks[0]
    t = ch.tactics
    n = len(game.moves)
    assert t.libs.shape == (n + 1, S * S) and t.chains.shape == (n + 1, 4, 8) and ch.stones.shape == (n + 1, S * S)
    assert t.n_chains[0] == 0 and not ch.stones[0].any()
    # row ch.index[e] is the position before entry e, row + 1 the one after it
    e = len(SHAPE)
    before, after = t.chains_of(int(ch.index[e])), t.chains_of(int(ch.index[e]) + 1)
    assert [(c.anchor, c.liberties, c.dead) for c in before] == [(P(3, 3), 1, True)]
    assert [(c.anchor, c.size, c.liberties, c.capturable, c.dead) for c in after] == [(P(3, 3), 2, 2, True, False)]
    assert ch.stones[int(ch.index[e]) + 1][P(4, 3)] == 1 and t.libs[int(ch.index[e]) + 1][P(4, 3)] == 2
    # a refused entry: the records behind it give the zero row
    rs2 = _set(_game(SHAPE + [(P(3, 3), -1), (P(0, 0), 1)]))
    ch2 = next(rs2.tactics())
    assert ch2.status[0] != 0 and ch2.tactics.n_chains[len(SHAPE)] == 1 and not ch2.tactics.n_chains[len(SHAPE) + 1:].any()
    assert not ch2.tactics.libs[len(SHAPE) + 1:].any()


def test_review_flags_on_a_played_out_ladder():
    # the shape as set-up stones: move numbers count the played moves
    game = _game(SHAPE + PLAY, n_setup=len(SHAPE))
    flags = review.move_flags(game, _set(game))
    assert flags == {1: ["ladder"], 2: [], 3: ["ladder"], 4: ["missed"], 5: []}
    rows = [{"move_number": m, "colour": "B", "played": "A1", "played_share": 0.5, "played_mean": 0.1, "best": "B2", "best_mean": 0.2,
             "top": [{"pv": ["B2", "C3"]}]} for m in (1, 2, 4, 9)]
    plain = [review.format_row(dict(r)) for r in rows]
    review.add_tactics(rows, game, record_set=_set(game))
    assert [r["tactics"] for r in rows] == [["ladder"], [], ["missed"], []]
    text = [review.format_row(r) for r in rows]
    assert text[0] == plain[0] + "  | ladder" and text[1] == plain[1] and text[2] == plain[2] + "  | missed" and text[3] == plain[3]
    # the same moves with the ladder broken: running is no mistake, and nothing was missed
    broken = _game(SHAPE[:4] + [(P(6, 6), 1), (P(3, 4), -1)] + PLAY, n_setup=len(SHAPE) + 1)
    assert review.move_flags(broken, _set(broken)) == {1: [], 2: [], 3: [], 4: [], 5: []}


def test_review_flags_logic():
    C = tactics_mod.Chain
    N = S * S
    before, after = np.zeros(N, np.int8), np.zeros(N, np.int8)
    before[[P(3, 3), P(7, 7), P(7, 8), P(8, 7)]] = [1, -1, -1, -1]
    after[:] = before
    after[P(4, 3)] = 1
    libs = np.zeros(N, np.uint8)
    libs[[P(7, 7), P(7, 8), P(8, 7)]] = 2
    dead = C(P(3, 3), 1, 1, 1, 19, P(4, 3), -1, 9)
    run = C(P(3, 3), 1, 2, 2, 17, P(4, 4), P(5, 3), 9)
    safe = C(P(3, 3), 1, 2, 2, 0, -1, -1, 9)
    prey = C(P(7, 7), -1, 3, 2, 17, P(6, 7), P(7, 6), 5)
    f = lambda cb, ca, action=P(4, 3), colour=1, st=after, lb=libs: tactics_mod.review_flags(S, action, colour, before, cb, st, ca, lb)   # noqa: E731
    assert f([dead], [run]) == ["ladder"]
    assert f([dead], [safe]) == [] and f([dead], []) == []               # the chain got away / has three liberties now
    assert f([dead._replace(status=17)], [run]) == []                    # capturable, not dead: running was right
    assert f([dead], [run], action=P(0, 0)) == []                        # played elsewhere
    assert f([dead], [run], action=N) == []                              # a pass
    assert f([dead._replace(colour=-1)], [run]) == []                    # the opponent's dead chain
    assert f([prey], []) == ["missed"] and f([dead, prey], [run]) == ["ladder", "missed"]
    assert f([prey._replace(size=2)], []) == [] and f([prey._replace(status=0)], []) == []
    assert f([prey], [], colour=-1) == []                                # the mover's own chain is not missed
    one = libs.copy()
    one[P(7, 7)] = 1
    assert f([prey], [], lb=one) == []                                   # in atari now: not left standing
    gone = after.copy()
    gone[[P(7, 7), P(7, 8), P(8, 7)]] = 0
    assert f([prey], [], st=gone) == []                                  # captured


class LadderEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: `tactics` serves the model's chains of a case"""
    model = type("N", (), {"name": "scripted"})()

    def __init__(self, size, case):
        names, recs = TC.case_records(size)
        rows = T.record_tactics(size, recs[names.index(case)])[1]
        self.chains = [tactics_mod.Chain(*(int(v) for v in r)) for r in rows]

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def tactics(self):
        return self.chains


@pytest.fixture()
def conf9(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def test_gtp_sgo_ladders(conf9):
    e = gtp.GTPEngine(engine=LadderEngine(S, "ladder_b"))
    assert e.parse_command("known_command sgo-ladders") == "= true\n\n" and "sgo-ladders" in e.parse_command("list_commands").split()
    assert e.parse_command("sgo-ladders") == "= D6 black size 1 liberties 2 capturable attack D5 defend E6\n\n"
    assert e.parse_command("sgo_ladders") == e.parse_command("sgo-ladders")
    e = gtp.GTPEngine(engine=LadderEngine(S, "ladder_atari_w"))
    assert e.parse_command("sgo-ladders") == "= D6 black size 1 liberties 1 dead attack E6 defend none\n\n"
    e = gtp.GTPEngine(engine=LadderEngine(S, "ladder_breaker_b"))
    assert e.parse_command("sgo-ladders") == "=\n\n"                    # listed, and not caught: no line
    e = gtp.GTPEngine(engine=LadderEngine(S, "ladder_beside_b"))
    lines = e.parse_command("sgo-ladders")[2:].rstrip("\n").split("\n")
    assert [l.split()[0] for l in lines] == ["A9", "J9", "D6"] and lines[1].split()[5:7] == ["1", "dead"]

    class Host(object):
        """the host engine's surface: no load, no tactics"""
        model = type("N", (), {"name": "x"})()

    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-ladders") == "? not supported\n\n"


def test_chain_view():
    c = tactics_mod.Chain(30, -1, 4, 2, 1 | 16 | 8, 31, -1, 600)
    assert c.capturable and not c.dead and c.unknown and c.colour == -1 and c.nodes == 600
    t = tactics_mod.Tactics(9, np.zeros((1, 81), np.uint8), np.array([3], np.int32), np.arange(16, dtype=np.int32).reshape(1, 2, 8))
    assert [c.anchor for c in t.chains_of(0)] == [0, 8]                  # more chains than rows: the stored ones
    assert tactics_mod.stones_of(5, T.build_record(5, [0, 24], [7], True).reshape(1, -1)).tolist()[0] == \
        [1, 0, 0, 0, 0, 0, 0, -1] + [0] * 16 + [1]
