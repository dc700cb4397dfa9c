"""CPU-only: the host side of interactive games -- engine.SessionEngine's genmove loop and gtp.DeviceSejongGoEngine behind
GTPEngine -- on a small fake of the three sgo_session_* calls (no GPU, no library), and the bindings' missing-symbol error."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from sejonggo_amd import _lib, gtp
from sejonggo_amd.engine import MoveRecord, SessionEngine

S = 9
A = S * S + 1


def _ints(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (n,))


class FakeLib(object):
    """The three session calls on plain boards: stones never die, genmove takes the first empty point (or resigns)."""

    def __init__(self, eng):
        self.eng = eng
        self.calls = []

    def sgo_session_open(self, ctx, n, slots, resign, stream):
        for s in _ints(slots, n.value):
            self.eng.games[int(s)] = {"stones": {}, "to_play": 1, "armed": False}
        self.calls.append(("open", _ints(slots, n.value).tolist()))
        return 0

    def sgo_session_play(self, ctx, n, slots, actions, colors, status, stream):
        st = _ints(status, n.value)
        for i, (s, a, c) in enumerate(zip(_ints(slots, n.value), _ints(actions, n.value), _ints(colors, n.value))):
            g = self.eng.games.get(int(s))
            if g is None or g["armed"]:
                st[i] = -203
            elif not 0 <= a < A:
                st[i] = -102
            elif int(a) in g["stones"]:
                st[i] = -101
            else:
                mover = int(c) or g["to_play"]
                if a < S * S:
                    g["stones"][int(a)] = mover
                g["to_play"] = -mover
                st[i] = 0
        self.calls.append(("play", _ints(slots, n.value).tolist(), _ints(actions, n.value).tolist(), _ints(colors, n.value).tolist()))
        return 0

    def sgo_session_genmove(self, ctx, n, slots, stream):
        gs = [self.eng.games.get(int(s)) for s in _ints(slots, n.value)]
        if any(g is None or g["armed"] for g in gs):
            return -203
        for g in gs:
            g["armed"], g["wait"] = True, self.eng.delay
        return 0

    def sgo_last_error(self):
        return b"a listed slot is not a holding session"


class FakeSession(SessionEngine):
    def __init__(self, n_games=2, sims=16, energy=4, delay=3):
        self.S, self.A, self.G, self.sims, self.E = S, A, n_games, sims, energy
        self.lib, self.ctx, self.stream = FakeLib(self), None, None
        self.status = _lib.Status()
        self.records, self.game_ids, self.games = {}, {}, {}
        self.delay, self.resign_next, self.n_steps = delay, False, 0
        self.net = type("Net", (), {"name": "fake-net"})()
        self._fresh = []

    def close(self):
        self.ctx = None

    def _on_stream(self):
        return contextlib.nullcontext()

    def _stream_ptr(self):
        return None

    def step(self):
        self.n_steps += 1
        for s, g in sorted(self.games.items()):
            if not g["armed"]:
                continue
            g["wait"] -= 1
            if g["wait"] > 0:
                continue
            g["armed"] = False
            a = -1 if self.resign_next else min(set(range(S * S)) - set(g["stones"]))
            if a >= 0:
                g["stones"][a] = g["to_play"]
                g["to_play"] = -g["to_play"]
            pol = np.zeros(A)
            if a >= 0:
                pol[a] = 1.0
            self._fresh.append((s, MoveRecord(policy=pol, value=np.float32(-0.5), action=a, move_n=0, player=1)))
        self.status.n_records = len(self._fresh)
        return self.status

    def drain(self):
        for s, r in self._fresh:
            self.records.setdefault(s, []).append(r)
        n, self._fresh, self.status.n_records = len(self._fresh), [], 0
        return n

    def board(self, slot):
        g = self.games[slot]
        b = np.zeros((1, S, S, 17), np.int32)
        for a, c in g["stones"].items():
            b[0, a // S, a % S, 0 if c == g["to_play"] else 1] = 1
        b[..., 16] = g["to_play"]
        return b

    def tree_dict(self, slot):
        return {'subtree': {}, 'count': 0}


@pytest.fixture()
def gtp_engine(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    eng = FakeSession()
    dev = gtp.DeviceSejongGoEngine(16, engine=eng, slot=1)
    return gtp.GTPEngine(engine=dev), dev, eng


def test_gtp_text_on_the_device_engine(gtp_engine):
    e, dev, eng = gtp_engine
    assert eng.lib.calls == [("open", [1])] and "fake-net" in e.name()
    assert e.parse_command("play B E5") == "=\n\n"
    assert eng.lib.calls[-1] == ("play", [1], [4 * S + 4], [1]) and dev.player == 1 and dev.board[0, 0, 0, -1] == -1 and dev.move == 2
    assert e.parse_command("genmove W") == "= A9\n\n"                 # action 0 = (0, 0): column A, top row
    assert e.board[0, 0, 0, 1] == 1 and e.player == -1 and dev.move == 3
    assert e.parse_command("play B pass") == "=\n\n" and eng.lib.calls[-1][2] == [S * S] and dev.player == 1
    assert e.parse_command("genmove W") == "= B9\n\n"
    assert e.parse_command("play B J1") == "=\n\n" and eng.lib.calls[-1][2] == [8 * S + 8]
    with pytest.raises(ValueError, match="occupied"):
        e.parse_command("play W J1")
    with pytest.raises(ValueError, match="not to move"):
        e.parse_command("genmove B")                                  # white is to move
    assert dev.move == 6
    eng.resign_next = True
    board = dev.board
    assert e.parse_command("genmove W") == "= resign\n\n"
    assert np.array_equal(board, dev.board) and dev.move == 6
    assert e.parse_command("clear_board") == "=\n\n"
    assert eng.lib.calls[-1] == ("open", [1]) and not dev.board[..., :16].any() and dev.move == 1 and dev.player == 1
    assert not dev.mcts_tree['subtree']


def test_genmove_steps_are_bounded(gtp_engine):
    from sejonggo_amd.build import build_lib
    build_lib()                                         # _lib.check reads the library's error text
    _, dev, eng = gtp_engine
    eng.open([0])
    bound = eng.genmove_step_bound(2)
    assert bound >= eng.sims + 3
    eng.delay = bound                                   # the move arrives with the last step the bound allows
    assert [a for a, _, _ in eng.genmove([0, 1])] == [0, 0]
    eng.delay, eng.n_steps = bound + 1, 0
    with pytest.raises(_lib.SgoError, match="recorded no move within %d steps" % bound):
        eng.genmove([0, 1])
    assert eng.n_steps == bound
    with pytest.raises(_lib.SgoError, match="sgo_session_genmove"):    # still armed: the library refuses, nothing is stepped
        eng.genmove([0])
    assert eng.n_steps == bound


def test_batched_play_returns_one_status_per_slot():
    eng = FakeSession(n_games=3)
    eng.open([0, 2])
    assert eng.play([0, 2, 1], [5, A, 5]).tolist() == [0, -102, -203]
    assert eng.play([0, 2], [5, 6], [None, -1]).tolist() == [-101, 0] and eng.lib.calls[-1][3] == [0, -1]
    with pytest.raises(ValueError):
        eng.play([0, 2], [5])


def test_temperature_and_noise_are_refused():
    eng = FakeSession()
    with pytest.raises(ValueError):
        gtp.DeviceSejongGoEngine(16, engine=eng, temperature=1)
    with pytest.raises(ValueError):
        gtp.DeviceSejongGoEngine(16, engine=eng, add_noise=True)
    dev = gtp.DeviceSejongGoEngine(16, engine=eng)
    with pytest.raises(ValueError):
        dev.set_temperature(1)
    with pytest.raises(ValueError):
        SessionEngine(None, graph=True)
    assert eng.lib.calls == [("open", [0])]


def test_a_stale_library_is_named(monkeypatch):
    """Entry points are added without a version bump, so a library that predates one must fail at load() with the rebuild hint."""
    from sejonggo_amd.build import build_lib
    build_lib()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SYMBOLS", _lib.SYMBOLS + ["sgo_session_not_there"])
    with pytest.raises(_lib.SgoError, match=r"lacks sgo_session_not_there.*rebuild"):
        _lib.load()
    monkeypatch.setattr(_lib, "SYMBOLS", _lib.SYMBOLS[:-1])
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in ("sgo_session_open", "sgo_session_play", "sgo_session_genmove"))
