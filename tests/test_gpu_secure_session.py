"""GPU: sgo_session_secure (include/sgo.h "securing moves") on session slots set up with sgo_session_setup, on a 5x5 and a 9x9
context: the outputs equal sgo_secure (the host twin) and the model (tests/secure_model.py) on what sgo_game_board shows, for both
sides; a slot that is no holding session is refused and its rows stay as they were filled; a slot may be listed twice."""
import numpy as np
import pytest

from tests import secure_cases as SC
from tests import secure_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL16, FILL32 = 0x5A5A, 0x3C3C3C3C
CASES = ("capture_makes_eye", "capture_opens_eye", "connect", "two_eyes", "corner3", "suicide")


def _filled(S, n):
    NW = (S * S + 31) // 32
    return np.full(n, 77, np.int32), np.full((n, S * S, 4), FILL16, np.int16), np.full((n, 4, NW), FILL32, np.uint32), np.full((n, 8), FILL32, np.int32)


@pytest.mark.parametrize("S", [5, 9])
def test_session_secure(S):
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    pos = dict((n, (b, w)) for n, b, w, _ in SC.positions(S))
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=8, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1, 6, 2]
        eng.open(slots)
        moves, cols = [], []
        for k, name in enumerate(CASES):
            b, w = pos[name]
            if k % 2:                                                # every other case with the colours swapped, white's stones first
                b, w = w, b
            moves.append(list(b) + list(w) if k % 2 == 0 else list(w) + list(b))
            cols.append([1] * len(b) + [-1] * len(w) if k % 2 == 0 else [-1] * len(w) + [1] * len(b))
        st, _ = eng.setup(slots, moves, cols)
        assert not st.any()
        recs = np.concatenate([pack_boards(eng.board(s)) for s in slots])                # what sgo_game_board shows, packed
        for side in (0, 1):
            want = M.secure(S, recs, side=side)
            _, table, sets, counts = _filled(S, len(slots))
            assert lib.sgo_secure(S, len(slots), L.ptr(np.ascontiguousarray(recs)), side, L.ptr(table), L.ptr(sets), L.ptr(counts)) == 0
            v = eng.secure(slots, side)
            assert not v.status.any()
            for got in ((v.table, v.sets, v.counts), (table, sets, counts)):
                assert np.array_equal(got[0], want["table"]) and np.array_equal(got[1], want["sets"]) and np.array_equal(got[2], want["counts"]), side
        both = [M.secure(S, recs, side=side)["counts"] for side in (0, 1)]
        assert sum(int((c[:, 4] > 0).sum()) for c in both) >= 4 and sum(int((c[:, 7] > 0).sum()) for c in both) >= 1
        # slots 5 and 7 are no sessions; slot 3 is listed twice
        want = M.secure(S, recs, side=1)
        ask = np.array([5, 3, 7, 3, 4], np.int32)
        status, table, sets, counts = _filled(S, 5)
        rc = lib.sgo_session_secure(eng.ctx, 5, L.ptr(ask), 1, L.ptr(status), L.ptr(table), L.ptr(sets), L.ptr(counts), L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (table[i] == FILL16).all() and (sets[i] == FILL32).all() and (counts[i] == FILL32).all()
        for i, k in ((1, 2), (3, 2), (4, 0)):
            assert np.array_equal(table[i], want["table"][k]) and np.array_equal(sets[i], want["sets"][k]) and np.array_equal(counts[i], want["counts"][k])
        # the refusals: a slot outside the context, a side outside {0, 1}, a NULL output; n == 0 is a no-op
        one = np.array([8], np.int32)
        args = lambda **kw: [eng.ctx, kw.get("n", 1), L.ptr(kw.get("slots", ask)), kw.get("side", 0), L.ptr(status),   # noqa: E731
                             kw.get("table", L.ptr(table)), kw.get("sets", L.ptr(sets)), kw.get("counts", L.ptr(counts)), L.stream_ptr()]
        for bad in (dict(slots=one), dict(side=2), dict(side=-1), dict(table=None), dict(sets=None), dict(counts=None), dict(n=-1)):
            assert lib.sgo_session_secure(*args(**bad)) == SGO_ERR_ARG, bad
        assert lib.sgo_session_secure(eng.ctx, 0, None, 0, None, None, None, None, L.stream_ptr()) == 0
    finally:
        eng.close()


@pytest.fixture()
def env():
    from sejonggo_amd import _lib
    from sejonggo_amd.conf import conf
    _lib.require_gpu()
    keep = dict(conf)
    yield conf
    conf.clear()
    conf.update(keep)


def test_gtp_on_the_device(env):
    """the 9x9 `capture_opens_eye` position played into a device session stone by stone: `sgo-secure`, `sgo-secure opponent` and
    `sgo-secure min 1` are the model's text on the board the session shows"""
    from sejonggo_amd import gtp, secure as sc
    from sejonggo_amd.rollout import real_board
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    S = 9
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    black, white = [(b, w) for n, b, w, _ in SC.positions(S) if n == "capture_opens_eye"][0]
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for c, pts in (("B", black), ("W", white)):                  # white's stones last: black is to move
            for a in pts:
                assert e.parse_command("play %s %s" % (c, e._vertex(a))) == "=\n\n"
        rec = pack_boards(dev.board)
        stones = np.asarray(real_board(dev.board), dtype=np.int8).reshape(-1)
        for words, side, k in (("", 0, 2), ("opponent", 1, 2), ("min 1", 0, 1)):
            m = M.secure(S, rec, side=side)
            text = sc.format_board(sc.Secure(S, m["table"], m["sets"], m["counts"]), 0, stones, e._vertex, k)
            assert e.parse_command(("sgo-secure " + words).strip()) == "= " + text + "\n\n", words
        assert "harmful 1\nbest " in e.parse_command("sgo-secure") and "sgo-secure" in e.parse_command("list_commands").split()
    finally:
        dev.close()
