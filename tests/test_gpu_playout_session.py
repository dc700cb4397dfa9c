"""GPU: sgo_session_playout (include/sgo.h "light playouts") on session slots set up with sgo_session_setup, on a 5x5 and a 9x9
context: ownership, AMAF and sums equal sgo_playout (the host twin) and the model (tests/playout_model.py) on what sgo_game_board
shows; a slot that is no holding session is refused and its rows stay as they were filled; a slot may be listed twice; the table is
optional."""
import numpy as np
import pytest

from tests import playout_cases as PC
from tests import playout_model as PM

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL32, FILL64 = 0x3C3C3C3C, 0x5A5A5A5A5A5A5A5A
CASES = ("eye_in2", "eye_edge1", "eye_in0", "eye_not", "words", "eye_corner1")
PER_ROW, SEED, PLIES = 5, 51, 8


def _filled(S, n):
    return (np.full(n, 77, np.int32), np.full((n, 2, S * S), FILL32, np.int32), np.full((n, 2, S * S), FILL32, np.int32),
            np.full((n, 8), FILL64, np.int64))


@pytest.mark.parametrize("S", [5, 9])
def test_session_playout(S):
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    pos = dict((p[0], p) for p in PC.positions(S))
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=8, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1, 6, 2]
        eng.open(slots)
        moves, cols = [], []
        for k, name in enumerate(CASES):
            _, b, w = pos[name][:3]
            moves.append(list(b) + list(w) if k % 2 == 0 else list(w) + list(b))
            cols.append([1] * len(b) + [-1] * len(w) if k % 2 == 0 else [-1] * len(w) + [1] * len(b))
        st, _ = eng.setup(slots, moves, cols)
        assert not st.any()
        n = len(slots)
        recs = np.ascontiguousarray(np.concatenate([pack_boards(eng.board(s)) for s in slots]))   # what sgo_game_board shows, packed
        sl = np.array(slots, np.int32)
        for rules in (0, 1):
            want = PM.playouts(S, recs, None, PER_ROW, SEED, rules, PLIES)
            assert want["sums"][:, 7].tolist() == [PER_ROW] * n and want["amaf"][:, 0].any()
            _, own, am, sums = _filled(S, n)
            assert lib.sgo_playout(S, n, L.ptr(recs), n, None, PER_ROW, SEED, rules, PLIES, L.ptr(own), L.ptr(am), L.ptr(sums)) == 0
            assert (own == want["own"]).all() and (am == want["amaf"]).all() and (sums == want["sums"]).all(), ("host twin", rules)
            for amaf in (True, False):
                status, own, am, sums = _filled(S, n)
                rc = lib.sgo_session_playout(eng.ctx, n, L.ptr(sl), PER_ROW, SEED, rules, PLIES, L.ptr(status), L.ptr(own), L.ptr(am) if amaf else None,
                                             L.ptr(sums), L.stream_ptr())
                assert rc == 0 and not status.any(), lib.sgo_last_error()
                assert (own == want["own"]).all() and (sums == want["sums"]).all(), ("session", rules, amaf)
                assert (am == (want["amaf"] if amaf else FILL32)).all(), ("session amaf", rules, amaf)
        v = eng.playouts(slots, per_row=PER_ROW, seed=SEED, max_plies=PLIES)
        want = PM.playouts(S, recs, None, PER_ROW, SEED, 1, PLIES)
        assert not v.status.any() and (v.own == want["own"]).all() and (v.amaf == want["amaf"]).all() and (v.sums == want["sums"]).all()
        # slots 5 and 7 are no sessions; slot 3 is listed twice: g counts the list position, so the two rows differ
        listed = np.array([5, 3, 7, 3, 4], np.int32)
        want = PM.playouts(S, recs, [-1, 2, -1, 2, 0], PER_ROW, SEED, 1, PLIES)
        status, own, am, sums = _filled(S, 5)
        rc = lib.sgo_session_playout(eng.ctx, 5, L.ptr(listed), PER_ROW, SEED, 1, PLIES, L.ptr(status), L.ptr(own), L.ptr(am), L.ptr(sums), L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (own[i] == FILL32).all() and (am[i] == FILL32).all() and (sums[i] == FILL64).all()
        for i in (1, 3, 4):
            assert (own[i] == want["own"][i]).all() and (am[i] == want["amaf"][i]).all() and (sums[i] == want["sums"][i]).all(), i
        v = eng.playouts([5, 3], per_row=2)
        assert v.status.tolist() == [SGO_ERR_STATE, 0] and not v.own[0].any() and v.sums[1, 7] == 2
        # the refusals: a slot outside the context, a bound, a NULL output; n == 0 is a no-op
        one = np.array([8], np.int32)
        args = lambda **q: [eng.ctx, q.get("n", 1), L.ptr(q.get("slots", listed)), q.get("per_row", 2), 1, q.get("rules", 1), q.get("plies", 0),   # noqa: E731
                            q.get("status", L.ptr(status)), q.get("own", L.ptr(own)), None, q.get("sums", L.ptr(sums)), L.stream_ptr()]
        for bad in (dict(slots=one), dict(rules=2), dict(per_row=0), dict(per_row=PM.MAX_PER_ROW + 1), dict(plies=4 * S * S + 1), dict(status=None),
                    dict(own=None), dict(sums=None), dict(n=-1)):
            assert lib.sgo_session_playout(*args(**bad)) == SGO_ERR_ARG, bad
        assert lib.sgo_session_playout(eng.ctx, 0, None, 2, 1, 1, 0, None, None, None, None, L.stream_ptr()) == 0
    finally:
        eng.close()
