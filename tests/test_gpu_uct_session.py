"""GPU: sgo_session_uct (include/sgo.h "playout tree search") on session slots set up with sgo_session_setup, on a 5x5 and a 9x9
context: every table equals sgo_uct_dev's route on the records of the same positions (the host twin sgo_uct) and the model
(tests/uct_model.py) on what sgo_game_board shows; a slot that is no holding session is refused with SGO_ERR_STATE and its rows stay as
they were filled; a slot may be listed twice; rave and own are optional."""
import numpy as np
import pytest

from tests import playout_cases as PC
from tests import uct_model as UM

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL32, FILL64 = 0x3C3C3C3C, 0x5A5A5A5A5A5A5A5A
CASES = ("eye_in2", "eye_edge1", "eye_in0", "eye_not", "words", "eye_corner1")
KEYS = ("visits", "wins2", "rave", "own", "sums", "info")
ARGS = dict(trees=3, sims=10, seed=51, max_plies=8, komi2=3, expand_at=1, rave_equiv=64, prior=4, max_nodes=11)


def _filled(S, n):
    N = S * S
    return {"status": np.full(n, 77, np.int32), "visits": np.full((n, N + 1), FILL32, np.int32), "wins2": np.full((n, N + 1), FILL32, np.int32),
            "rave": np.full((n, 2, N + 1), FILL32, np.int32), "own": np.full((n, 2, N), FILL32, np.int32), "sums": np.full((n, 8), FILL64, np.int64),
            "info": np.full((n, 4), FILL32, np.int32)}


def _ints(rules, **change):
    a = dict(ARGS, **change)
    return [a["trees"], a["sims"], a["seed"], rules, a["max_plies"], a["komi2"], a["expand_at"], a["rave_equiv"], a["prior"], a["max_nodes"]]


@pytest.mark.parametrize("S", [5, 9])
def test_session_uct(S):
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
            want = UM.search(S, recs, None, rules=rules, **ARGS)
            assert want["sums"][:, 7].tolist() == [30] * n and want["rave"][:, 0].any()
            tw = _filled(S, n)
            assert lib.sgo_uct(S, n, L.ptr(recs), n, None, *_ints(rules), *[L.ptr(tw[k]) for k in KEYS], None) == 0, lib.sgo_last_error()
            for k in KEYS:
                assert np.array_equal(tw[k], want[k]), ("host twin", rules, k)
            for tables in (True, False):
                got = _filled(S, n)
                rc = lib.sgo_session_uct(eng.ctx, n, L.ptr(sl), *_ints(rules), L.ptr(got["status"]),
                                         *[L.ptr(got[k]) if tables or k not in ("rave", "own") else None for k in KEYS], L.stream_ptr())
                assert rc == 0 and not got["status"].any(), lib.sgo_last_error()
                for k in KEYS:
                    assert np.array_equal(got[k], want[k] if tables or k not in ("rave", "own") else np.full_like(got[k], FILL32)), ("session", rules, tables, k)
        v = eng.uct(slots, trees=3, sims=10, seed=51, komi=1.5, max_plies=8, expand_at=1, rave_equiv=64, prior=4)
        want = UM.search(S, recs, None, rules=1, **ARGS)
        assert not v.status.any() and all(np.array_equal(getattr(v, k), want[k]) for k in KEYS)
        assert [v.best(i) for i in range(n)] == want["info"][:, 3].tolist()
        # slots 5 and 7 are no sessions; slot 3 is listed twice: g counts the list position, so the two rows differ
        listed = np.array([5, 3, 7, 3, 4], np.int32)
        want = UM.search(S, recs, [-1, 2, -1, 2, 0], rules=1, **ARGS)
        got = _filled(S, 5)
        rc = lib.sgo_session_uct(eng.ctx, 5, L.ptr(listed), *_ints(1), L.ptr(got["status"]), *[L.ptr(got[k]) for k in KEYS], L.stream_ptr())
        assert rc == 0 and got["status"].tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for k in KEYS:
            for i in (0, 2):
                assert (got[k][i] == (FILL64 if k == "sums" else FILL32)).all(), (k, i)
            for i in (1, 3, 4):
                assert np.array_equal(got[k][i], want[k][i]), (k, i)
        v = eng.uct([5, 3], trees=1, sims=2)
        assert v.status.tolist() == [SGO_ERR_STATE, 0] and not v.visits[0].any() and v.best(0) is None and v.sums[1, 7] == 2
        # the refusals: a slot outside the context, a bound, a NULL output; n == 0 is a no-op
        one = np.array([8], np.int32)

        def call(slots_=listed, n_=1, rules=1, null=(), **change):
            return lib.sgo_session_uct(eng.ctx, n_, L.ptr(slots_), *_ints(rules, **change), None if "status" in null else L.ptr(got["status"]),
                                       *[None if k in null else L.ptr(got[k]) for k in KEYS], L.stream_ptr())
        assert call(slots_=one) == SGO_ERR_ARG and call(n_=-1) == SGO_ERR_ARG and call(rules=2) == SGO_ERR_ARG
        for bad in (dict(trees=0), dict(sims=0), dict(sims=UM.MAX_SIMS + 1), dict(max_plies=4 * S * S + 1), dict(komi2=4 * S * S + 1), dict(expand_at=11),
                    dict(rave_equiv=-1), dict(prior=1025), dict(max_nodes=12), dict(max_nodes=0)):
            assert call(**bad) == SGO_ERR_ARG, bad
        for k in ("status", "visits", "wins2", "sums", "info"):
            assert call(null=(k,)) == SGO_ERR_ARG, k
        assert lib.sgo_session_uct(eng.ctx, 0, None, *_ints(1), None, None, None, None, None, None, None, L.stream_ptr()) == 0
    finally:
        eng.close()
