"""GPU: sgo_session_life (include/sgo.h "unconditional life") on 9x9 session slots set up with sgo_session_setup: the outputs equal
the model (tests/life_model.py) on what sgo_game_board shows; a slot that is no holding session is refused and its rows stay as
they were filled; a slot may be listed twice."""
import numpy as np
import pytest

from tests import life_cases as LC
from tests import life_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL = 0x3C3C3C3C
S = 9
CASES = ("two_eyes", "dead_stone", "cascade", "wall", "shared", "diagonal_alive")


def _model_of_board(board17):
    from sejonggo_amd.rollout import real_board
    stones = real_board(board17).reshape(-1)
    m = M.point_life(S, [int(a) for a in np.flatnonzero(stones == 1)], [int(a) for a in np.flatnonzero(stones == -1)])
    NW = (S * S + 31) // 32
    sets = np.stack([M._words(m["alive"][0], NW), M._words(m["alive"][1], NW), M._words(m["terr"][0], NW), M._words(m["terr"][1], NW)])
    return sets, np.array(m["counts"], np.int32)


def test_session_life():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    pos = dict((n, (b, w)) for n, b, w in LC.positions(S))
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=8, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1, 6, 2]
        eng.open(slots)
        moves, cols = [], []
        for k, name in enumerate(CASES):
            b, w = pos[name]
            if k % 2:                                            # every other case with the colours swapped
                b, w = w, b
            moves.append(list(b) + list(w))
            cols.append([1] * len(b) + [-1] * len(w))
        st, _ = eng.setup(slots, moves, cols)
        assert not st.any()
        want = [_model_of_board(eng.board(s)) for s in slots]
        assert sum(int(c[:2].sum()) > 0 for _, c in want) >= 4 and want[1][1][4:6].tolist() == [0, 1]   # the dead stone, colours swapped
        v = eng.life(slots)
        assert not v.status.any()
        for i in range(len(slots)):
            assert np.array_equal(v.sets[i], want[i][0]) and np.array_equal(v.counts[i], want[i][1]), CASES[i]
        # slots 5 and 7 are no sessions; slot 3 is listed twice
        ask = np.array([5, 3, 7, 3, 4], np.int32)
        NW = (S * S + 31) // 32
        status, sets, counts = np.full(5, 77, np.int32), np.full((5, 4, NW), FILL, np.uint32), np.full((5, 8), FILL, np.int32)
        rc = lib.sgo_session_life(eng.ctx, 5, L.ptr(ask), L.ptr(status), L.ptr(sets), L.ptr(counts), L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (sets[i] == FILL).all() and (counts[i] == FILL).all()
        for i, k in ((1, 2), (3, 2), (4, 0)):
            assert np.array_equal(sets[i], want[k][0]) and np.array_equal(counts[i], want[k][1])
        # the refusals: a slot outside the context, NULL outputs; n == 0 is a no-op
        one = np.array([8], np.int32)
        assert lib.sgo_session_life(eng.ctx, 1, L.ptr(one), L.ptr(status), L.ptr(sets), L.ptr(counts), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_life(eng.ctx, 1, L.ptr(ask), L.ptr(status), None, L.ptr(counts), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_life(eng.ctx, 0, None, None, None, None, L.stream_ptr()) == 0
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


def test_gtp_and_review_on_the_device(env, tmp_path):
    """the 5x5 settled board played into a device session stone by stone: `sgo-life` before and after the last stone; the same
    moves as a record through review.main --life: the flags tests/test_life_host.py derives from the model, and without --life the
    lines are the same text without them"""
    import io
    from sejonggo_amd import gtp, review
    from sejonggo_amd.stub_nets import make_stub
    from tests.test_life_host import SETTLED_GAME, SETTLED_TEXT, review_sgf
    size = 5
    env.update({'SIZE': size, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", size), size=size, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for a, c in SETTLED_GAME[:-3]:
            assert e.parse_command("play %s %s" % ("B" if c > 0 else "W", e._vertex(a))) == "=\n\n"
        before = e.parse_command("sgo-life")
        assert before.endswith("\nsettled 24/25 black 14 white 10\n\n") and before.split("\n")[4] == "BB.WW"
        assert e.parse_command("play B %s" % e._vertex(SETTLED_GAME[-3][0])) == "=\n\n"
        assert e.parse_command("sgo-life") == "= " + SETTLED_TEXT + "\n\n"
        assert "sgo-life" in e.parse_command("list_commands").split()
    finally:
        dev.close()
    sgf = tmp_path / "g.sgf"
    sgf.write_text(review_sgf())
    args = [str(sgf), "--net", "hash", "--symmetry", "identity", "--sims", "8", "--energy", "4"]
    plain, flagged = io.StringIO(), io.StringIO()
    assert review.main(args, out=plain) == 0 and review.main(args + ["--life"], out=flagged) == 0
    a, b = plain.getvalue().rstrip("\n").split("\n"), flagged.getvalue().rstrip("\n").split("\n")
    assert len(a) == len(b) == 3 and "|" not in plain.getvalue()
    assert b == [a[0], a[1] + "  | inside decided", a[2]]
