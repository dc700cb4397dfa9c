"""GPU: sgo_session_shapes (include/sgo.h "shape search") on 9x9 session slots set up with sgo_session_setup: the outputs equal the
model (tests/shapes_model.py) on what sgo_game_board shows; a slot that is no holding session is refused and its rows stay as they
were filled; a slot may be listed twice; the context is byte for byte what it was (the dumps of tests/block_audit.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import block_audit as BA
from tests import shapes_cases as SC
from tests import shapes_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL = 0x3C3C3C3C
S = 9
CASES = ("hook@1,1", "hook_swapped", "hook/g4", "hook@br", "two_stones", "corner@0,0")


def _model_of_board(board17, sh):
    from sejonggo_amd.rollout import real_board
    stones = real_board(board17).reshape(-1)
    hits, cover, _ = M.point_shapes(S, [int(a) for a in np.flatnonzero(stones == 1)], [int(a) for a in np.flatnonzero(stones == -1)], sh)
    return np.array(hits, np.int32), M._words(cover, (S * S + 31) // 32)


def _same_dump(a, b):
    """two (games, pool) dumps of block_audit.dump_engine hold the same bytes"""
    def same(x, y):
        if isinstance(x, dict):
            return sorted(x) == sorted(y) and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, np.ndarray):
            return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        return x == y
    return same(a[0], b[0]) and same(a[1], b[1])


def test_session_shapes():
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.shapes import Shape
    from sejonggo_amd.stub_nets import make_stub
    from tests.fake_shapes_records import model_shape
    pos = dict((n, (b, w)) for n, b, w in SC.positions(S))
    hook, corner = Shape.parse(".XO/*X."), Shape.parse("+---\n|*X.\n|XO.\n|...")
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=8, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1, 6, 2]
        eng.open(slots)
        moves, cols = [], []
        for name in CASES:
            b, w = pos[name]
            moves.append(list(b) + list(w))
            cols.append([1] * len(b) + [-1] * len(w))
        st, _ = eng.setup(slots, moves, cols)
        assert not st.any()
        before = BA.dump_engine(eng)
        for shape in (hook, corner):
            want = [_model_of_board(eng.board(s), model_shape(shape)) for s in slots]
            hit = [int(h[0]) > 0 for h, _ in want]
            assert any(hit) and not all(hit)
            v = eng.shapes(slots, shape)
            assert not v.status.any()
            for i in range(len(slots)):
                assert np.array_equal(v.hits[i], want[i][0]) and np.array_equal(v.cover_words[i], want[i][1]), CASES[i]
        want = [_model_of_board(eng.board(s), model_shape(hook)) for s in slots]
        assert [int(h[2]) for h, _ in want[:3]] == [1 << 0, 1 << 8, 1 << 4]               # as drawn, exchanged, turned
        # slots 5 and 7 are no sessions; slot 3 is listed twice
        ask = np.array([5, 3, 7, 3, 4], np.int32)
        NW = (S * S + 31) // 32
        status, hits, cover = np.full(5, 77, np.int32), np.full((5, 4), FILL, np.int32), np.full((5, NW), FILL, np.uint32)
        s = hook.to_struct()
        rc = lib.sgo_session_shapes(eng.ctx, 5, L.ptr(ask), C.byref(s), L.ptr(status), L.ptr(hits), L.ptr(cover), L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (hits[i] == FILL).all() and (cover[i] == FILL).all()
        for i, k in ((1, 2), (3, 2), (4, 0)):
            assert np.array_equal(hits[i], want[k][0]) and np.array_equal(cover[i], want[k][1])
        # the refusals: a slot outside the context, NULL outputs, a shape the compiler refuses (wider than the board); n == 0 is a no-op
        one = np.array([8], np.int32)
        assert lib.sgo_session_shapes(eng.ctx, 1, L.ptr(one), C.byref(s), L.ptr(status), L.ptr(hits), L.ptr(cover), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_shapes(eng.ctx, 1, L.ptr(ask), C.byref(s), L.ptr(status), None, L.ptr(cover), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_shapes(eng.ctx, 1, L.ptr(ask), None, L.ptr(status), L.ptr(hits), L.ptr(cover), L.stream_ptr()) == SGO_ERR_ARG
        wide = Shape([[1] * (S + 1)]).to_struct()
        assert lib.sgo_session_shapes(eng.ctx, 1, L.ptr(ask), C.byref(wide), L.ptr(status), L.ptr(hits), L.ptr(cover), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_shapes(eng.ctx, 0, None, C.byref(s), None, None, None, L.stream_ptr()) == 0
        assert _same_dump(before, BA.dump_engine(eng))                # the context was only read
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
    """the hook played into a 5x5 device session stone by stone: `sgo-find` before and after the stone that completes it; the same
    moves as a record through review.main --find: the flags tests/test_shapes_host.py derives from the model, and without --find the
    lines are the same text without them"""
    import io
    from sejonggo_amd import gtp, review
    from sejonggo_amd.stub_nets import make_stub
    from tests.test_shapes_host import GAME_A, HOOK, _sgf
    size = 5
    env.update({'SIZE': size, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", size), size=size, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for a, c in GAME_A[:2]:
            assert e.parse_command("play %s %s" % ("B" if c > 0 else "W", e._vertex(a))) == "=\n\n"
        assert e.parse_command("sgo-find " + HOOK).endswith("\nhits 0 variants - cover 0\n\n")
        assert e.parse_command("play B %s" % e._vertex(GAME_A[2][0])) == "=\n\n"
        assert e.parse_command("sgo-find " + HOOK) == "= .....\n.###.\n..##.\n.....\n.....\nhits 1 variants 0 cover 5\n\n"
        assert "sgo-find" in e.parse_command("list_commands").split()
    finally:
        dev.close()
    sgf, shape_file = tmp_path / "g.sgf", tmp_path / "hook.txt"
    sgf.write_text(_sgf(GAME_A[:4]))
    shape_file.write_text(HOOK.replace("/", "\n") + "\n")
    args = [str(sgf), "--net", "hash", "--symmetry", "identity", "--sims", "8", "--energy", "4"]
    plain, flagged = io.StringIO(), io.StringIO()
    assert review.main(args, out=plain) == 0 and review.main(args + ["--find", str(shape_file)], out=flagged) == 0
    a, b = plain.getvalue().rstrip("\n").split("\n"), flagged.getvalue().rstrip("\n").split("\n")
    assert len(a) == len(b) == 4 and "|" not in plain.getvalue()
    assert b == [a[0], a[1], a[2] + "  | appears", a[3] + "  | disappears"]
