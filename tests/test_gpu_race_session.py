"""GPU: sgo_session_race (include/sgo.h "capturing races") on session slots set up with sgo_session_setup, on a 5x5 and a 9x9
context: asked and enumerated rows equal sgo_race (the host twin) and the model (tests/race_model.py) on what sgo_game_board shows;
a slot that is no holding session is refused and its rows stay as they were filled; a slot may be listed twice; GTP's `sgo-race`
answers on a device session."""
import numpy as np
import pytest

from tests import race_cases as RC
from tests import race_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL = 0x3C3C3C3C
T = 6
CASES = {5: ("tiny", "box", "run", "open", "empty_point", "ko"), 9: ("seki", "eye", "nakade", "plain_2v2", "plain_2v1", "shared")}


def _filled(S, n):
    NW = (S * S + 31) // 32
    return np.full(n, 77, np.int32), np.full(n, FILL, np.int32), np.full((n, T, 16), FILL, np.int32), np.full((n, T, NW), FILL, np.uint32)


def _same(n_pairs, rows, regions, want, pairs, what):
    for i, k in pairs:
        m = len(want["rows"][k])
        assert n_pairs[i] == want["n_pairs"][k], (what, i)
        assert rows[i, :m].tolist() == want["rows"][k].tolist() and regions[i, :m].tolist() == want["regions"][k].tolist(), (what, i, rows[i, :m].tolist())
        assert (rows[i, m:] == FILL).all() and (regions[i, m:] == FILL).all(), (what, "behind the listed rows", i)


@pytest.mark.parametrize("S", [5, 9])
def test_session_race(S):
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    pos = dict((p[0], p) for p in RC.positions(S))
    NW = (S * S + 31) // 32
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=8, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1, 6, 2]
        eng.open(slots)
        moves, cols, ask, region = [], [], [], []
        for k, name in enumerate(CASES[S]):
            _, b, w, _, _, a, reg = pos[name]
            moves.append(list(b) + list(w) if k % 2 == 0 else list(w) + list(b))
            cols.append([1] * len(b) + [-1] * len(w) if k % 2 == 0 else [-1] * len(w) + [1] * len(b))
            ask.append(a)
            region.append(M._words(range(S * S) if reg is None else reg, NW))
        st, _ = eng.setup(slots, moves, cols)
        assert not st.any()
        ask, region, n = np.array(ask, np.int32).reshape(-1, 2), np.stack(region), len(slots)
        recs = np.ascontiguousarray(np.concatenate([pack_boards(eng.board(s)) for s in slots]))   # what sgo_game_board shows, packed
        kw = dict(rules=1, max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION, max_nodes=RC.MAX_NODES, max_pairs=T)
        par = (1, RC.MAX_LIBS, RC.MAX_REGION, RC.MAX_NODES, T)
        for what, a, g in (("enumerated", None, None), ("asked", ask, None), ("asked in regions", ask, region)):
            want = M.race(S, recs, ask=a, region=g, **kw)
            _, nt, rows, regs = _filled(S, n)
            assert lib.sgo_race(S, n, L.ptr(recs), L.ptr(a), L.ptr(g), *par, L.ptr(nt), L.ptr(rows), L.ptr(regs)) == 0
            _same(nt, rows, regs, want, [(i, i) for i in range(n)], (what, "host twin"))
            status, nt, rows, regs = _filled(S, n)
            sl = np.array(slots, np.int32)
            rc = lib.sgo_session_race(eng.ctx, n, L.ptr(sl), L.ptr(a), L.ptr(g), *par, L.ptr(status), L.ptr(nt), L.ptr(rows), L.ptr(regs), L.stream_ptr())
            assert rc == 0 and not status.any()
            _same(nt, rows, regs, want, [(i, i) for i in range(n)], (what, "session"))
        v = eng.race(slots, ask=ask, max_libs=RC.MAX_LIBS, max_region=RC.MAX_REGION, max_nodes=RC.MAX_NODES, max_pairs=T)
        want = M.race(S, recs, ask=ask, **kw)
        assert not v.status.any() and v.n_pairs.tolist() == want["n_pairs"].tolist()
        assert all(v.rows[i, :len(want["rows"][i])].tolist() == want["rows"][i].tolist() for i in range(n))
        assert len({M.verdicts(want["rows"][i][0]) for i in range(n)}) >= 3
        # slots 5 and 7 are no sessions; slot 3 is listed twice, once asked and once enumerated
        listed = np.array([5, 3, 7, 3, 4], np.int32)
        a = np.array([(0, 1), tuple(ask[2]), (0, 1), (-1, -1), tuple(ask[0])], np.int32)
        status, nt, rows, regs = _filled(S, 5)
        rc = lib.sgo_session_race(eng.ctx, 5, L.ptr(listed), L.ptr(a), None, *par, L.ptr(status), L.ptr(nt), L.ptr(rows), L.ptr(regs), L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert nt[i] == FILL and (rows[i] == FILL).all() and (regs[i] == FILL).all()
        _same(nt, rows, regs, want, [(1, 2), (4, 0)], "repeated and refused, asked")
        _same(nt, rows, regs, M.race(S, recs, **kw), [(3, 2)], "repeated, enumerated")
        # the refusals: a slot outside the context, a bound, a NULL output; n == 0 is a no-op
        one = np.array([8], np.int32)
        args = lambda **q: [eng.ctx, q.get("n", 1), L.ptr(q.get("slots", listed)), None, None, q.get("rules", 1), q.get("libs", 4),   # noqa: E731
                            q.get("region", 6), q.get("nodes", 64), q.get("pairs", T), L.ptr(status), q.get("nt", L.ptr(nt)),
                            q.get("rows", L.ptr(rows)), q.get("regs", L.ptr(regs)), L.stream_ptr()]
        for bad in (dict(slots=one), dict(rules=2), dict(libs=0), dict(libs=9), dict(region=0), dict(region=33), dict(nodes=0), dict(nodes=32769),
                    dict(pairs=65), dict(nt=None), dict(rows=None), dict(regs=None), dict(n=-1)):
            assert lib.sgo_session_race(*args(**bad)) == SGO_ERR_ARG, bad
        assert lib.sgo_session_race(eng.ctx, 0, None, None, None, 1, 4, 6, 64, T, None, None, None, None, L.stream_ptr()) == 0
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
    """the 9x9 `plain_2v2` position played into a device session stone by stone: `sgo-race`, with two vertices, with `inherited` and
    with a small budget are the model's text on the board the session shows"""
    from sejonggo_amd import gtp, race as rc
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    S = 9
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    _, black, white, _, _, a, _ = [p for p in RC.positions(S) if p[0] == "plain_2v2"][0]
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for c, pts in (("B", black), ("W", white)):
            for p in pts:
                assert e.parse_command("play %s %s" % (c, e._vertex(p))) == "=\n\n"
        rec = pack_boards(dev.board)

        def text(ask=None, **kw):
            m = M.race(S, rec, ask=None if ask is None else [ask], **kw)
            return "\n".join(rc.format_pair(rc.Pair(*(int(x) for x in r)), e._vertex, S * S) for r in m["rows"][0])

        assert e.parse_command("sgo-race") == "= " + text() + "\n\n" and "C9 E9 libs 2 2 shared 0 empty 4 first to move wins " in text()
        assert e.parse_command("sgo-race E9 C9") == "= " + text(a) + "\n\n" and text(a).count("\n") == 0
        assert e.parse_command("sgo-race C9 E9 inherited nodes 5 libs 3") == "= " + text(a, rules=0, max_nodes=5, max_libs=3) + "\n\n"
        assert " unknown" in text(a, rules=0, max_nodes=5, max_libs=3)
        assert e.parse_command("sgo-race B9 C9") == "? no pair on B9 C9\n\n" and "sgo-race" in e.parse_command("list_commands").split()
    finally:
        dev.close()
