"""GPU: sgo_session_connect (include/sgo.h "connections") on session slots set up with sgo_session_setup, on a 5x5 and a 9x9 context:
asked and enumerated rows, group maps and counts equal sgo_connect (the host twin) and the model (tests/connect_model.py) on what
sgo_game_board shows; a slot that is no holding session is refused and its rows stay as they were filled; a slot may be listed twice;
GTP's `sgo-connect` and `sgo-groups` answer on a device session."""
import numpy as np
import pytest

from tests import connect_cases as CC
from tests import connect_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL = 0x3C3C3C3C
FILL16 = 0x3C3C
T = 6
CASES = {5: ("diagonal", "jump", "jump_edge", "peep", "fill", "empty_point"),
         9: ("cutter_atari", "false_join", "chain3", "bamboo", "two_colours", "crosscut")}


def _filled(S, n):
    NW = (S * S + 31) // 32
    return (np.full(n, 77, np.int32), np.full(n, FILL, np.int32), np.full((n, T, M.W), FILL, np.int32), np.full((n, T, NW), FILL, np.uint32),
            np.full((n, S * S), FILL16, np.int16), np.full((n, 4), FILL, np.int32))


def _same(out, want, pairs, what):
    n_pairs, rows, regions, groups, counts = out
    for i, k in pairs:
        m = len(want["rows"][k])
        assert n_pairs[i] == want["n_pairs"][k], (what, i)
        assert rows[i, :m].tolist() == want["rows"][k].tolist() and regions[i, :m].tolist() == want["regions"][k].tolist(), (what, i, rows[i, :m].tolist())
        assert (rows[i, m:] == FILL).all() and (regions[i, m:] == FILL).all(), (what, "behind the listed rows", i)
        assert groups[i].tolist() == want["groups"][k].tolist() and counts[i].tolist() == want["counts"][k].tolist(), (what, "map", i)


@pytest.mark.parametrize("S", [5, 9])
def test_session_connect(S):
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    pos = dict((p[0], p) for p in CC.positions(S))
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
        kw = dict(rules=1, cut_libs=CC.CUT_LIBS, max_region=CC.MAX_REGION, max_nodes=CC.MAX_NODES, max_pairs=T)
        par = (1, CC.CUT_LIBS, CC.MAX_REGION, CC.MAX_NODES, T)
        for what, a, g in (("enumerated", None, None), ("asked", ask, None), ("asked in regions", ask, region)):
            want = M.connect(S, recs, ask=a, region=g, **kw)
            out = _filled(S, n)[1:]
            assert lib.sgo_connect(S, n, L.ptr(recs), L.ptr(a), L.ptr(g), *par, *[L.ptr(o) for o in out]) == 0
            _same(out, want, [(i, i) for i in range(n)], (what, "host twin"))
            status, *out = _filled(S, n)
            sl = np.array(slots, np.int32)
            rc = lib.sgo_session_connect(eng.ctx, n, L.ptr(sl), L.ptr(a), L.ptr(g), *par, L.ptr(status), *[L.ptr(o) for o in out], L.stream_ptr())
            assert rc == 0 and not status.any()
            _same(out, want, [(i, i) for i in range(n)], (what, "session"))
        v = eng.connect(slots, ask=ask, cut_libs=CC.CUT_LIBS, max_region=CC.MAX_REGION, max_nodes=CC.MAX_NODES, max_pairs=T)
        want = M.connect(S, recs, ask=ask, **kw)
        assert not v.status.any() and v.n_pairs.tolist() == want["n_pairs"].tolist()
        assert all(v.rows[i, :len(want["rows"][i])].tolist() == want["rows"][i].tolist() for i in range(n))
        assert all(v.groups[i].tolist() == want["groups"][i].tolist() and v.group_counts[i].tolist() == want["counts"][i].tolist() for i in range(n))
        assert len({M.verdict(want["rows"][i][0]) for i in range(n)}) >= 3
        # slots 5 and 7 are no sessions; slot 3 is listed twice, once asked and once enumerated
        listed = np.array([5, 3, 7, 3, 4], np.int32)
        a = np.array([(0, 1), tuple(ask[2]), (0, 1), (-1, -1), tuple(ask[0])], np.int32)
        status, *out = _filled(S, 5)
        rc = lib.sgo_session_connect(eng.ctx, 5, L.ptr(listed), L.ptr(a), None, *par, L.ptr(status), *[L.ptr(o) for o in out], L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert out[0][i] == FILL and (out[1][i] == FILL).all() and (out[2][i] == FILL).all() and (out[3][i] == FILL16).all() and (out[4][i] == FILL).all()
        _same(out, want, [(1, 2), (4, 0)], "repeated and refused, asked")
        _same(out, M.connect(S, recs, **kw), [(3, 2)], "repeated, enumerated")
        v = eng.connect([5, 3])
        assert v.status.tolist() == [SGO_ERR_STATE, 0] and (v.groups[0] == -1).all() and v.n_pairs[0] == 0
        # the refusals: a slot outside the context, a bound, a NULL output; n == 0 is a no-op
        one = np.array([8], np.int32)
        P = [L.ptr(o) for o in out]
        args = lambda **q: [eng.ctx, q.get("n", 1), L.ptr(q.get("slots", listed)), None, None, q.get("rules", 1), q.get("libs", 1),   # noqa: E731
                            q.get("region", 6), q.get("nodes", 64), q.get("pairs", T), L.ptr(status), q.get("o0", P[0]), q.get("o1", P[1]),
                            q.get("o2", P[2]), q.get("o3", P[3]), q.get("o4", P[4]), L.stream_ptr()]
        for bad in (dict(slots=one), dict(rules=2), dict(libs=-1), dict(libs=5), dict(region=0), dict(region=33), dict(nodes=0), dict(nodes=32769),
                    dict(pairs=65), dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(o4=None), dict(n=-1)):
            assert lib.sgo_session_connect(*args(**bad)) == SGO_ERR_ARG, bad
        assert lib.sgo_session_connect(eng.ctx, 0, None, None, None, 1, 1, 6, 64, T, None, None, None, None, None, None, L.stream_ptr()) == 0
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
    """the 9x9 `chain3` position and a white stone played into a device session stone by stone: `sgo-connect`, with two vertices, with
    `inherited` and with a small budget, and `sgo-groups` are the model's text on the board the session shows"""
    from sejonggo_amd import connect as cn, gtp
    from sejonggo_amd.stub_nets import make_stub
    from tests.rollout_model import pack_boards
    S = 9
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    _, black, white, _, _, _, _ = [p for p in CC.positions(S) if p[0] == "chain3"][0]
    white = [S * S - 1]
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for c, pts in (("B", black), ("W", white)):
            for p in pts:
                assert e.parse_command("play %s %s" % (c, e._vertex(p))) == "=\n\n"
        rec = pack_boards(dev.board)
        a = (black[1], black[0])

        def model(ask=None, **kw):
            return M.connect(S, rec, ask=None if ask is None else [ask], **kw)

        def text(ask=None, **kw):
            return "\n".join(cn.format_pair(cn.Pair(*(int(x) for x in r)), e._vertex, S * S) for r in model(ask, **kw)["rows"][0])

        assert e.parse_command("sgo-connect") == "= " + text() + "\n\n" and text().count("\n") == 1 and text().count(" connected ") == 2
        assert e.parse_command("sgo-connect %s %s" % (e._vertex(a[0]), e._vertex(a[1]))) == "= " + text(a) + "\n\n" and text(a).count("\n") == 0
        assert e.parse_command("sgo-connect %s %s inherited nodes 5 cutlibs 2" % (e._vertex(a[1]), e._vertex(a[0]))) == \
            "= " + text(a, rules=0, max_nodes=5, cut_libs=2) + "\n\n"
        assert " unknown " in text(a, rules=0, max_nodes=5, cut_libs=2)
        assert e.parse_command("sgo-connect A9 B8") == "? no pair on A9 B8\n\n"
        m = model()
        want = cn.format_groups(S, m["groups"][0], set(black)) + "\nchains 4 groups 2 connected 2"
        board = want.split("\nchains")[0]                             # three black stones and the column letter A; one white stone
        assert e.parse_command("sgo-groups") == "= " + want + "\n\n" and board.count("A") == 4 and board.count("a") == 1
        assert {"sgo-connect", "sgo-groups"} <= set(e.parse_command("list_commands").split())
    finally:
        dev.close()
