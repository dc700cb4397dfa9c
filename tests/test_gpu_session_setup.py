"""GPU: sgo_session_setup / engine.SessionEngine.setup -- a session slot set to a position in one launch -- against the
reference's game records (tests/golden/sgf_S19.npz: board hashes and legal masks after every ply), against the chain of
sgo_session_play calls it stands for, and for its atomic refusal and its pool accounting.  Rounding-free stub net, identity
symmetry; the tree-block accounting is audited after every command (tests/block_audit.py)."""
import numpy as np
import pytest

from tests import block_audit as BA
from tests.helpers import load, sha8, unpack_mask

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_OCCUPIED, SGO_ERR_RANGE, SGO_ERR_STATE = -1, -101, -102, -203


@pytest.fixture()
def env():
    from sejonggo_amd import _lib, symmetry
    from sejonggo_amd.conf import conf
    _lib.require_gpu()
    keep, keep_sym = dict(conf), list(symmetry.SYMMETRIES)
    symmetry.SYMMETRIES[:] = symmetry.SYMMETRIES[0:1]
    yield conf
    symmetry.SYMMETRIES[:] = keep_sym
    conf.clear()
    conf.update(keep)


def _audit(eng):
    v = BA.audit(*BA.dump_engine(eng))
    assert v == [], v[:10]
    return v


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _engine(S, G, **kw):
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    kw.setdefault("sims", 16)
    kw.setdefault("energy", 4)
    return SessionEngine(make_stub("hash", S), size=S, n_games=G, komi=5.5, symmetry="identity", **kw)


def _root_legal(eng, slot):
    """the legal bits of the slot's root block as a 0/1 vector of A entries"""
    st = eng.block_state(slot)
    words = st["legal"][st["root_blk"]]
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:eng.A]


def _golden_game(z, gi, S):
    p = "g%02d_" % gi
    mv = z[p + "moves"]
    actions = [S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv]
    colors = [int(c) for _, _, c in mv]
    return actions, colors, z[p + "hashes"], z[p + "masks"]


def _first_capture(z, gi):
    """the first ply of the record after which the board holds fewer stones than a ply before + 1"""
    S = int(z["size"])
    from sejonggo_amd import play
    board, _ = play.game_init(S)
    for ply, (x, y, c) in enumerate(z["g%02d_moves" % gi]):
        before = int(board[0, :, :, :2].sum())
        play.make_play(int(x), int(y), board, None if c == 0 else int(c))
        if int(y) < S and int(board[0, :, :, :2].sum()) < before + 1:
            return ply + 1                               # the position after `ply + 1` plies is the first with a capture
    raise AssertionError("no capture in the record")


def test_reference_positions(env):
    """8 slots set to prefixes of golden games 0 and 3 in ONE call -- lengths 0, 1, 8, 9 (the 8-ply history fills), the plies
    around the first capture, the middle and the full game: the board hash and the root's legal bits equal the reference's."""
    z = load("sgf_S19.npz")
    S = int(z["size"])
    cap0 = _first_capture(z, 0)
    g0, g3 = _golden_game(z, 0, S), _golden_game(z, 3, S)
    cases = [(g0, 0), (g3, 1), (g0, 8), (g3, 9), (g0, cap0 - 1), (g0, cap0), (g3, len(g3[0]) // 2), (g3, len(g3[0]))]
    eng = _engine(S, len(cases))
    try:
        slots = np.arange(len(cases))
        eng.open(slots)
        status, fail_at = eng.setup(slots, [g[0][:k] for g, k in cases], [g[1][:k] for g, k in cases])
        assert not status.any() and (fail_at == -1).all(), (status, fail_at)
        _audit(eng)
        for s, (g, k) in enumerate(cases):
            assert np.array_equal(sha8(eng.board(s)), g[2][k]), (s, k)
            # the record holds play.legal_moves' vector, which flags the ILLEGAL points
            assert np.array_equal(_root_legal(eng, s), 1 - unpack_mask(g[3][k], eng.A)), (s, k)
            st = eng.block_state(s, blocks=False)
            assert st["phase"] == 4 and st["free_top"] == st["L"] - 1
            assert not eng.tree_dict(s)['subtree']
    finally:
        eng.close()


def _random_list(rng, S, n):
    """passes, explicit colours, out-of-turn stones on a board tracked by the host rules, so that no point is occupied"""
    from sejonggo_amd import play
    board, _ = play.game_init(S)
    acts, cols = [], []
    for _ in range(n):
        to_play = int(board[0, 0, 0, -1])
        empty = np.flatnonzero(~board[0, :, :, :2].any(axis=-1).reshape(-1))
        r = rng.rand()
        if r < 0.12 or not len(empty):
            a = S * S
        else:
            a = int(rng.choice(empty))
        col = 0 if rng.rand() < 0.5 else (to_play if rng.rand() < 0.6 else -to_play)
        acts.append(a)
        cols.append(col)
        play.make_play(a % S if a < S * S else 0, a // S if a < S * S else S, board, None if col == 0 else col)
    return acts, cols


# black plays a1 into white's b1 + a2: a suicide, which make_play executes (the stone is removed again)
SUICIDE_5 = ([1, 12, 5, 13, 0], [-1, 1, -1, 1, 1])


@pytest.mark.parametrize("S,seed", [(5, 11), (7, 12)])
def test_equals_the_chain_of_plays(env, S, seed):
    """setup(list) and open + one play per move leave block_state and board equal in every array: seeded random lists with
    passes, explicit and out-of-turn colours, and a suicide."""
    rng = np.random.RandomState(seed)
    lists = [_random_list(rng, S, n) for n in (0, 1, 7, 9, 3 * S * S // 2)]
    if S == 5:
        lists.append(SUICIDE_5)
    G = len(lists)
    one, chain = _engine(S, G), _engine(S, G)
    try:
        slots = np.arange(G)
        one.open(slots, resign=-0.5)
        chain.open(slots, resign=-0.5)
        # a searched tree in one slot of both, so that setup has something to drop (free blocks keep their stale words, which
        # block_state dumps too: both engines have the same past)
        one.genmove([G - 1])
        chain.genmove([G - 1])
        status, fail_at = one.setup(slots, [a for a, _ in lists], [c for _, c in lists])
        assert not status.any(), (status, fail_at)
        chain.open(slots, resign=-0.5)
        for j in range(max(len(a) for a, _ in lists)):
            due = [s for s in range(G) if j < len(lists[s][0])]
            st = chain.play(due, [lists[s][0][j] for s in due], [lists[s][1][j] for s in due])
            assert not st.any(), (j, st)
        _audit(one)
        _audit(chain)
        for s in range(G):
            # min_free, the game's high-water mark, included: a slot that searched before its setup starts anew, as open does
            _same_state(one.block_state(s), chain.block_state(s))
            assert np.array_equal(one.board(s), chain.board(s)), s
        if S == 5:
            assert one.board(G - 1)[0, 0, 0, :2].sum() == 0            # the suicide stone is gone
        # move_n, player and the kept threshold, through the next command: a genmove resigns or moves alike
        ra, rb = one.genmove(slots), chain.genmove(slots)
        for (a1, v1, p1), (a2, v2, p2) in zip(ra, rb):
            assert a1 == a2 and np.float32(v1).tobytes() == np.float32(v2).tobytes() and p1.tobytes() == p2.tobytes()
        for s in range(G):
            assert np.array_equal(one.board(s), chain.board(s)), s
    finally:
        one.close()
        chain.close()


def test_atomic_refusal_and_pool_accounting(env):
    """9x9, 24 private blocks per game and a shared pool: slot 0 holds a searched tree on shared blocks.  Three setups that are
    refused (an occupied point at index j, an action of A + 3, a list for a slot that is searching / runs an ordinary game) leave
    it -- and the refused slot -- unchanged in every word while the other slots of the same call go through; a duplicate slot or
    an over-long list is SGO_ERR_ARG and changes nothing; a setup that goes through returns every shared block."""
    from sejonggo_amd import _lib
    S, G, POOL = 9, 4, 640
    A = S * S + 1
    eng = _engine(S, G, sims=64, energy=8, blocks_per_game=24, shared_blocks=POOL, self_play=True)
    try:
        eng.open([0, 1, 2])
        assert not eng.play([0], [40]).any()
        eng.analyze([0])
        _audit(eng)
        held = int((eng.block_state(0, blocks=False)["ovfMap"] >= 0).sum())
        assert held > 0                                               # the tree lives on shared blocks
        before0, board0 = eng.block_state(0), eng.board(0)
        # 1: an occupied point at index 3 for slot 0, slot 1 goes through
        status, fail_at = eng.setup([0, 1], [[0, 1, 2, 1, 5], [3, 4]])
        assert status.tolist() == [SGO_ERR_OCCUPIED, 0] and fail_at.tolist() == [3, -1]
        _same_state(before0, eng.block_state(0))
        assert np.array_equal(board0, eng.board(0))
        assert eng.board(1)[0, 0, 3, 1] == 1 or eng.board(1)[0, 0, 3, 0] == 1
        # 2: an action of A + 3 at index 1
        status, fail_at = eng.setup([1, 0], [[7], [0, A + 3]])
        assert status.tolist() == [0, SGO_ERR_RANGE] and fail_at.tolist() == [-1, 1]
        _same_state(before0, eng.block_state(0))
        # 3: a slot that runs an ordinary game, and a session that is searching
        rng = np.random.RandomState(5)
        eng.start_games([3], noises=rng.dirichlet([0.03] * A, size=1), uniforms=rng.random_sample((1, 2 * S * S)))
        eng.arm([2])
        eng.step()
        eng.step()
        b2, b3 = eng.block_state(2), eng.block_state(3)
        assert b2["phase"] in (1, 2) and b3["phase"] in (1, 2)
        status, fail_at = eng.setup([3, 1, 2], [[1], [9, 10, 11], [2]])
        assert status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE] and fail_at.tolist() == [-1, -1, -1]
        _same_state(b2, eng.block_state(2))
        _same_state(b3, eng.block_state(3))
        _same_state(before0, eng.block_state(0))
        assert eng.block_state(1, blocks=False)["phase"] == 4
        eng.wait([2])
        # a duplicate slot, an over-long list: SGO_ERR_ARG, nothing runs
        b1 = eng.block_state(1)
        with pytest.raises(_lib.SgoError):
            eng.setup([1, 1], [[0], [1]])
        with pytest.raises(_lib.SgoError):
            eng.setup([1], [[S * S] * (4 * S * S + 1)])
        _same_state(b1, eng.block_state(1))
        _same_state(before0, eng.block_state(0))
        status, _ = eng.setup([1], [[S * S] * (4 * S * S)])               # the cap itself is served
        assert status.tolist() == [0]
        _audit(eng)
        # pool accounting: the setup of slot 0 returns every shared block it held
        status, _ = eng.setup([0], [[40, 41]])
        assert status.tolist() == [0]
        _audit(eng)
        assert int((eng.block_state(0, blocks=False)["ovfMap"] >= 0).sum()) == 0
        pool, games = eng.pool_state(), [eng.block_state(k, blocks=False) for k in range(G)]
        assert pool["poolCtl"][0] + pool["poolCtl"][1] + sum(int((g["ovfMap"] >= 0).sum()) for g in games) == POOL
        # and the slot searches again from the new position
        a, _, pol = eng.genmove([0])[0]
        assert 0 <= a < A and pol[40] == 0 and pol[41] == 0
        _audit(eng)
    finally:
        eng.close()
