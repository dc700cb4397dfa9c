"""GPU: interactive (session) slots of the device engine -- sgo_session_open / _play / _genmove, engine.SessionEngine and
gtp.DeviceSejongGoEngine -- against the reference's GTP session (tests/golden/gtp_S9.npz, recorded from sejonggo_nomodel.py) and
against the host engine gtp.SejongGoEngine, which the same golden pins.  Rounding-free stub nets, identity symmetry; after every
command the tree-block accounting is audited (tests/block_audit.py)."""
import functools

import numpy as np
import pytest

from tests import block_audit as BA
from tests.helpers import dict_tree_hash, load, name_of, sha8

pytestmark = pytest.mark.gpu

SGO_ERR_OCCUPIED, SGO_ERR_RANGE, SGO_ERR_STATE = -101, -102, -203


@pytest.fixture()
def env():
    from sejonggo_amd import _lib, symmetry
    from sejonggo_amd.conf import conf
    _lib.require_gpu()
    keep, keep_sym = dict(conf), list(symmetry.SYMMETRIES)
    symmetry.SYMMETRIES[:] = symmetry.SYMMETRIES[0:1]     # the host engine evaluates under the identity, too
    yield conf
    symmetry.SYMMETRIES[:] = keep_sym
    conf.clear()
    conf.update(keep)


def _tree_hash(tree):
    return dict_tree_hash(tree if tree else {'subtree': {}})


def _audit(eng):
    v = BA.audit(*BA.dump_engine(eng))
    assert v == [], v[:10]
    return v


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _golden():
    z = load("gtp_S9.npz")
    script, replies = name_of(z, "script").split("\n"), name_of(z, "replies").split("\x1e")
    assert len(script) == len(replies) == len(z["board_hash"])
    return z, script, replies


def _check_golden_command(z, i, cmd, board, tree):
    assert np.array_equal(sha8(board), z["board_hash"][i]), (i, cmd)
    assert board[0, 0, 0, -1] == z["to_play"][i], (i, cmd)
    if cmd.startswith("genmove") and int(z["n_nodes"][i]) > 0:
        h, nn = dict_tree_hash(tree)
        assert nn == int(z["n_nodes"][i]) and h == z["tree_hash"][i].tobytes(), (i, cmd)
    elif int(z["n_nodes"][i]) == 0:
        assert tree is None or not tree['subtree'], (i, cmd)


def test_reference_session_one_slot(env):
    """test_gtp_session_matches_reference on the device tree: replies, board and side to move after every command, the kept
    subtree after every genmove, and the evaluations consumed."""
    from sejonggo_amd import gtp
    from sejonggo_amd.stub_nets import make_stub
    z, script, replies = _golden()
    S = int(z["size"])
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': int(z["sims"]), 'ENERGY': int(z["energy"]), 'KOMI': float(z["komi"])})
    dev = gtp.DeviceSejongGoEngine(int(z["sims"]), net=make_stub("hash", S), size=S, energy=int(z["energy"]),
                                   komi=float(z["komi"]), symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        assert dev.model.name in e.name()
        for i, cmd in enumerate(script):
            assert e.parse_command(cmd) == replies[i], (i, cmd)
            _check_golden_command(z, i, cmd, dev.board, dev.mcts_tree)
        assert int(dev.engine.status.total_evals) == int(z["n_predict"])
        assert dev.move == 1 + sum(c.startswith(("play", "genmove")) for c in script)
    finally:
        dev.close()


def test_four_staggered_sessions_on_a_shared_pool(env):
    """Four sessions in one context replay the golden session, slot k starting k ticks late, so that holds, external moves and
    searches of different slots coincide; all due plays of a tick are ONE play call, all due genmoves ONE genmove call.
    24 private blocks per game are far fewer than a tree needs: overflow ids and pool returns carry the trees."""
    from sejonggo_amd import gtp
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.play import index2coord
    from sejonggo_amd.stub_nets import make_stub
    z, script, replies = _golden()
    S, G = int(z["size"]), 4
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': int(z["sims"]), 'ENERGY': int(z["energy"]), 'KOMI': float(z["komi"])})
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=G, sims=int(z["sims"]), energy=int(z["energy"]),
                        komi=float(z["komi"]), symmetry="identity", blocks_per_game=24, shared_blocks=640)
    text = gtp.GTPEngine(engine=object())                # vertex text and the commands that touch no game
    color = gtp.COLOR_TO_PLAYER
    backed = 0
    try:
        assert eng.pool_info()["private_per_game"] == 24 and eng.pool_info()["shared_blocks"] == 640
        eng.open(np.arange(G))
        for tick in range(len(script) + G - 1):
            due = [(k, tick - k) for k in range(G) if 0 <= tick - k < len(script)]
            reply = {}
            plays = [(k, i) for k, i in due if script[i].startswith("play")]
            gens = [(k, i) for k, i in due if script[i].startswith("genmove")]
            for k, i in due:
                if script[i] == "clear_board":
                    eng.open([k])
                    reply[k] = "=\n\n"
                elif (k, i) not in plays and (k, i) not in gens:
                    reply[k] = text.parse_command(script[i])
            if plays:
                xy = [text.parse_move(script[i].split()[2]) for _, i in plays]
                st = eng.play([k for k, _ in plays], [y * S + x for x, y in xy], [color[script[i].split()[1]] for _, i in plays])
                assert not st.any(), st
                reply.update({k: "=\n\n" for k, _ in plays})
            if gens:
                for (k, i), (a, _, _) in zip(gens, eng.genmove([k for k, _ in gens])):
                    assert color[script[i].split()[1]] == -eng.board(k)[0, 0, 0, -1]      # the mover asked for has moved
                    reply[k] = "= " + text.print_move(*index2coord(a, S)) + "\n\n"
            for k, i in due:
                assert reply[k] == replies[i], (tick, k, script[i])
                _check_golden_command(z, i, script[i], eng.board(k), eng.tree_dict(k))
            v = _audit(eng)
            backed = max(backed, v.stats["backed"])
        assert int(eng.status.total_evals) == G * int(z["n_predict"])
        assert backed > 24, backed                         # the trees did live on shared blocks
        # every shared block is accounted for: free, returned, or behind an overflow id of a slot (the audit's pool partition)
        pool, games = eng.pool_state(), [eng.block_state(k, blocks=False) for k in range(G)]
        held = sum(int((g["ovfMap"] >= 0).sum()) for g in games)
        assert pool["poolCtl"][0] + pool["poolCtl"][1] + held == 640
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- fuzz against the host engine
FUZZ_SEEDS = (301, 302, 303, 304, 305, 306)


class _Pair(object):
    """One device session and one host SejongGoEngine on the same stub net, driven command by command and compared after each."""

    def __init__(self, conf, S, E, sims, resign):
        from sejonggo_amd import gtp, predicting_queue_worker as pq
        from sejonggo_amd.play import game_init
        from sejonggo_amd.stub_nets import make_stub
        conf.update({'SIZE': S, 'MCTS_SIMULATIONS': sims, 'ENERGY': E, 'KOMI': 5.5, 'GPUs': [0]})
        self.S, self.A, self.pq = S, S * S + 1, pq
        net = make_stub("hash", S)
        pq.set_model_factory(lambda kind: net)
        self.host = gtp.SejongGoEngine(sims, game_init(S)[0], resign=resign)
        self.dev = gtp.DeviceSejongGoEngine(sims, net=net, resign=resign, size=S, energy=E, komi=5.5, symmetry="identity", n_games=1)
        self.eng = self.dev.engine
        self.follow = self.fresh = self.resigned = 0
        self.check("open")

    def close(self):
        self.dev.close()
        self.pq.set_model_factory(None)
        self.pq.destroy_predicting_workers([0])

    def check(self, what):
        assert np.array_equal(self.dev.board, self.host.board), what
        assert self.dev.player == self.host.player and self.dev.move == self.host.move, what
        assert _tree_hash(self.dev.mcts_tree) == _tree_hash(self.host.mcts_tree), what
        _audit(self.eng)

    def xy(self, a):
        return a % self.S, a // self.S

    def most_visited(self):
        """the root's most visited child that was evaluated (the follow path), or None"""
        t = self.host.mcts_tree
        kids = [(c['count'], a) for a, c in (t['subtree'].items() if t else []) if c['subtree']]
        return max(kids)[1] if kids else None

    def play(self, a, color=None, what="play"):
        """color None: the side to move"""
        t = self.host.mcts_tree
        to_play = int(self.host.board[0, 0, 0, -1])
        in_turn = color is None or color == to_play
        followed = bool(in_turn and t and a in t['subtree'] and t['subtree'][a]['subtree'])
        x, y = self.xy(a)
        self.host.play(to_play if color is None else color, x, y)
        self.dev.play(0 if color is None else color, x, y)
        if not in_turn:
            self.host.mcts_tree = None                   # the documented deviation: the device drops the tree
        elif followed:
            self.follow += 1
            assert self.dev.mcts_tree['subtree'], what
        else:
            self.fresh += 1
            assert not self.dev.mcts_tree['subtree'], what
        self.check((what, a, color))

    def occupied(self, a):
        before, board, th = self.eng.block_state(0), self.dev.board, _tree_hash(self.dev.mcts_tree)
        assert self.eng.play([0], [a]).tolist() == [SGO_ERR_OCCUPIED]
        with pytest.raises(ValueError):
            self.dev.play(0, *self.xy(a))
        _same_state(before, self.eng.block_state(0))
        assert np.array_equal(board, self.dev.board) and th == _tree_hash(self.dev.mcts_tree)
        self.check(("occupied", a))

    def genmove(self):
        c = int(self.host.board[0, 0, 0, -1])
        hx, hy, hp, hv, _, _ = self.host.genmove(c)
        dx, dy, dp, dv, _, _ = self.dev.genmove(c)
        assert (dx, dy) == (hx, hy), "genmove"
        assert np.float32(dv).tobytes() == np.float32(np.asarray(hv).reshape(-1)[0]).tobytes()
        if hy == self.S + 1:
            self.resigned += 1                           # the host hands back the raw policy there, the device a zero row
            assert not np.asarray(dp).any()
        else:
            assert np.asarray(dp, np.float64).tobytes() == np.asarray(hp, np.float64).tobytes()
        self.check(("genmove", hx, hy))


@functools.lru_cache(maxsize=None)
def _fuzz_case(seed):
    """Runs one fuzzed script; (follow, fresh, resign) counted by the HOST engine's rules."""
    from sejonggo_amd.conf import conf
    rng = np.random.RandomState(seed)
    S = int(rng.choice([5, 7]))
    E = int(rng.choice([1, 4, 8]))
    sims = E * int(rng.randint(2, 6)) + int(rng.randint(0, E))
    resign = None if rng.rand() < 0.4 else float(rng.uniform(-1, 0.5))
    n_cmd = 14
    at_occupied, at_color = (int(v) for v in rng.choice(np.arange(3, n_cmd), size=2, replace=False))
    p = _Pair(conf, S, E, sims, resign)
    try:
        for i in range(n_cmd):
            stones = np.flatnonzero(p.host.board[0, :, :, :2].any(axis=-1).reshape(-1))
            empty = np.flatnonzero(~p.host.board[0, :, :, :2].any(axis=-1).reshape(-1))
            if i == at_occupied and len(stones):
                p.occupied(int(rng.choice(stones)))
                continue
            if i == at_color and len(empty):
                p.play(int(rng.choice(empty)), color=-int(p.host.board[0, 0, 0, -1]), what="out of turn")
                continue
            kind = rng.choice(["genmove", "empty", "visited", "pass"], p=[0.4, 0.2, 0.3, 0.1])
            best = p.most_visited()
            if kind == "visited" and best is not None:
                p.play(best, what="visited")
            elif kind == "empty" and len(empty):
                p.play(int(rng.choice(empty)), what="empty")
            elif kind == "pass":
                p.play(S * S, what="pass")
            else:
                p.genmove()
        return p.follow, p.fresh, p.resigned
    finally:
        p.close()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzzed_sessions_device_equals_host(env, seed):
    """14 random commands per case -- genmove, play on an empty point, play of the host root's most visited child (the follow
    path), pass, one play on an occupied point (refused, nothing changes), one out-of-turn colour (the documented deviation: the
    host's tree is dropped by hand) -- on the device session and on gtp.SejongGoEngine; boards, moves, values, policy targets and
    tree hashes agree after every command and the block accounting stays exact."""
    _fuzz_case(seed)


def test_fuzz_reaches_follow_fresh_and_resign(env):
    """A condition on the cases, counted by the host path's rules: over the six seeds at least 6 plays follow into an evaluated
    child, at least 6 start a fresh tree, and at least one genmove resigns."""
    counts = np.array([_fuzz_case(seed) for seed in FUZZ_SEEDS])
    follow, fresh, resigned = counts.sum(axis=0)
    print("SESSION_FUZZ follow=%d fresh=%d resign=%d per seed %s" % (follow, fresh, resigned, counts.tolist()))
    assert follow >= 6 and fresh >= 6 and resigned >= 1, counts.tolist()


def test_19x19_follow(env):
    """The multi-word rows of Geo<19>: play B, genmove W, play B onto the most visited child (follow), genmove W."""
    p = _Pair(env, 19, 8, 24, None)
    try:
        p.play(3 * 19 + 15, what="first")
        p.genmove()
        best = p.most_visited()
        assert best is not None
        p.play(best, what="visited")
        assert p.follow == 1
        p.genmove()
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------- a root on a shared block
ROOT_MAX_MOVES = 6


def test_root_on_a_shared_block_keys_tactics_rollout_sources(env):
    """The overflow arm of the root look-up behind sgo_session_keys, sgo_session_tactics and sgo_rollout_start_sessions: 5x5, two
    sessions, the smallest private region a context takes (energy + 2 = 6 blocks) beside a shared pool.  Slot 0 plays genmoves
    until its root has an overflow id (root_blk >= 6: after the SECOND genmove with this net and 16 simulations, on id 9; at most
    ROOT_MAX_MOVES are allowed and the test fails if none gets there), slot 1 keeps its root on block 0 as the control.  Listed in
    one call each, both slots give what sgo_keys and sgo_tactics give for the board sgo_game_board shows, and the rollout's
    source records -- read through the pointer sgo_rollout_list hands out -- are that board."""
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine, unpack_positions
    from sejonggo_amd.rollout import RolloutEngine
    from sejonggo_amd.stub_nets import make_stub
    from tests import rollout_model as M
    S, E, sims, mc = 5, 4, 16, 16
    net = make_stub("hash", S)
    eng = SessionEngine(net, size=S, n_games=2, sims=sims, energy=E, komi=5.5, symmetry="identity", blocks_per_game=E + 2,
                        shared_blocks=400)
    rol = RolloutEngine(net, size=S, max_rollouts=4, max_sources=2)
    try:
        lib = L.require_gpu()
        cap = eng.pool_info()["private_per_game"]
        assert cap == E + 2 and eng.pool_info()["shared_blocks"] == 400
        eng.open([0, 1])
        assert not eng.play([1], [7]).any()                # a fresh tree: the root is block 0
        moves = 0
        while eng.block_state(0, blocks=False)["root_blk"] < cap and moves < ROOT_MAX_MOVES:
            (a, _, _), = eng.genmove([0])
            assert 0 <= a <= S * S
            moves += 1
        roots = [eng.block_state(s, blocks=False)["root_blk"] for s in (0, 1)]
        print("ROOT_ON_SHARED_BLOCK moves=%d root_blk=%s private=%d" % (moves, roots, cap))
        assert roots[0] >= cap and roots[1] == 0, (moves, roots)
        _audit(eng)
        slots = np.array([0, 1], np.int32)
        boards = np.concatenate([eng.board(s) for s in slots])
        assert boards[0, :, :, :2].any() and boards[1, :, :, :2].any()
        rows = np.ascontiguousarray(M.pack_boards(boards), dtype=np.uint32)
        # keys
        k0, cn, mk = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.int32)
        assert lib.sgo_keys(S, 2, L.ptr(rows), None, L.ptr(k0), L.ptr(cn), L.ptr(mk), None) == 0
        got = eng.keys(slots)
        assert not got["status"].any() and k0[0] != k0[1]
        assert np.array_equal(got["key0"], k0) and np.array_equal(got["canon"], cn) and np.array_equal(got["mask"], mk)
        # tactics
        libs, nc, chains = np.zeros((2, S * S), np.uint8), np.zeros(2, np.int32), np.zeros((2, mc, 8), np.int32)
        assert lib.sgo_tactics(S, 2, L.ptr(rows), mc, L.ptr(libs), L.ptr(nc), L.ptr(chains)) == 0
        t = eng.tactics(slots, max_chains=mc)
        assert not t.status.any() and libs[0].any() and libs[1].any()
        assert np.array_equal(t.libs, libs) and np.array_equal(t.n_chains, nc) and np.array_equal(t.chains, chains)
        # rollout sources: sgo_rollout_start_sessions, then the records behind sgo_rollout_list
        assert rol.start_sessions(eng, slots, per_src=2, seed=3, max_plies=8) == 2
        assert list(rol.session_status) == [0, 0]
        src = rol.source_records(2, 2)
        assert np.array_equal(unpack_positions(src, S), boards)
        NW = lib.sgo_plane_words(S)
        assert np.array_equal(src[:, :2 * NW], rows[:, :2 * NW])         # stones and the to-play bit, word for word
        assert all(np.array_equal(eng.board(s), boards[i:i + 1]) for i, s in enumerate(slots))
        assert [eng.block_state(s, blocks=False)["root_blk"] for s in (0, 1)] == roots
    finally:
        rol.close()
        eng.close()


# ---------------------------------------------------------------------------------------------- a mixed context
def _mixed_games(eng, noises, uni):
    eng.start_games([0, 1], noises=noises, uniforms=uni)


def _run(eng, audit=False):
    """steps until no game is active, draining as it goes (the record buffer holds 2 * n_games + 16 moves)"""
    while True:
        st = eng.step()
        if st.n_records:
            eng.drain()
        if audit:
            _audit(eng)
        if not st.n_active:
            return


def _finished(eng, slots):
    eng.drain()
    res = eng.results(slots)
    out = []
    for s, r in zip(slots, res):
        moves = [(m['move_n'], m['action'], m['player'], np.float32(m['value']).tobytes(), m['policy'].tobytes(), m['packed'].tobytes())
                 for m in eng.records[s]]
        out.append((moves, r.tobytes()))
    return out


def test_session_beside_ordinary_games(env):
    """5x5, slots 0 and 1 play self-play games with fixed noise and draws while slot 2 is a session driven between the steps:
    the two games' records and results equal, byte for byte, those of the same games in a context without the session slot.
    Misuse is refused and changes nothing: session calls on an ordinary game, genmove on a searching session, actions outside
    [0, A)."""
    from sejonggo_amd import _lib
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    S, sims, E, nm = 5, 24, 4, 14
    A = S * S + 1
    rng = np.random.RandomState(77)
    noises, uni = rng.dirichlet([0.03] * A, size=2), rng.random_sample((2, nm))
    kw = dict(size=S, sims=sims, energy=E, stop_exploration=4, num_moves=nm, komi=5.5, symmetry="identity", self_play=True)
    ref = SessionEngine(make_stub("hash", S), n_games=2, **kw)
    try:
        _mixed_games(ref, noises, uni)
        _run(ref)
        want = _finished(ref, [0, 1])
    finally:
        ref.close()
    assert all(len(m) > 4 for m, _ in want)

    eng = SessionEngine(make_stub("hash", S), n_games=3, **kw)
    try:
        eng.open([2])
        _mixed_games(eng, noises, uni)
        eng.step()
        eng.step()
        _audit(eng)
        # session calls on a running ordinary game
        before = eng.block_state(0)
        assert eng.play([0, 2], [3, 7]).tolist() == [SGO_ERR_STATE, 0]
        with pytest.raises(_lib.SgoError):
            eng.arm([0])
        with pytest.raises(_lib.SgoError):
            eng.arm([2, 0])                               # ... and then nothing is armed, slot 2 included
        with pytest.raises(_lib.SgoError):
            eng.open([0])
        _same_state(before, eng.block_state(0))
        assert eng.block_state(2, blocks=False)["phase"] == 4
        # an action outside [0, A)
        before = eng.block_state(2)
        assert eng.play([2], [A]).tolist() == [SGO_ERR_RANGE] and eng.play([2], [-1]).tolist() == [SGO_ERR_RANGE]
        _same_state(before, eng.block_state(2))
        eng.step()
        # genmove on a session that is already searching
        eng.arm([2])
        eng.step()
        eng.step()
        before = eng.block_state(2)
        assert before["phase"] in (1, 2)
        with pytest.raises(_lib.SgoError):
            eng.arm([2])
        assert eng.play([2], [0]).tolist() == [SGO_ERR_STATE]
        _same_state(before, eng.block_state(2))
        (a, v, pol), = eng.wait([2])
        assert 0 <= a < A and pol.shape == (A,) and pol.any()
        _audit(eng)
        # the session never adds noise although the context's ordinary games do: its root priors are the net's, in float32
        assert np.array_equal(pol, pol.astype(np.float32).astype(np.float64))
        best = int(np.argmax(eng.root_table(2)["N"]))
        assert eng.play([2], [best]).tolist() == [0]
        eng.genmove([2])
        _audit(eng)
        _run(eng, audit=True)
        assert _finished(eng, [0, 1]) == want
        assert eng.results([2])[0]["done"] == 0 and eng.block_state(2, blocks=False)["phase"] == 4
        # sgo_start_games turns the session slot back into an ordinary game
        eng.start_games([2], noises=noises[:1], uniforms=uni[:1])
        with pytest.raises(_lib.SgoError):
            eng.arm([2])
        _run(eng)
        _audit(eng)
        (moves, res), = _finished(eng, [2])
        assert moves == want[0][0] and eng.results([2])[0]["done"] == 1
    finally:
        eng.close()
