"""GPU: search-only analysis and reports on session slots -- sgo_session_analyze / sgo_session_report, engine.SessionEngine
.analyze / .report, gtp.DeviceSejongGoEngine.analyze / .undo -- against the host engine gtp.SejongGoEngine with its `analyze`
(the comparator: root prediction, new_tree when there is no tree, select_play's simulation loop with the move discarded), which
the reference's GTP golden pins through the same search code.  Rounding-free stub net, identity symmetry; after every command
the tree-block accounting is audited (tests/block_audit.py)."""
import functools

import numpy as np
import pytest

from tests.helpers import load
from tests.test_gpu_session import _Pair, _audit, _finished, _mixed_games, _run, _same_state, _tree_hash

pytestmark = pytest.mark.gpu

SGO_ERR_STATE, SGO_ACTION_ANALYSIS = -203, -2
TOP, DEPTH = 5, 8


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


# ---------------------------------------------------------------------------------------------- the report, walked in Python
def _order(children):
    """the children of a dict node in select_play's temperature-0 order: count, then mean, then the HIGHER index; best first"""
    return sorted(children.items(), key=lambda kv: (kv[1]['count'], kv[1]['mean_value'], kv[0]), reverse=True)


def _walk(tree, top, depth):
    """(top_action [top], pv [top][depth], ties) from a tree_dict: the rule of sgo_session_report written out.  ties = pairs of
    neighbours among the top children that have the same count (decided by mean or index)."""
    top_action, pv = np.full(top, -1, np.int32), np.full((top, depth), -1, np.int32)
    ranked = _order(tree['subtree'])[:top]
    ties = sum(1 for (_, a), (_, b) in zip(ranked, ranked[1:]) if a['count'] == b['count'])
    for k, (a, node) in enumerate(ranked):
        top_action[k] = a
        line = [a]
        while len(line) < depth and node['subtree']:
            m, child = _order(node['subtree'])[0]
            if child['count'] <= 0:
                break
            line.append(m)
            node = child
        pv[k, :len(line)] = line[:depth]
    return top_action, pv, ties


def _check_report(eng, slot, top=TOP, depth=DEPTH):
    """report(slot) against root_table and the Python walk; returns (pvs of length >= 3, ties among the top children)"""
    r = eng.report([slot], top=top, depth=depth)
    t, tree = eng.root_table(slot), eng.tree_dict(slot)
    ex = t["EX"].astype(bool)
    assert r["status"][0] == 0
    assert np.array_equal(r["N"][0], np.where(ex, t["N"], -1))
    assert r["Q"][0].tobytes() == np.where(ex, t["Q"], np.float32(0)).astype(np.float32).tobytes()
    assert r["P"][0].tobytes() == np.where(ex, t["P"], 0).astype(np.float32).tobytes()
    assert r["root_count"][0] == t["root_count"] and r["root_value"][0].tobytes() == np.float32(t["root_value"]).tobytes()
    assert r["n_children"][0] == int(ex.sum()) and r["to_play"][0] == eng.board(slot)[0, 0, 0, -1]
    if t["root_count"]:
        assert r["root_mean"][0].tobytes() == np.float32(t["root_value"] / np.float32(t["root_count"])).tobytes()
    want_top, want_pv, ties = _walk(tree, top, depth)
    assert np.array_equal(r["top_action"][0], want_top), (r["top_action"][0], want_top)
    assert np.array_equal(r["pv"][0], want_pv), (r["pv"][0], want_pv)
    return int(((want_pv >= 0).sum(axis=1) >= 3).sum()), ties


# ---------------------------------------------------------------------------------------------- fuzz against the host engine
FUZZ_SEEDS = (401, 402, 403, 404, 405, 406)


class _PairA(_Pair):
    """_Pair with analyze and undo.  `hist` mirrors the device engine's move list for the host's undo; `analysed` is true while
    the tree is one that an analysis searched (kept through plays that follow into it, cleared when the tree is dropped or a
    genmove has searched it)."""

    def __init__(self, *a):
        self.hist, self.analysed = [], False
        self.n_unexpanded = self.n_deepen = self.n_gen_on_analysed = self.n_follow_analysed = self.n_undo = 0
        super(_PairA, self).__init__(*a)

    def _has_tree(self):
        t = self.host.mcts_tree
        return bool(t and t['subtree'])

    def play(self, a, color=None, what="play"):
        to_play = int(self.host.board[0, 0, 0, -1])
        follow0 = self.follow
        super(_PairA, self).play(a, color=color, what=what)
        self.hist.append((a, to_play if color is None else color))
        if self.follow > follow0:
            self.n_follow_analysed += 1 if self.analysed else 0
        else:
            self.analysed = False
        assert [m for m, _ in self.dev.moves] == [m for m, _ in self.hist], what

    def genmove(self):
        c, resigned0, on_analysed = int(self.host.board[0, 0, 0, -1]), self.resigned, self.analysed and self._has_tree()
        move0 = self.host.move
        super(_PairA, self).genmove()
        if self.resigned == resigned0:
            assert self.host.move == move0 + 1
            self.hist.append((int(self.dev.moves[-1][0]), c))
            self.n_gen_on_analysed += 1 if on_analysed else 0
            self.analysed = False
        assert len(self.dev.moves) == len(self.hist)

    def analyze(self, sims):
        had_tree = self._has_tree()
        board, move = self.dev.board, self.dev.move
        hp, hv = self.host.analyze(sims)
        dp, dv = self.dev.analyze(sims)
        assert np.float32(dv).tobytes() == np.float32(np.asarray(hv).reshape(-1)[0]).tobytes()
        want = np.zeros(self.A)
        for a, child in self.host.mcts_tree['subtree'].items():
            want[a] = child['p']                              # the row a genmove from this root records (policy_target)
        assert np.asarray(dp, np.float64).tobytes() == want.tobytes()
        assert np.array_equal(board, self.dev.board) and move == self.dev.move
        self.n_unexpanded += 0 if had_tree else 1
        self.n_deepen += 1 if had_tree else 0
        self.analysed = True
        self.check(("analyze", sims))

    def undo(self):
        from sejonggo_amd.play import game_init
        if not self.hist:
            with pytest.raises(ValueError):
                self.dev.undo()
            return False
        self.dev.undo()
        self.hist.pop()
        h = self.host
        h.board, h.player = game_init(self.S)
        h.mcts_tree, h.move = None, 1
        for a, col in self.hist:
            h.play(col, *self.xy(a), update_tree=False)
        self.analysed = False
        self.n_undo += 1
        assert not self.dev.mcts_tree['subtree']
        self.check("undo")
        return True


@functools.lru_cache(maxsize=None)
def _fuzz_case(seed):
    """One fuzzed script.  It opens with analyze, analyze, play of the most visited child, genmove, undo -- so that every seed
    brings one case of each condition by construction -- and goes on with 9 random commands.  Four of the six seeds have no
    resign threshold, so their genmove on the analysed tree cannot resign.  The conditions of
    test_fuzz_reaches_every_kind_of_analysis are thus met by the fixed opening alone (the host path cannot be run without a GPU
    to pick seeds by); the random tail adds cases on top -- what it adds is in the printed ANALYSIS_FUZZ line -- and is there
    for the orders of commands the opening does not hold.  Returns the counters and the report figures."""
    from sejonggo_amd.conf import conf
    rng = np.random.RandomState(seed)
    S = int(rng.choice([5, 7]))
    E = int(rng.choice([1, 4, 8]))
    sims = E * int(rng.randint(2, 6)) + int(rng.randint(0, E))
    resign = None if seed % 3 else float(rng.uniform(-1, 0.5))
    script = ["analyze", "analyze", "visited", "genmove", "undo"]
    script += list(rng.choice(["analyze", "genmove", "visited", "empty", "pass", "undo"], size=9, p=[0.3, 0.2, 0.2, 0.1, 0.05, 0.15]))
    p = _PairA(conf, S, E, sims, resign)
    try:
        for kind in script:
            empty = np.flatnonzero(~p.host.board[0, :, :, :2].any(axis=-1).reshape(-1))
            best = p.most_visited()
            if kind == "analyze":
                p.analyze(None if rng.rand() < 0.25 else E * int(rng.randint(1, 5)))
            elif kind == "visited" and best is not None:
                p.play(best, what="visited")
            elif kind == "empty" and len(empty):
                p.play(int(rng.choice(empty)), what="empty")
            elif kind == "pass":
                p.play(S * S, what="pass")
            elif kind == "undo" and p.undo():
                pass
            else:
                p.genmove()
        # the final state, searched once more so that it holds a tree, for the report
        p.analyze(E * 6)
        long_pv, ties = _check_report(p.eng, 0)
        return (p.n_unexpanded, p.n_deepen, p.n_gen_on_analysed, p.n_follow_analysed, p.n_undo), (long_pv, ties)
    finally:
        p.close()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzzed_analysis_device_equals_host(env, seed):
    """14 commands per case -- analyze, analyze again, genmove, play of the most visited child, play elsewhere, pass, undo -- on
    the device session and on gtp.SejongGoEngine: boards, move numbers, tree hashes after every command, value and prior row of
    every analysis, move, value and policy row of every genmove agree; the block accounting stays exact; the report of the final
    state equals root_table and a Python walk over tree_dict."""
    _fuzz_case(seed)


def test_fuzz_reaches_every_kind_of_analysis(env):
    """Conditions on the cases, counted by the host engine's rules: over the six seeds at least 6 analyses start from an
    unexpanded root, 6 deepen a tree, 4 genmoves run on an analysed tree, 4 plays follow into one, and 3 undos happen."""
    counts = np.array([_fuzz_case(seed)[0] for seed in FUZZ_SEEDS])
    un, deep, gen, follow, undo = counts.sum(axis=0)
    print("ANALYSIS_FUZZ unexpanded=%d deepen=%d genmove_on_analysed=%d follow_into_analysed=%d undo=%d per seed %s"
          % (un, deep, gen, follow, undo, counts.tolist()))
    assert un >= 6 and deep >= 6 and gen >= 4 and follow >= 4 and undo >= 3, counts.tolist()


# ---------------------------------------------------------------------------------------------- the 19x19 report
@functools.lru_cache(maxsize=None)
def _report_19():
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    z = load("sgf_S19.npz")
    S = int(z["size"])
    mv = z["g01_moves"][:150]
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=2, sims=24, energy=8, komi=float(z["komi"]), symmetry="identity")
    try:
        eng.open([0, 1])
        status, _ = eng.setup([0], [[S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv]], [[int(c) for _, _, c in mv]])
        assert not status.any()
        eng.analyze([0], 24)
        _audit(eng)
        figures = _check_report(eng, 0)
        # a slot that does not hold: its status says so and its rows keep what the caller filled in
        eng.arm_analysis([1], 24)
        eng.step()
        out = eng.report([0], top=TOP, depth=DEPTH)
        both = {k: np.concatenate([np.full_like(v, -7), v]) for k, v in out.items()}
        eng.report_into([1, 0], both)
        assert both["status"].tolist() == [SGO_ERR_STATE, 0]
        for k, v in both.items():
            if k != "status":
                assert (v[0] == -7).all(), k
                assert v[1].tobytes() == out[k][0].tobytes(), k
        eng.wait([1], 24)
        return figures
    finally:
        eng.close()


def test_report_19x19_and_a_slot_that_does_not_hold(env):
    """Setup to ply 150 of golden game 1, 24 simulations at energy 8: the report equals root_table and the Python walk; a
    searching slot in the same call gets SGO_ERR_STATE and keeps its sentinel rows."""
    _report_19()


def test_reports_reach_long_lines_and_ties(env):
    """Condition on the report cases (the six fuzz finals and the 19x19 one): at least 5 principal variations of 3 or more
    moves, and at least one tie on count among the top children that the mean or the index decides."""
    figs = [_fuzz_case(seed)[1] for seed in FUZZ_SEEDS] + [_report_19()]
    long_pv, ties = np.array(figs).sum(axis=0)
    print("ANALYSIS_REPORT pv_of_3_or_more=%d ties_on_count=%d per case %s" % (long_pv, ties, figs))
    assert long_pv >= 5 and ties >= 1, figs


# ---------------------------------------------------------------------------------------------- additivity, search-only
def _session(S=5, G=2, sims=16, E=4, **kw):
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    return SessionEngine(make_stub("hash", S), size=S, n_games=G, sims=sims, energy=E, komi=5.5, symmetry="identity", **kw)


def _record_of(eng, slot):
    """steps until the armed slot has written its record; the whole record"""
    for _ in range(400):
        if eng.step().n_records:
            eng.drain()
        if eng.records.get(slot):
            return eng.records[slot].pop(0)
    raise AssertionError("no record")


@pytest.mark.parametrize("S,E,a,b", [(5, 4, 8, 12), (7, 8, 8, 16), (5, 1, 3, 4)])
def test_analyses_add_up(env, S, E, a, b):
    """E | a and E | b: analyze(a) then analyze(b) leaves the tree and the child tables of one analyze(a + b) on a twin slot, and
    costs exactly one evaluation more (the second root evaluation)."""
    eng = _session(S=S, E=E, sims=4 * E)
    try:
        eng.open([0, 1])
        lists = [[S + 1, 2 * S + 3, S * S, 3]] * 2
        assert not eng.setup([0, 1], lists)[0].any()
        t0 = int(eng.status.total_evals)
        eng.analyze([0], a)
        _audit(eng)
        eng.analyze([0], b)
        t1 = int(eng.status.total_evals)
        eng.analyze([1], a + b)
        t2 = int(eng.status.total_evals)
        _audit(eng)
        assert (t1 - t0) - (t2 - t1) == 1 and t2 - t1 <= 1 + a + b
        assert eng.tree_serialize(0)[0].tobytes() == eng.tree_serialize(1)[0].tobytes()
        r = eng.report([0, 1], top=TOP, depth=DEPTH)
        for k, v in r.items():
            assert v[0].tobytes() == v[1].tobytes(), k
        assert r["root_count"][0] == a + b
    finally:
        eng.close()


def test_analysis_is_search_only(env):
    """Board, move number and side to move stay; the record has action -2, the root's value and the prior row; a resign threshold
    of +1.0 does not stop an analysis, the genmove that follows resigns and leaves the tree as it was; misuse raises and arms
    nothing."""
    from sejonggo_amd import _lib
    S, E = 5, 4
    A = S * S + 1
    eng = _session(S=S, G=4, sims=16, E=E, self_play=True)
    try:
        eng.open([0, 1], resign=1.0)
        eng.open([2])
        assert not eng.setup([0, 1, 2], [[6, 7, 8]] * 3)[0].any()
        board = eng.board(0)
        eng.arm_analysis([0], 12)
        rec = _record_of(eng, 0)
        _audit(eng)
        assert rec['action'] == SGO_ACTION_ANALYSIS and rec['move_n'] == 3 and rec['player'] == 1      # black moved last
        assert np.array_equal(board, eng.board(0)) and eng.block_state(0, blocks=False)["phase"] == 4
        r = eng.report([0], top=TOP, depth=DEPTH)
        assert r["root_count"][0] == 12 and r["to_play"][0] == board[0, 0, 0, -1]
        # the value is the net's on the root, the row the root's priors: what a genmove of the twin without a threshold records
        eng.arm([2])
        gen = _record_of(eng, 2)
        assert gen['action'] >= 0 and gen['move_n'] == 3
        assert np.float32(rec['value']).tobytes() == np.float32(gen['value']).tobytes()
        assert rec['policy'].tobytes() == gen['policy'].tobytes() and rec['packed'].tobytes() == gen['packed'].tobytes()
        # the threshold of +1.0 is still there: genmove resigns, and the analysed tree stays as it is
        tree = eng.tree_serialize(0)[0].tobytes()
        state = eng.block_state(0)
        eng.arm([0])
        res = _record_of(eng, 0)
        assert res['action'] == -1 and not res['policy'].any() and res['move_n'] == 3
        assert eng.tree_serialize(0)[0].tobytes() == tree and np.array_equal(board, eng.board(0))
        _same_state(state, eng.block_state(0))
        # setup keeps the threshold, too
        assert not eng.setup([1], [[6]])[0].any()
        assert eng.genmove([1])[0][0] == -1
        # misuse: an ordinary game, a searching session, fewer simulations than a round
        rng = np.random.RandomState(3)
        eng.start_games([3], noises=rng.dirichlet([0.03] * A, size=1), uniforms=rng.random_sample((1, 2 * S * S)))
        eng.step()
        eng.arm_analysis([2], 8)
        eng.step()
        eng.step()
        s0, s2, s3 = eng.block_state(0), eng.block_state(2), eng.block_state(3)
        assert s2["phase"] in (1, 2)
        for bad in ([3], [0, 3], [2], [0, 2]):
            with pytest.raises(_lib.SgoError):
                eng.arm_analysis(bad, 8)
        with pytest.raises(_lib.SgoError) as e:
            eng.arm_analysis([0], E - 1)
        assert "(-1)" in str(e.value)
        _same_state(s0, eng.block_state(0))
        _same_state(s2, eng.block_state(2))
        _same_state(s3, eng.block_state(3))
        assert eng.block_state(0, blocks=False)["phase"] == 4                 # slot 0 was armed by none of the refused calls
        assert eng.wait([2], 8)[0][0] == SGO_ACTION_ANALYSIS
        _audit(eng)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- a mixed context
def test_analysis_beside_ordinary_games(env):
    """test_session_beside_ordinary_games' byte-for-byte check with slot 2 doing setup / analyze / report between the steps of
    two self-play games: their records and results are those of the same games in a context without the session slot."""
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
        assert not eng.setup([2], [[12, 7, 11]])[0].any()
        eng.step()
        _audit(eng)
        eng.analyze([2], 8)
        _audit(eng)
        assert eng.report([2])["root_count"][0] == 8
        eng.step()
        eng.analyze([2])                                   # the context's 24 simulations on top
        r = eng.report([2], top=TOP, depth=DEPTH)
        assert r["root_count"][0] == 8 + sims and r["status"][0] == 0
        _check_report(eng, 2)
        assert not eng.setup([2], [[12, 7]])[0].any()
        eng.genmove([2])
        _audit(eng)
        _run(eng, audit=True)
        assert _finished(eng, [0, 1]) == want
        assert eng.results([2])[0]["done"] == 0 and eng.block_state(2, blocks=False)["phase"] == 4
    finally:
        eng.close()
