"""GPU: the engine step and the session calls in contexts of MORE THAN 1 024 game slots -- the regime in which k_compact's threads own
runs of several games (per = ceil(G / 1024): 2, 3 and 4 at G = 1 025, 2 050 and 3 073), k_session_arm's list walk takes a second
trip, and nothing else in the suite runs.  tests/compact_model.py is the plain model of the compaction;
tests/test_compact_model_power.py shows which of its fault switches need more than one game per thread and which need staggered
games.  All cases: 5x5, the rounding-free `hash` stub net, identity symmetry, thin searches (energy 4; 10 simulations and 3 plies for
self-play, so the last round of a move is short; 16 simulations for sessions).

  a  self-play against the oracle at G = 1 025, 2 050, 3 073: recorded draws per game, a resign threshold on about a third of the
     games, every third slot restarted with new draws the moment it finishes (as often as the draws last), so that games are out
     of step and root requests meet leaf requests; after EVERY step the evaluation list is read back and checked
  b  the same at G = 1 025 with 10 private blocks per game and the shared pool; pool accounting and one whole-context block audit
  c  status folds at G = 2 050: three chosen slots run out of draws; error_game, error, n_active, n_done
  d  1 100 sessions: open, setup, analyze, report, play, genmove -- each ONE call over a shuffled list of all slots -- against the
     host engine; the all-or-none rule of the arming with the one slot that does not hold in the second trip of the walk, then in
     the first

WHERE THE CASES DEPART FROM THEIR FIRST DESCRIPTION, because the numbers do not exist at these sizes.  The one workgroup gives
ceil(G / per) threads a run, the rest none: 513, 684 and 769 threads at the three sizes.  So threads 959 / 960 own no game at any of
them, and wave 11 none at G = 2 050 (684 threads are waves 0 .. 10).  The sampled runs therefore take, beside threads 63 / 64, the
two threads on either side of the start of the LAST wave that holds games (639 / 640 at 2 050, 767 / 768 at 3 073: the second is
the last thread, with its partial run), and case c puts its failing first-of-a-run game into wave 10, the last wave with games at
2 050 -- and adds a third failing slot, the game after the lower one in the same run, so that `two fail in one run` is a case too.
A failed game rests in PH_DONE until it is restarted, as a finished one does, so n_done counts both; the results tell them apart.

SLOTS CHECKED against the oracle in case a: all 1 025 (1 366 games with the restarts) at G = 1 025; at G = 2 050 680 slots (900 games)
(200 complete runs of 3 evenly spread, the runs of threads 63, 64, 639, 640, the last thread's one game, slots 0, 1 023, 1 024, 2 049 and
100 random ones) and at G = 3 073 892 slots (1 198 games; the same with runs of 4 and threads 767 / 768), each with every game it played.

Measured on MI355X (pytest --durations=0 of this module alone, 6 tests, 12.2 s together with 1.7 s of start-up in the first):
  3.05s test_sessions_in_one_call_each           2.62s test_selfplay_from_the_shared_pool
  2.12s test_selfplay_equals_the_oracle[1025]    1.24s test_selfplay_equals_the_oracle[3073]    0.92s test_selfplay_equals_the_oracle[2050]
  0.11s test_status_folds_over_runs_and_waves
Every population runs 20 steps (19 lists).  Steps on which restarted slots ask for their root while other games ask for leaves:
5, 7 and 7 at the three sizes; games of 0, 1, 2 and 3 moves among those checked: 80 / 143 / 50 / 1 093 at G = 1 025.  The three
chosen slots of case c fail on step 6 of 10, slot 601 first in the status.
"""
import numpy as np
import pytest

from tests import block_audit as BA
from tests import compact_model as M

pytestmark = pytest.mark.gpu

S, SIMS, E, NM, STOP = 5, 10, 4, 3, 2
A = S * S + 1
SGO_ERR_DRAWS, SGO_ERR_STATE, SGO_ACTION_ANALYSIS = -202, -203, -2
PH_DONE, PH_HOLD = 3, 4


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def _net():
    from sejonggo_amd.stub_nets import make_stub
    return make_stub("hash", S)


# ---------------------------------------------------------------------------------------------- which slots meet the oracle
def _last_wave_start(G):
    """the first thread of the last wave of the one workgroup that owns a game"""
    threads = -(-G // M.per_thread(G))
    return (threads - 1) // M.WAVE * M.WAVE


def _sample(G):
    """(slots sorted, complete runs among them): every slot at G = 1 025; above, the sample the module docstring describes"""
    per = M.per_thread(G)
    threads = -(-G // per)
    full = [t for t in range(threads) if t * per + per <= G]
    if G <= 1025:
        return np.arange(G), len(full)
    rng = np.random.RandomState(G)
    w = _last_wave_start(G)
    picked = set(full[int(i)] for i in np.linspace(0, len(full) - 1, 200)) | {63, 64, w - 1, w, threads - 1}
    slots = set([0, 1023, 1024, G - 1]) | set(int(s) for s in rng.choice(G, size=100, replace=False))
    for t in picked:
        slots |= set(range(*M.run_of(G, t)))
    assert all(t in picked for t in (63, 64, w - 1, w)) and M.run_of(G, threads - 1)[1] == G
    return np.array(sorted(slots)), len([t for t in picked if t in full])


class _Finished(object):
    """what _compare_with_oracle reads of an engine, kept per finished game (a restart replaces the slot's tree)"""

    def __init__(self):
        self.games, self.trees, self.tables, self.results = [], {}, {}, {}

    def keep(self, eng, slot, draw, res):
        gd = eng.game_data(slot, res)
        gd["slot"] = draw                                            # _compare_with_oracle's key into the draws
        self.games.append(gd)
        self.trees[draw], self.tables[draw], self.results[draw] = eng.tree_serialize(slot), eng.root_table(slot), res.copy()

    def tree_serialize(self, draw):
        return self.trees[draw]

    def root_table(self, draw):
        return self.tables[draw]


class _ListEraser(object):
    """The engine's net, which overwrites the evaluation list with -1 before it answers: by then sgo_collect has turned the list
    into the network input (the tensor route; nothing else reads the list), and the step that follows writes the next list into
    erased memory -- so the rows that step wrote can be COUNTED, not taken from n_eval."""

    def __init__(self, net):
        self.net, self.name, self.view = net, net.name, None

    def predict_on_batch(self, x):
        self.view.fill_(-1)
        return self.net.predict_on_batch(x)


def _check_list(lst, st, G, private, n_private_blocks):
    """the evaluation list after a step: as many rows as n_eval says and none behind them, no block twice, and -- on the rows that
    name private blocks, where block // private_per_game is the game -- game-major order and at most E rows per game.  Returns the
    rows per game (private rows)."""
    n = int(st.n_eval)
    assert int((lst >= 0).sum()) == n and (lst[:n] >= 0).all(), (n, int((lst >= 0).sum()))
    assert st.n_active + st.n_done == G, (st.n_active, st.n_done)
    rows = lst[:n]
    assert len(np.unique(rows)) == n
    own = rows[rows < n_private_blocks]
    games = own // private
    assert (np.diff(games) >= 0).all()
    counts = np.bincount(games, minlength=G)
    assert counts.max(initial=0) <= E
    return counts


def _population(G, seed, **pool):
    """Runs G slots to the end with restarts; returns what the tests assert on."""
    import torch
    from sejonggo_amd.engine import SelfPlayEngine
    net = _net()
    D = G + G // 3                                                   # draws: one per slot and one restart for a third of them
    rng = np.random.RandomState(seed)
    noises, uni = rng.dirichlet([0.03] * A, size=D), rng.random_sample((D, NM))
    resign = [None if rng.rand() < 0.67 else float(rng.uniform(-1, 0.2)) for _ in range(D)]
    eraser = _ListEraser(net)
    eng = SelfPlayEngine(eraser, size=S, n_games=G, sims=SIMS, energy=E, stop_exploration=STOP, num_moves=NM, komi=5.5,
                         symmetry="identity", **pool)
    try:
        assert not eng.packed and not eng.graph
        info = eng.pool_info()
        private = info["private_per_game"]
        eraser.view = view = eng._index_view()
        view.fill_(-1)
        sample, runs = _sample(G)
        wanted = np.zeros(G, bool)
        wanted[sample] = True
        eng.start_games(np.arange(G), noises=noises[:G], uniforms=uni[:G], resign=resign[:G], ids=list(range(G)))
        draw_of, live, nxt = np.arange(G), np.ones(G, bool), G
        fin = _Finished()
        unseen, seen_at = list(M.EVAL_LIST_FAULTS), {}
        just_started, coexist, n_lists, n_games, steps = np.zeros(0, np.int64), [], 0, 0, 0
        for step in range(400):
            st = eng.step()
            steps += 1
            lst = view.cpu().numpy()
            counts = _check_list(lst, st, G, private, G * private)
            n_lists += st.n_eval > 0
            if not pool and st.n_eval > 0:
                assert counts.sum() == st.n_eval
                # the recorded request counts through the model: the list is the model's, and a switch that moves rows shows on it
                t = M.from_counts(counts, E, lst[:st.n_eval])
                good = M.compact(t)
                assert np.array_equal(good["eval_idx"], lst[:st.n_eval]) and good["n_eval"] == st.n_eval
                for f in list(unseen):
                    if "eval_idx" in M.differs(M.compact_block(t, f), good, ("eval_idx",)):
                        unseen.remove(f)
                        seen_at[f] = step
            # the slots (re)started before this step ask for their root now: one row each.  A game with two rows or more asks for
            # leaves (a root request is one row), so both kinds stand in this list
            if not pool and len(just_started) and len(just_started) < G:
                assert (counts[just_started] == 1).all(), step
                if counts.max() >= 2:
                    coexist.append(step)
            just_started = np.zeros(0, np.int64)
            if st.n_records > 0:
                eng.drain()
            if st.n_done > 0:
                res = eng.results()
                done = np.flatnonzero((res["done"] == 1) & live)
                assert (res["done"] >= 0).all()
                for s in done:
                    if wanted[s]:
                        fin.keep(eng, int(s), int(draw_of[s]), res[s])
                    eng.records[int(s)] = []
                n_games += len(done)
                live[done] = False
                again = [int(s) for s in done if s % 3 == 0][:D - nxt]
                if again:
                    draws = list(range(nxt, nxt + len(again)))
                    eng.start_games(again, noises=noises[draws], uniforms=uni[draws], resign=[resign[d] for d in draws], ids=draws)
                    draw_of[again], live[again] = draws, True
                    nxt += len(again)
                    just_started = np.array(again, np.int64)
            if not live.any():
                break
        assert not live.any() and nxt == D and n_games == D
        out = {"fin": fin, "sample": sample, "runs": runs, "unseen": unseen, "seen_at": seen_at, "coexist": coexist, "steps": steps,
               "lists": n_lists, "draws": (uni, noises, resign), "net": net, "status": (st.n_active, st.n_done, st.error)}
        if pool:
            torch.cuda.synchronize()
            out["pool"] = _pool_accounting(eng)
        return out
    finally:
        eng.close()


def _against_the_oracle(out):
    """every kept game: boards, policy rows, values, tree and root table through _compare_with_oracle; length and result here"""
    from oracle import oracle as ora
    from tests.test_gpu_engine import _compare_with_oracle
    fin, (uni, noises, resign), net = out["fin"], out["draws"], out["net"]
    draws = sorted(fin.trees)
    _compare_with_oracle(fin, fin.games, draws, S, SIMS, E, STOP, NM, uni, noises, net, resign=resign)
    lengths = np.zeros(NM + 1, np.int64)
    for d in draws:
        g = ora.Game(S, SIMS, E, STOP, NM, uniforms=uni[d], noises=noises[d:d + 1], resign=resign[d]).run(net)
        o, r = g.result(), fin.results[d]
        assert (g.n_moves, o["end_reason"], o["winner"], o["black"], o["white"], o["last_player"]) == (
            r["n_moves"], r["end_reason"], r["winner"], r["black"], r["white"], r["last_player"]), d
        lengths[g.n_moves] += 1
    return len(draws), lengths


@pytest.mark.parametrize("G", [1025, 2050, 3073])
def test_selfplay_equals_the_oracle(L, G):
    """case a.  Counted conditions on the inputs: the sampled slots hold at least 200 complete runs (all of them at 1 025), every
    length of game from 0 to 3 moves occurs, root and leaf requests stand in one list on at least 5 steps (counted from the restart
    schedule), and the recorded request counts make each of the three switches of the model that move rows of the evaluation list
    change that list on some step."""
    out = _population(G, 1000 + G)
    per = M.per_thread(G)
    assert out["runs"] >= min(200, G // per) and len(out["sample"]) >= (G if G == 1025 else 200 * per)
    assert all(s in out["sample"] for s in (0, 1023, 1024, G - 1))
    n, lengths = _against_the_oracle(out)
    print("MANY_SLOTS G=%d steps=%d lists=%d slots_checked=%d games_checked=%d lengths=%s coexisting_steps=%s switches_seen_at=%s"
          % (G, out["steps"], out["lists"], len(out["sample"]), n, lengths.tolist(), out["coexist"], out["seen_at"]))
    assert n >= len(out["sample"]) and (lengths > 0).all(), lengths
    assert out["unseen"] == [], out["unseen"]
    assert len(out["coexist"]) >= 5, out["coexist"]
    assert out["status"] == (0, G, 0)


def _pool_accounting(eng):
    """at the end of the run: every shared block is free, on the return list or behind one overflow id; one audit of everything"""
    info = eng.pool_info()
    dumps, pstate = BA.dump_engine(eng)
    v = BA.audit(dumps, pstate)
    held = sum(int(np.sum(d["ovfMap"] >= 0)) for d in dumps.values())
    return {"info": info, "violations": list(v), "held": held, "ctl": pstate["poolCtl"], "pool_blocks": pstate["pool_blocks"]}


def test_selfplay_from_the_shared_pool(L):
    """case b: G = 1 025, 10 private blocks per game, a pool of 900 blocks per game.  Every slot against the oracle; the pool
    accounting is exact and one audit of the whole context is clean."""
    G = 1025
    pool = G * 900
    out = _population(G, 2000 + G, blocks_per_game=10, shared_blocks=pool)
    n, lengths = _against_the_oracle(out)
    p = out["pool"]
    print("MANY_SLOTS pool G=%d steps=%d games_checked=%d lengths=%s held=%d free=%d low_water=%d" % (
        G, out["steps"], n, lengths.tolist(), p["held"], p["info"]["shared_free"], p["info"]["shared_free_low_water"]))
    assert n >= G and (lengths > 0).all()
    assert p["info"]["private_per_game"] == 10 and p["info"]["shared_blocks"] == p["pool_blocks"] == pool
    assert p["violations"] == [], p["violations"][:10]
    assert p["ctl"][0] + p["ctl"][1] + p["held"] == pool and p["held"] > 0                # free + returned + held: every block
    assert p["info"]["shared_free"] == p["ctl"][0] and 0 < p["info"]["shared_free_low_water"] < pool - G     # the trees lived on it
    assert out["status"] == (0, G, 0)


def test_status_folds_over_runs_and_waves(L):
    """case c: G = 2 050 (three games per thread), every move sampled.  Slots 601 and 602 -- the second and third game of thread
    200's run, wave 3 -- and 2 040 -- the first game of thread 680's run, wave 10 -- start with ONE uniform draw and fail with
    SGO_ERR_DRAWS at their second move.  error_game is 601 and error -202; every other game finishes, and equals the oracle on the
    runs around the failing slots, the first and last slots and 100 random ones; n_done is all 2 050 slots (a failed slot rests in
    PH_DONE) with exactly 2 047 finished by their results; n_active + n_done is G after every step."""
    from sejonggo_amd.engine import SelfPlayEngine
    from tests.test_gpu_engine import _compare_with_oracle
    G = 2050
    per = M.per_thread(G)
    bad = [200 * per + 1, 200 * per + 2, 680 * per]
    assert per == 3 and bad == [601, 602, 2040] and M.run_of(G, 200) == (600, 603) and M.run_of(G, 680)[0] == 2040
    assert 200 // M.WAVE == 3 and 680 // M.WAVE == 10 == _last_wave_start(G) // M.WAVE
    net = _net()
    rng = np.random.RandomState(77)
    noises, uni = rng.dirichlet([0.03] * A, size=G), rng.random_sample((G, NM))
    rest = np.setdiff1d(np.arange(G), bad)
    eng = SelfPlayEngine(net, size=S, n_games=G, sims=SIMS, energy=E, stop_exploration=NM, num_moves=NM, komi=5.5,
                         symmetry="identity", raise_on_error=False)
    try:
        eng.start_games(rest, noises=noises[rest], uniforms=uni[rest])
        eng.start_games(bad, noises=noises[bad], uniforms=uni[bad, :1])
        first_error = None
        for step in range(400):
            st = eng.step()
            assert st.n_active + st.n_done == G, step
            assert (st.error_game, st.error) == (-1, 0) or (st.error_game in bad and st.error == SGO_ERR_DRAWS), (st.error_game, st.error)
            if st.error and first_error is None:
                first_error = (step, st.error_game)
            if st.n_records > 0:
                eng.drain()
            if st.n_active == 0:
                break
        assert (st.n_active, st.n_done) == (0, G)
        assert (st.error_game, st.error) == (bad[0], SGO_ERR_DRAWS), (st.error_game, st.error, first_error)
        res = eng.results()
        assert (res["done"][bad] == SGO_ERR_DRAWS).all() and (res["done"][rest] == 1).all() and int((res["done"] == 1).sum()) == G - 3
        assert st.n_done == int((res["done"] != 0).sum())
        for s in bad:
            b = eng.block_state(s, blocks=False)
            assert (b["phase"], b["error"]) == (PH_DONE, SGO_ERR_DRAWS) and len(eng.records[s]) == 1, s
        sample = set([0, 1, 1023, 1024, 2049]) | set(range(597, 609)) | set(range(2034, 2046)) | set(int(s) for s in rng.choice(rest, 100, False))
        sample = sorted(sample - set(bad))
        games = [eng.game_data(s, res[s]) for s in sample]
        _compare_with_oracle(eng, games, sample, S, SIMS, E, NM, NM, uni, noises, net, resign=[None] * G)      # two passes end a game early
        print("MANY_SLOTS folds: first error at step %s, %d steps, %d slots against the oracle" % (first_error, step + 1, len(sample)))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- sessions
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


def _xy(a):
    return (a % S, a // S) if a < S * S else (0, S)


def test_sessions_in_one_call_each(env):
    """case d: SessionEngine(n_games=1 100), sims 16, energy 4.  open, setup (seeded legal lists of 0 .. 12 moves with passes and
    out-of-turn colours), analyze, report, play of the most visited child and genmove: ONE call each over a shuffled list of all
    1 100 slots.  Every list position from 1 024 up and 60 below meet the host engine gtp.SejongGoEngine on the same net: value and
    prior row of the analysis, the tree after it, the report's counts, best children and principal variations, the generated move
    with its value and policy row, the tree and the board after it.  Then the all-or-none rule of the arming: one slot that is no
    holding session (it played an ordinary one-ply game to its end) at list position 1 050, then at 5 -- SGO_ERR_STATE, nothing
    armed: the next step lists no evaluation and the phases at list positions 0, 1 023, 1 024 and 1 099 are unchanged."""
    from sejonggo_amd import _lib, gtp, predicting_queue_worker as pq
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.play import game_init
    from tests.test_gpu_session import _tree_hash
    from tests.test_gpu_session_analysis import _order, _walk
    from tests.test_gpu_session_setup import _random_list
    G, sims, TOP, DEPTH = 1100, 16, 5, 8
    net = _net()
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': sims, 'ENERGY': E, 'KOMI': 5.5, 'GPUs': [0]})
    rng = np.random.RandomState(1100)
    order = rng.permutation(G).astype(np.int32)                      # list position -> slot
    assert (order != np.arange(G)).mean() > 0.99
    lists = [_random_list(rng, S, int(n)) for n in rng.randint(0, 13, size=G)]       # by list position
    assert set(len(a) for a, _ in lists) == set(range(13))
    checked = sorted(set(range(1024, G)) | set(int(i) for i in rng.choice(1024, size=60, replace=False)))
    assert len(checked) == G - 1024 + 60
    pq.set_model_factory(lambda kind: net)
    host = gtp.SejongGoEngine(sims, game_init(S)[0])
    eng = SessionEngine(net, size=S, n_games=G, sims=sims, energy=E, komi=5.5, symmetry="identity", num_moves=1)
    try:
        eng.open(order)
        status, fail_at = eng.setup(order, [a for a, _ in lists], [c for _, c in lists])
        assert not status.any() and (fail_at == -1).all()
        analysis = eng.analyze(order, sims)
        assert all(a == SGO_ACTION_ANALYSIS for a, _, _ in analysis)
        rep = eng.report(order, top=TOP, depth=DEPTH)
        assert not rep["status"].any() and (rep["root_count"] == sims).all() and (rep["top_action"][:, 0] >= 0).all()
        best = rep["top_action"][:, 0].copy()
        # the host engine on the checked positions, up to its own analysis
        hosts = {}
        for i in checked:
            host.board, host.player = game_init(S)
            host.mcts_tree, host.move = None, 1
            for a, col in zip(*lists[i]):
                host.play(int(host.board[0, 0, 0, -1]) if col == 0 else col, *_xy(a), update_tree=False)
            slot = int(order[i])
            assert np.array_equal(eng.board(slot), host.board), i
            hp, hv = host.analyze(sims)
            _, dv, dp = analysis[i]
            assert np.float32(dv).tobytes() == np.float32(np.asarray(hv).reshape(-1)[0]).tobytes(), i
            tree = host.mcts_tree
            want = np.zeros(A)
            for a, child in tree['subtree'].items():
                want[a] = child['p']
            assert np.asarray(dp, np.float64).tobytes() == want.tobytes(), i
            assert _tree_hash(eng.tree_dict(slot)) == _tree_hash(tree), i
            want_top, want_pv, _ = _walk(tree, TOP, DEPTH)
            assert np.array_equal(rep["top_action"][i], want_top) and np.array_equal(rep["pv"][i], want_pv), i
            counts = np.full(A, -1, np.int32)
            for a, child in tree['subtree'].items():
                counts[a] = child['count']
            assert np.array_equal(rep["N"][i], counts) and rep["n_children"][i] == len(tree['subtree']), i
            assert rep["to_play"][i] == host.board[0, 0, 0, -1] and _order(tree['subtree'])[0][0] == best[i], i
            hosts[i] = (host.board, host.player, host.mcts_tree, host.move)
        # the most visited child on every slot, then a move of the engine's own on every slot
        assert not eng.play(order, best).any()
        moves = eng.genmove(order)
        followed = 0
        for i in checked:
            host.board, host.player, host.mcts_tree, host.move = hosts[i]
            host.play(int(host.board[0, 0, 0, -1]), *_xy(int(best[i])))
            followed += bool(host.mcts_tree and host.mcts_tree['subtree'])
            hx, hy, hp, hv, _, _ = host.genmove(int(host.board[0, 0, 0, -1]))
            a, dv, dp = moves[i]
            slot = int(order[i])
            assert _xy(a) == (hx, hy), i
            assert np.float32(dv).tobytes() == np.float32(np.asarray(hv).reshape(-1)[0]).tobytes(), i
            assert np.asarray(dp, np.float64).tobytes() == np.asarray(hp, np.float64).tobytes(), i
            assert np.array_equal(eng.board(slot), host.board) and _tree_hash(eng.tree_dict(slot)) == _tree_hash(host.mcts_tree), i
        assert followed > len(checked) // 2                          # the play followed into the analysed tree
        # all or none.  The slot at list position 1 050 plays an ordinary game of one ply to its end: no session, and it asks for nothing
        odd = int(order[1050])
        eng.start_games([odd])
        for _ in range(60):
            st = eng.step()
            if st.n_records > 0:
                eng.drain()
            if st.n_active == 0:
                break
        assert st.n_active == 0 and eng.results([odd])[0]["done"] == 1 and eng.block_state(odd, blocks=False)["phase"] == PH_DONE
        watch = [int(order[i]) for i in (0, 1023, 1024, 1099)]          # the swap below leaves these list positions as they are
        for at in (1050, 5):
            lst = order.copy()
            lst[1050], lst[at] = lst[at], lst[1050]                  # the odd slot at list position `at`
            assert lst[at] == odd and sorted(lst) == list(range(G))
            assert [int(lst[i]) for i in (0, 1023, 1024, 1099)] == watch and odd not in watch
            before = [eng.block_state(s, blocks=False)["phase"] for s in watch]
            assert before == [PH_HOLD] * 4
            for arm in (eng.arm, lambda slots: eng.arm_analysis(slots, sims)):
                with pytest.raises(_lib.SgoError) as e:
                    arm(lst)
                assert "(%d)" % SGO_ERR_STATE in str(e.value)
                st = eng.step()
                assert st.n_eval == 0 and st.n_active == 0
                assert [eng.block_state(s, blocks=False)["phase"] for s in watch] == before
        v = BA.audit(*BA.dump_engine(eng, full=[int(order[i]) for i in (0, 5, 1023, 1024, 1050, 1099)]))
        assert v == [], v[:10]
    finally:
        eng.close()
        host.close()
        pq.set_model_factory(None)
        pq.destroy_predicting_workers([0])
