"""GPU: the tree-block accounting of the real engine, audited after every step (tests/block_audit.py on the dumps of
sgo_debug_block_state / sgo_debug_pool_state).  Moves and serialised trees cannot show a leaked block, a block that is free and
linked at once, or a shared block held twice -- block ids never enter them; the audit does, at the step
where it happens.  tests/test_block_audit.py proves on a model of the allocator that the audit reports such faults.

Every test prints one BLOCK_AUDIT line (audits, most blocks in use / in flight, deepest chain, most overflow ids backed)."""
import numpy as np
import pytest

from tests import block_audit as BA
from tests.helpers import load, PackedProbe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def _audit(eng, tally, full=None):
    games, pool = BA.dump_engine(eng, full)
    v = tally.add(BA.audit(games, pool), games)
    assert v == [], v[:10]
    return games, pool


def _selfplay(S, G, sims, E, nm, seed, stop=4, **kw):
    from sejonggo_amd.engine import SelfPlayEngine
    from sejonggo_amd.stub_nets import make_stub
    rng = np.random.RandomState(seed)
    noises = rng.dirichlet([0.03] * (S * S + 1), size=G)
    uni = rng.random_sample((G, nm))
    eng = SelfPlayEngine(make_stub("hash", S), size=S, n_games=G, sims=sims, energy=E, stop_exploration=stop, num_moves=nm,
                         komi=5.5, symmetry="identity", **kw)
    eng.start_games(np.arange(G), noises=noises, uniforms=uni)
    return eng, noises, uni


def _run_audited(eng, tally, max_steps=4000):
    for _ in range(max_steps):
        st = eng.step()
        _audit(eng, tally)
        if st.n_records >= eng.G:
            eng.drain()
        if st.n_active == 0:
            break
    assert st.n_active == 0
    eng.drain()
    return st


def test_a_whole_golden_game_audits_clean_after_every_step(L):
    """(a) async_05: 5x5, 64 sims, 16 leaves per round, 38 moves, 24 rounds without a best leaf, default pool sizes.  The oracle
    reaches a chain of 37 expanded nodes below the root in this game (tests/test_block_audit.py pins that on the CPU)."""
    from sejonggo_amd.engine import SelfPlayEngine
    from sejonggo_amd.stub_nets import make_stub
    z = load("async_05.npz")
    S, nm = int(z["size"]), int(z["num_moves"])
    eng = SelfPlayEngine(make_stub(bytes(z["net"]).decode(), S), size=S, n_games=1, sims=int(z["sims"]), energy=int(z["energy"]),
                         stop_exploration=int(z["stop_exploration"]), num_moves=None if nm < 0 else nm, komi=float(z["komi"]),
                         symmetry="identity")
    uni = np.zeros((1, max(1, eng.max_moves)))
    uni[0, :len(z["uniforms"])] = z["uniforms"]
    eng.start_games([0], noises=z["noises"][:1], uniforms=uni)
    tally = BA.Tally()
    _audit(eng, tally)                                   # right after k_start
    _run_audited(eng, tally)
    print(tally.line("golden_5x5"))
    res = eng.results()
    gd = eng.game_data(0, res[0])
    assert len(gd["moves"]) == len(z["move_index"])
    for i, mv in enumerate(gd["moves"]):
        a = mv["move"][0] + S * mv["move"][1] if mv["move"][1] != S else S * S
        assert a == z["move_index"][i] and mv["policy"].tobytes() == z["move_policy"][i].tobytes(), i
        assert mv["value"].tobytes() == z["move_value"][i].tobytes(), i
    assert gd["result"] == bytes(z["result"]).decode()
    assert eng.status.total_evals == int(z["n_predict"])
    assert eng.status.none_events == int(z["none_events"]) and eng.status.none_events > 0
    assert tally.audits_fifo > 0 and tally.audits_empty > 0
    assert tally.deepest >= 33                          # the re-root's pointer jumping needs at least 6 passes
    eng.close()


B_SHAPE = dict(S=9, G=16, sims=64, E=8, nm=6)
B_POOL = 2400     # the oracle's trees of these 16 games hold 1 712 nodes at their peak (1 550 beyond the private regions)


def test_practically_every_block_from_the_shared_pool(L):
    """(b) private regions of the minimum size (E + 2): all but ten blocks of every tree are overflow ids."""
    E = B_SHAPE["E"]
    eng, _, _ = _selfplay(seed=51, blocks_per_game=E + 2, shared_blocks=B_POOL, **B_SHAPE)
    tally = BA.Tally()
    backed = np.zeros(B_SHAPE["G"], np.int64)
    for _ in range(4000):
        st = eng.step()
        games, pool = _audit(eng, tally)
        backed = np.maximum(backed, [int(np.sum(games[s]["ovfMap"] >= 0)) for s in range(B_SHAPE["G"])])
        if st.n_records >= eng.G:
            eng.drain()
        if st.n_active == 0:
            break
    print(tally.line("shared_pool_9x9"), "pool low water %d of %d" % (pool["poolCtl"][2], B_POOL))
    assert st.n_active == 0 and st.error == 0 and eng.status.total_moves == B_SHAPE["G"] * B_SHAPE["nm"]
    assert np.all(backed > 0), backed
    assert pool["poolCtl"][2] < B_POOL // 2
    eng.close()


def test_19x19_geometry(L):
    """(c) six slots per lane, twelve legal words per block."""
    eng, _, _ = _selfplay(S=19, G=4, sims=64, E=8, nm=3, seed=52, stop=30, blocks_per_game=10, shared_blocks=1024)
    tally = BA.Tally()
    games, _ = _audit(eng, tally)
    assert games[0]["NW"] == 12 and games[0]["APAD"] == 384 and games[0]["cap"] == 10
    st = _run_audited(eng, tally)
    print(tally.line("19x19"))
    assert st.error == 0 and eng.status.total_moves == 4 * 3 and tally.backed > 0
    eng.close()


def test_two_model_games_keep_two_trees(L):
    """(d) the side not to move keeps its own tree: it follows the move when it holds it, and is rebuilt from a fresh block
    otherwise.  play_move swaps the two trees before the launch ends, so either fate shows on the ROOT of the first dump after
    the move (block_audit.other_tree_fates): expanded = followed, bSlot == -2 = fresh.  The run on the MI355X printed 12
    game-audits with a tree that followed and 76 with a fresh root (8 of those after the first move of a game, when there was
    no other tree yet)."""
    from sejonggo_amd.engine import SelfPlayEngine
    from sejonggo_amd.stub_nets import make_stub
    S, sims, E, nm, G = 9, 32, 8, 12, 8
    eng = SelfPlayEngine(make_stub("hash", S), net2=make_stub("hash2", S), size=S, n_games=G, sims=sims, energy=E,
                         stop_exploration=0, num_moves=nm, symmetry="identity", blocks_per_game=12, shared_blocks=G * 300)
    eng.start_eval_games(np.arange(G), first_model=[g % 2 for g in range(G)])
    tally = BA.Tally()
    st = _run_audited(eng, tally)
    print(tally.line("two_model_9x9"), "other tree followed the move in %d game-audits, fresh in %d" % (tally.followed, tally.fresh))
    assert st.error == 0 and G <= eng.status.total_moves <= G * nm
    assert tally.followed > 0 and tally.fresh > 0 and tally.backed > 0
    eng.close()


def test_exhaustion_and_recovery(L):
    """(e) the too-small pool of test_many_games_share_one_pool_and_exhaustion_is_loud: while games fail, failed slots hold
    nothing and every shared block stays in exactly one place; restarts bring the whole pool back."""
    S, sims, E, G, nm = 9, 64, 8, 32, 10
    pool = G * 40
    eng, noises, uni = _selfplay(S=S, G=G, sims=sims, E=E, nm=nm, seed=41, blocks_per_game=10, shared_blocks=pool,
                                 raise_on_error=False)
    tally = BA.Tally()
    _run_audited(eng, tally)
    res = eng.results()
    failed = [s for s in range(G) if res[s]["done"] < 0]
    assert len(failed) > 0 and all(res[s]["done"] == -201 for s in failed) and tally.failed_slots == len(failed)
    eng.start_games(failed, noises=noises[failed], uniforms=uni[failed])
    _audit(eng, tally)
    eng.step()
    games, _ = _audit(eng, tally)
    assert all(games[s]["error"] == 0 and games[s]["phase"] != BA.PH_IDLE for s in failed)
    eng.start_games(np.arange(G), noises=noises, uniforms=uni)
    _audit(eng, tally)
    eng.step()
    _, ps = _audit(eng, tally)
    print(tally.line("exhaustion_9x9"), "failed slots %d" % len(failed))
    info = eng.pool_info()
    assert info["shared_free"] == info["shared_blocks"] == pool and ps["poolCtl"][0] == pool and ps["poolCtl"][1] == 0
    eng.close()


def test_restart_in_mid_search(L):
    """(f) half of the slots restarted while their leaves are in flight: audited with the returns still on poolRet, and after
    the step that merges them."""
    G = 8
    eng, noises, uni = _selfplay(S=9, G=G, sims=64, E=8, nm=6, seed=53, blocks_per_game=10, shared_blocks=1400)
    tally = BA.Tally()
    for _ in range(14):                                  # into the second move's search
        eng.step()
        games, _ = _audit(eng, tally)
    half = list(range(0, G, 2))
    assert all(games[s]["fifo_tail"] > games[s]["fifo_head"] and np.any(games[s]["ovfMap"] >= 0) for s in half)
    eng.start_games(half, noises=noises[half], uniforms=uni[half])
    games, pool = _audit(eng, tally)
    assert pool["poolCtl"][1] > 0                        # the returns are still on poolRet
    assert all(games[s]["fifo_tail"] == games[s]["fifo_head"] == 0 and not np.any(games[s]["ovfMap"] >= 0) for s in half)
    eng.step()
    _, pool = _audit(eng, tally)
    assert pool["poolCtl"][1] == 0
    st = _run_audited(eng, tally)
    print(tally.line("restart_mid_search"))
    assert st.error == 0
    eng.close()


def test_two_half_populations_with_captured_rounds(L):
    """(g) the shape of (b) on engine.DualEngine: two contexts on two streams, every round a captured launch chain; each half
    audited after sync(), every few rounds."""
    from sejonggo_amd.engine import DualEngine
    from sejonggo_amd.stub_nets import make_stub
    S, G, sims, E, nm = (B_SHAPE[k] for k in ("S", "G", "sims", "E", "nm"))
    rng = np.random.RandomState(51)
    noises = rng.dirichlet([0.03] * (S * S + 1), size=G)
    uni = rng.random_sample((G, nm))
    eng = DualEngine(PackedProbe(make_stub("hash", S), S), n_games=G, size=S, sims=sims, energy=E, stop_exploration=4,
                     num_moves=nm, komi=5.5, symmetry="identity", blocks_per_game=E + 2, shared_blocks=B_POOL // 2)
    assert eng.graph and eng.packed and len(eng.halves) == 2
    eng.start_games(np.arange(G), noises=noises, uniforms=uni)
    tally = BA.Tally()
    for r in range(4000):
        st = eng.step()
        if r % 4 == 3 or st.n_active == 0:
            st = eng.sync()
            for e in eng.halves:
                _audit(e, tally)
            pools = eng.pool_state()
            assert len(pools) == 2 and eng.block_state(G - 1)["cap"] == E + 2
            eng.drain()
        if st.n_active == 0:
            break
    print(tally.line("dual_engine_9x9"))
    assert st.n_active == 0 and st.error == 0 and st.total_moves == G * nm
    assert all(e.n_graph_replays > 10 for e in eng.halves) and tally.backed > 0 and tally.audits >= 10
    assert all(p["poolCtl"][2] < p["pool_blocks"] for p in pools)
    eng.close()
