"""The power of tests/compact_model.py, shown without a GPU: on small synthetic request tables at G = 1 025 and 2 050 (two and three
games per thread of the one workgroup) every fault switch changes an output, on a table named here; on a LOCKSTEP table -- every
game asks for E evaluations of one kind, nothing has failed -- two of them change nothing, which is why the cases of
tests/test_gpu_many_slots.py are staggered (resign thresholds, restarts, short last rounds, chosen failing slots); and at 1 024
games, the most any test ran before, four of the six cannot show on any table at all."""
import numpy as np
import pytest

from tests import compact_model as M

E = 4
SIZES = (1025, 2050)


def _failing(G):
    """three failing slots: the last two games of one thread's run (at three games per thread the second and the third) and the first
    game of a run in another wave"""
    per = M.per_thread(G)
    a = 200 * per + per - 2                                                  # thread 200, wave 3
    c = 680 * per if per > 2 else 500 * per                                  # wave 10 (the last that holds games at 2 050) / wave 7
    return a, a + 1, c


def _tables(G):
    g = np.arange(G)
    root = g % 3 == 0
    n_req = np.where(root, 1, (g * 7 + g // 3) % (E + 1))                     # a root request is one row; leaf requests 0 .. E
    phase = np.array([M.PH_SEARCH, M.PH_WAIT_ROOT, M.PH_DONE, M.PH_SEARCH, M.PH_HOLD, M.PH_DONE, M.PH_IDLE])[(g + g // 5) % 7]
    error = np.zeros(G, np.int64)
    a, b, c = _failing(G)
    error[[a, b, c]] = (-202, -201, -203)
    return {"staggered": M.table(G, E, n_req, np.where(root, M.ROOT, M.LEAF), g % 2, phase, error),
            "leaf_only": M.table(G, E, (g * 7 + g // 3) % (E + 1), M.LEAF, 0, phase, 0),
            "lockstep_leaf": M.table(G, E, E, M.LEAF), "lockstep_root": M.table(G, 1, 1, M.ROOT)}


@pytest.mark.parametrize("G", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2050, 3073])
def test_the_block_shape_computes_the_definition(G):
    """without a switch the scan shape gives the running sums, on every table; the lists are dense and name every request once"""
    for name, t in _tables(max(G, 1025)).items():
        t = {k: (v[:G] if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        t["G"] = G
        want, got = M.compact(t), M.compact_block(t)
        assert M.differs(got, want) == [], (G, name)
        assert len(want["eval_idx"]) == want["n_eval"] == t["n_req"].sum() and (want["eval_idx"] != M.FILL).all()
        assert np.array_equal(want["eval_idx"] // 64, np.repeat(np.arange(G), t["n_req"]))                  # game-major
        assert len(want["leaf_out"]) == want["n_leaf"] and want["n_leaf"] + want["n_root"] == want["n_eval"]
        assert np.array_equal(want["leaf_out"], want["eval_idx"][np.repeat(t["req_kind"], t["n_req"]) == M.LEAF])
        assert np.array_equal(want["leaf_in"], want["leaf_out"] + 1000000)


# what each switch must change on the staggered table, at the least
SHOWS = {"one_per_thread": {"eval_base", "eval_idx", "n_eval", "n_leaf", "n_active"},      # at 1 025 the one lost game: a searching leaf game
         "run_base_stuck": {"eval_base", "list_base", "eval_idx", "leaf_out"},
         "wave_total_last": {"eval_base", "list_base", "eval_idx", "n_eval", "n_leaf", "n_root"},
         "kinds_share_scan": {"list_base", "leaf_in", "leaf_mv", "leaf_out"},
         "err_last": {"error_game", "error"},
         "fold_first_only": {"n_active", "n_done"}}


@pytest.mark.parametrize("G", SIZES)
def test_every_switch_shows_on_the_staggered_table(G):
    t = _tables(G)["staggered"]
    good = M.compact(t)
    a, b, c = _failing(G)
    assert (good["error_game"], good["error"]) == (a, -202) and a < b < c
    per = M.per_thread(G)
    assert M.run_of(G, 200)[0] <= a and b < M.run_of(G, 200)[1] and M.run_of(G, c // per)[0] == c and a // per // 64 == 3 != c // per // 64
    assert good["n_leaf"] > 0 and good["n_root"] > 0 and 0 < good["n_active"] < G and 0 < good["n_done"] < G
    for fault in M.FAULTS:
        d = set(M.differs(M.compact_block(t, fault), good))
        assert SHOWS[fault] <= d, (G, fault, sorted(d))
    # err_last, one condition at a time: two failing games in ONE run; two in different waves
    for keep, wrong in (((a, b), b), ((a, c), c)):
        one = dict(t, error=np.zeros(G, np.int64))
        one["error"][list(keep)] = -202
        assert M.compact(one)["error_game"] == a and M.compact_block(one, "err_last")["error_game"] == wrong, keep


@pytest.mark.parametrize("G", SIZES)
def test_what_a_lockstep_table_cannot_see(G):
    """every game E requests of one kind, nothing failed: a wrong list_base of the OTHER kind and a wrong error fold change nothing;
    the leaf-only table with uneven counts is blind to the shared scan too.  The four others show even here."""
    tables = _tables(G)
    for name in ("lockstep_leaf", "lockstep_root"):
        good = M.compact(tables[name])
        blind = [f for f in M.FAULTS if M.differs(M.compact_block(tables[name], f), good) == []]
        assert blind == ["kinds_share_scan", "err_last"], (G, name, blind)
    good = M.compact(tables["leaf_only"])
    blind = [f for f in M.FAULTS if M.differs(M.compact_block(tables["leaf_only"], f), good) == []]
    assert blind == ["kinds_share_scan", "err_last"], (G, blind)
    # and a lockstep table shows the three switches of the evaluation list by its length or by unwritten rows alone
    for f in M.EVAL_LIST_FAULTS:
        bad = M.compact_block(tables["lockstep_leaf"], f)
        assert bad["n_eval"] < G * E or (bad["eval_idx"] == M.FILL).any(), (G, f)


def test_at_1024_games_four_switches_cannot_show():
    """one game per thread: no run has a second game.  Only the shared scan of the two kinds and the fold over the WAVES of err_last
    are reachable"""
    for name, t in _tables(1025).items():
        t = {k: (v[:1024] if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        t["G"] = 1024
        good = M.compact(t)
        seen = [f for f in M.FAULTS if M.differs(M.compact_block(t, f), good)]
        assert seen == (["kinds_share_scan", "err_last"] if name == "staggered" else []), (name, seen)


def test_recorded_counts_make_a_table():
    """from_counts: the rows per game of a list read back from the device, with the listed blocks as payload, give that list back"""
    rng = np.random.RandomState(5)
    counts = rng.randint(0, E + 1, size=2050)
    blocks = np.repeat(np.arange(2050) * 40, counts) + rng.randint(0, 40, size=counts.sum())
    t = M.from_counts(counts, E, blocks)
    out = M.compact(t)
    assert np.array_equal(out["eval_idx"], blocks) and out["n_eval"] == counts.sum() == out["n_leaf"]
    for f in M.EVAL_LIST_FAULTS:
        assert "eval_idx" in M.differs(M.compact_block(t, f), out), f
