"""CPU: the model of the chains-and-ladders reader (tests/tactics_model.py) says what include/sgo.h states on the constructed cases
(tests/tactics_cases.py), the cases reach what they were built for, and every fault switch of the model that a position can show
changes a compared value of a named case -- so a green run of tests/test_gpu_tactics.py means something."""
import numpy as np
import pytest

from tests import tactics_cases as TC
from tests import tactics_model as T

# fault -> (board size, case name): the case whose compared values the switch changes
NOTICED_BY = {
    "desc_order": (9, "ladder_b"),
    "no_counter": (5, "counter_capture_b"),
    "ko_wrong_side": (5, "ko_b"),
    "no_root_ko": (5, "ko_w"),
    "root_ko_always": (5, "ko_b"),
    "depth_off_by_one": (19, "ladder_deep_b"),
    "shared_counter": (9, "ladder_atari_w"),
    "flag_as_stone": (5, "empty_w"),
    "padding_read": (5, "suicide_b"),
    "anchor_highest": (7, "snapback_b"),
}


def _row(S, name, fault=None):
    names, recs = TC.case_records(S)
    i = names.index(name)
    if fault is None:
        m = TC.case_model(S)
        return m["libs"][i], m["n_chains"][i], m["rows"][i], m["depths"][i]
    m = T.tactics(S, recs[i:i + 1], fault=fault)
    return m["libs"][0], m["n_chains"][0], m["rows"][0], m["depths"][0]


def _chain(S, name, anchor):
    rows, depths = _row(S, name)[2:]
    k = [int(r[0]) for r in rows].index(anchor)
    return T_row(rows[k]), depths[k]


def T_row(r):
    return dict(zip(("anchor", "colour", "size", "liberties", "status", "attack_move", "defend_move", "nodes"), (int(v) for v in r)))


@pytest.mark.parametrize("fault", sorted(NOTICED_BY))
def test_fault_switch_changes_a_named_case(fault):
    S, name = NOTICED_BY[fault]
    good, bad = _row(S, name), _row(S, name, fault)
    same = np.array_equal(good[0], bad[0]) and good[1] == bad[1] and np.array_equal(good[2], bad[2])
    assert not same, (fault, name)


def test_the_switches_no_position_can_show():
    """suicide_not_skipped: an allowed move keeps a liberty, so the switch changes nothing anywhere (checked on every case of
    three sizes).  libs_unsaturated: no chain of a supported board has 255 liberties; shown on the saturation alone."""
    assert set(T.FAULTS) == set(NOTICED_BY) | {"suicide_not_skipped", "libs_unsaturated"}
    for S in (5, 7, 9):
        names, recs = TC.case_records(S)
        good, bad = TC.case_model(S), T.tactics(S, recs, fault="suicide_not_skipped")
        assert all(np.array_equal(a, b) for a, b in zip(good["rows"], bad["rows"]))
    assert T.saturate(254) == 254 and T.saturate(255) == 255 and T.saturate(300) == 255 and T.saturate(300, "libs_unsaturated") == 44
    assert max(int(TC.case_model(S)["libs"].max()) for S in T.SIZES) < 255


def test_ladders_reach_what_they_were_built_for():
    C, E = T.A_CAPTURED, T.D_RAN
    for S, depth_a, nodes in ((9, 19, 25), (19, 59, 75)):
        t = 3 * S + 3
        row, d = _chain(S, "ladder_b", t)
        # the ladder works: A captures by the atari from below after chasing to the edge; the defender first extends and is safe
        assert row["status"] == C | E and row["attack_move"] == 4 * S + 3 and row["defend_move"] == 3 * S + 4
        assert row["nodes"] == nodes and d[0] == depth_a and row["liberties"] == 2 and row["size"] == 1
        assert _chain(S, "ladder_w", t)[0] == row                                        # no ko at the root: the side to move is no matter
        brk, db = _chain(S, "ladder_breaker_b", t)
        assert brk["status"] == 0 and brk["attack_move"] == -1 and 0 < db[0] < depth_a   # the breaker saves it, found deep in the tree
        hit, dh = _chain(S, "ladder_into_attacker_b", t)
        assert hit["status"] == C | E and dh[0] < depth_a                                # caught earlier, against the attacker's stone
        dead, dd = _chain(S, "ladder_atari_b", t)
        assert dead["status"] == C | E | T.D_CAPTURED and dead["defend_move"] == -1 and dd[1] == depth_a - 1 and dead["liberties"] == 1
    deep, dd = _chain(19, "ladder_deep_b", 60)
    assert deep["status"] == T.A_UNKNOWN and deep["nodes"] == 126 and dd[0] == T.MAX_DEPTH and deep["attack_move"] == -1
    # beside the ladder in one wavefront: chain slots 2 and 3 of ladder_beside
    rows = _row(19, "ladder_beside_b")[2]
    assert [int(r[0]) for r in rows] == [0, 18, 37, 60] and rows[3, 7] == 75


def test_small_cases():
    C, D, E = T.A_CAPTURED, T.D_CAPTURED, T.D_RAN
    S = 5
    # saved only by the counter-capture at (1,1); without it the model calls the stone dead
    row, _ = _chain(S, "counter_capture_b", 0)
    assert row["status"] == C | E and row["defend_move"] == S + 1
    bad = T_row(_row(S, "counter_capture_b", "no_counter")[2][0])
    assert bad["status"] == C | E | D and bad["defend_move"] == -1
    # the ko: white to move may not take (2,1) back at (1,1); with black to move the question is not ko-restricted
    t = S + 2
    assert _chain(S, "ko_w", t)[0]["status"] == E and _chain(S, "ko_w", t)[0]["attack_move"] == -1
    assert _chain(S, "ko_b", t)[0]["status"] == C | E and _chain(S, "ko_b", t)[0]["attack_move"] == S + 1
    # ... and black's chain on (1,0): white takes at (1,1) inside the tree, black's retake at (2,1) is the ko, so it is caught
    assert _chain(S, "ko_b", 1)[0]["status"] & C and not _chain(S, "ko_w", 1)[0]["status"] & C
    # the eye: the attacker's (0,0) is suicide and not allowed, the outside liberty (1,2) catches three stones
    row, _ = _chain(S, "suicide_b", 1)
    assert row["size"] == 3 and row["status"] & C and row["attack_move"] == 2 * S + 1
    # snapback at 7x7: the throw-in (2,2) is the attack, and the seven stones are dead whoever moves first
    row, _ = _chain(7, "snapback_w", 8)
    assert row["size"] == 7 and row["status"] == C | D | E and row["attack_move"] == 16 and row["defend_move"] == -1
    # 5x5, white to move: the flag shares the only plane word with the stones and is no stone
    assert _row(5, "empty_w")[1] == 0 and _row(5, "empty_w", "flag_as_stone")[1] == 1
    # more chains than any table holds
    assert _row(19, "lattice_b")[1] == 272 and len(_row(19, "lattice_b")[2]) == 128


def test_golden_positions_stay_inside_the_budgets():
    """Conditions on the inputs of the GPU test, every fourth position of the five golden 19x19 games (412 positions): at most
    0.5 % of the model's queries end unknown and no position lists more than 128 chains.  The model's own count on the committed
    games: 16 980 queries, 4 unknown (all at the node cap, 513 nodes), at most 65 listed chains.  Position 260 holds the query that
    visits depth 80 without passing it: the reader that gives up one ply early ends it sooner."""
    g = TC.golden_model()
    rows = np.concatenate(g["rows"])
    queries = len(rows) + int(((rows[:, 4] & T.D_RAN) != 0).sum())
    unknown = int(((rows[:, 4] & T.A_UNKNOWN) != 0).sum() + ((rows[:, 4] & T.D_UNKNOWN) != 0).sum())
    assert queries > 10000 and 0 < unknown <= 0.005 * queries
    assert int(g["n_chains"].max()) <= T.MAX_CHAINS
    capped = rows[(rows[:, 4] & (T.A_UNKNOWN | T.D_UNKNOWN)) != 0]
    assert (capped[:, 7] >= T.MAX_NODES + 1).all()
    assert int(np.concatenate(g["depths"]).max()) == T.MAX_DEPTH and int(g["depths"][260].max()) == T.MAX_DEPTH
    bad = T.tactics(19, TC.golden_records()[260:261], fault="depth_off_by_one")
    assert not np.array_equal(bad["rows"][0], g["rows"][260])
